"""float64 torch.autograd restatement of the sequence loss's training forward (test helper; never imported by the product): the
featurizer and the three encoder layers as tests/test_gpu_finetune.py restates them for the ddG path (oracle layer functions, dropout
multipliers given), then the ORDER-MASKED decoder and the output layer, written from the formulas of include/tmpnn.h:

    vis(i, k)  = ranks[E_idx[i, k]] < ranks[i]                                   (equal ranks: not visible)
    in_l(i, k) = mask_i * [ h_V^l_i | h_E_ik | vis * h_S_j | (vis ? h_V^l_j : h_V^enc_j) ]
    log_probs  = log_softmax(W_out h_V^dec3 + b)
"""
import numpy as np
import torch
import torch.nn.functional as F


def ones_mult(L, K):
    """Dropout multipliers of a run without dropout, in site order ([L,128] node sites, [L K,128] edge sites)."""
    return [np.ones((L * (K if s < 9 and s % 3 == 2 else 1), 128)) for s in range(15)]


def split_masks(flat, L, K):
    """keep_out of tmpnn_seqloss_forward -> the 15 sites' [rows,128] arrays; an edge site holds its L K rows at the start of its part."""
    from thermompnn_amd.finetune import mask_offsets
    off = mask_offsets(L)
    out = []
    for s in range(15):
        rows = L * K if s < 9 and s % 3 == 2 else L
        out.append(flat[off[s]:off[s] + rows * 128].reshape(rows, 128))
    return out


def log_probs_f64(sd, X, S, mask, ridx, cenc, E_idx, ranks, site_mult=None, dtype=torch.float64):
    """-> (log_probs [L,21] with a graph, W: {name: leaf}) for ProteinMPNN's state dict ``sd`` (no prefix), evaluated in ``dtype``:
    float64 is the restatement; float32 is the same mathematics at the device's precision, for measuring what fp32 alone costs."""
    from oracle import thermompnn_oracle as O
    W = {k: torch.as_tensor(v).detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    t = lambda a: torch.as_tensor(np.asarray(a))
    E_idx = np.asarray(E_idx)
    L, K = E_idx.shape
    X, mask = t(X).to(dtype)[None], t(mask).to(dtype)[None]
    ridx, cenc, S = t(ridx).long()[None], t(cenc).long()[None], t(S).long()[None]
    Ei = t(E_idx).long()[None]
    mult = site_mult if site_mult is not None else ones_mult(L, K)
    m = [t(x).to(dtype).view(1, L, 128) if x.shape[0] == L else t(x).to(dtype).view(1, L, K, 128) for x in mult]
    atoms = O.backbone_atoms(X)
    D_nb, _ = O.knn(atoms[O.CA], mask, K, Ei)
    blocks = [O.rbf(D_nb)]
    for a, b in O.PAIR_ORDER[1:]:
        D_ab = torch.sqrt(((atoms[a][:, :, None, :] - atoms[b][:, None, :, :]) ** 2).sum(-1) + 1e-6)
        blocks.append(O.rbf(O.gather_edges(D_ab[..., None], Ei)[..., 0]))
    d = O.positional_index(ridx, cenc, Ei)
    E_pos = F.linear(F.one_hot(d, 66).to(dtype), W["features.embeddings.linear.weight"], W["features.embeddings.linear.bias"])
    E = F.linear(torch.cat([E_pos] + blocks, -1), W["features.edge_embedding.weight"])
    hE = O.linear(O.layer_norm(E, W, "features.norm_edges"), W, "W_e")
    hV = torch.zeros(1, L, 128, dtype=dtype)
    ma = mask.unsqueeze(-1) * O.gather_nodes(mask.unsqueeze(-1), Ei).squeeze(-1)
    for l in range(3):
        p = f"encoder_layers.{l}"
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), O.cat_neighbors_nodes(hV, hE, Ei)], -1)
        msg = ma.unsqueeze(-1) * O.message(hEV, W, p)
        hV = O.layer_norm(hV + m[3 * l] * (msg.sum(-2) / 30.0), W, p + ".norm1")
        hV = O.layer_norm(hV + m[3 * l + 1] * O.ffn(hV, W, p + ".dense"), W, p + ".norm2")
        hV = mask.unsqueeze(-1) * hV
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), O.cat_neighbors_nodes(hV, hE, Ei)], -1)
        hE = O.layer_norm(hE + m[3 * l + 2] * O.message(hEV, W, p, ("W11", "W12", "W13")), W, p + ".norm3")
    hS = F.embedding(S, W["W_s.weight"])
    r = t(ranks).long()
    vis = (r[Ei[0]] < r[:, None]).to(dtype).view(1, L, K, 1)
    hS_j = vis * O.gather_nodes(hS, Ei)
    hVenc_j = O.gather_nodes(hV, Ei)
    for l in range(3):
        p = f"decoder_layers.{l}"
        hV_j = vis * O.gather_nodes(hV, Ei) + (1.0 - vis) * hVenc_j
        hESV = mask.view(1, L, 1, 1) * torch.cat([hE, hS_j, hV_j], -1)
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), hESV], -1)
        hV1 = O.layer_norm(hV + m[9 + 2 * l] * (O.message(hEV, W, p).sum(-2) / 30.0), W, p + ".norm1")
        hV = mask.unsqueeze(-1) * O.layer_norm(hV1 + m[10 + 2 * l] * O.ffn(hV1, W, p + ".dense"), W, p + ".norm2")
    logits = O.linear(hV, W, "W_out")
    return F.log_softmax(logits, -1)[0], W


def grads_f64(log_probs, W, dlp):
    """dL/dW for L = sum(log_probs * dlp) -> {name: grad in log_probs' dtype (zeros where autograd reaches none)}."""
    for v in W.values():
        v.grad = None
    (log_probs * torch.as_tensor(np.asarray(dlp)).to(log_probs.dtype)).sum().backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in W.items()}
