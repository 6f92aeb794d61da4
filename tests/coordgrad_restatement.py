"""float64 torch.autograd restatement of the sequence loss with the COORDINATES as a leaf (test helper; never imported by the
product). tests/seqloss_restatement.py carries X through numpy, so it cannot give dL / dX; this file states the same forward (oracle
layer functions, dropout multipliers given, the order-masked decoder of include/tmpnn.h) on a torch ``X`` and under the contract of the
_x backwards:

    the graph E_idx is given (a constant);
    D_max of _dist is DETACHED: D_adjust = D + (1 - mask_2D) * D_max.detach(), so pair 0 of a masked (i, j) carries no gradient.

``attach_dmax=True`` is the reference's own definition (D_max with its graph), for the cases where the two must coincide bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

from seqloss_restatement import ones_mult


def d_max_of(X, mask, dtype=torch.float64):
    """D_max of _dist [1,L,1] at the coordinates ``X`` [L,4,3], as a constant: what a finite difference around X must hold fixed."""
    ca, mask = torch.as_tensor(np.asarray(X)).to(dtype)[None, :, 1], torch.as_tensor(np.asarray(mask)).to(dtype)[None]
    m2 = mask.unsqueeze(1) * mask.unsqueeze(2)
    return (m2 * torch.sqrt(((ca.unsqueeze(1) - ca.unsqueeze(2)) ** 2).sum(3) + 1e-6)).max(-1, keepdim=True)[0]


def ca_distances(ca, mask, Ei, attach_dmax=False, d_max=None):
    """D_neighbors of _dist [1,L,K] on the given graph: mask_2D sqrt(|Ca_i - Ca_j|^2 + 1e-6) + (1 - mask_2D) D_max, D_max detached
    (or with its graph, or the given constant ``d_max``)."""
    m2 = mask.unsqueeze(1) * mask.unsqueeze(2)
    d = ca.unsqueeze(1) - ca.unsqueeze(2)
    D = m2 * torch.sqrt((d ** 2).sum(3) + 1e-6)
    if d_max is None:
        d_max = D.max(-1, keepdim=True)[0]
        if not attach_dmax:
            d_max = d_max.detach()
    return torch.gather(D + (1.0 - m2) * d_max, 2, Ei)


def log_probs_x(sd, X, S, mask, ridx, cenc, E_idx, ranks, site_mult=None, dtype=torch.float64, attach_dmax=False, d_max=None):
    """-> log_probs [L,21] with a graph over ``X`` (a torch tensor [L,4,3] of ``dtype``, usually a leaf that requires grad)."""
    from oracle import thermompnn_oracle as O
    W = {k: torch.as_tensor(v).detach().cpu().to(dtype) for k, v in sd.items()}
    t = lambda a: torch.as_tensor(np.asarray(a))
    E_idx = np.asarray(E_idx)
    L, K = E_idx.shape
    X, mask = X.to(dtype)[None], t(mask).to(dtype)[None]
    ridx, cenc, S = t(ridx).long()[None], t(cenc).long()[None], t(S).long()[None]
    Ei = t(E_idx).long()[None]
    mult = site_mult if site_mult is not None else ones_mult(L, K)
    m = [t(x).to(dtype).view(1, L, 128) if x.shape[0] == L else t(x).to(dtype).view(1, L, K, 128) for x in mult]
    atoms = O.backbone_atoms(X)
    blocks = [O.rbf(ca_distances(atoms[O.CA], mask, Ei, attach_dmax, d_max))]
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
    return F.log_softmax(logits, -1)[0]


def objective(sd, X, S, mask, ridx, cenc, E_idx, ranks, dlp, site_mult=None, dtype=torch.float64, attach_dmax=False, d_max=None):
    """The scalar sum(log_probs * dlp): its gradient with respect to X is what tmpnn_seqloss_backward_x returns for dlog_probs = dlp."""
    lp = log_probs_x(sd, X, S, mask, ridx, cenc, E_idx, ranks, site_mult, dtype, attach_dmax, d_max)
    return (lp * torch.as_tensor(np.asarray(dlp)).to(dtype)).sum()


def dX_f64(sd, X, S, mask, ridx, cenc, E_idx, ranks, dlp, site_mult=None, dtype=torch.float64, attach_dmax=False):
    """dL / dX [L,4,3] (numpy, ``dtype``) of ``objective`` at the coordinates ``X`` (array or tensor)."""
    Xl = torch.as_tensor(np.asarray(X)).detach().to(dtype).clone().requires_grad_(True)
    objective(sd, Xl, S, mask, ridx, cenc, E_idx, ranks, dlp, site_mult, dtype, attach_dmax).backward()
    return Xl.grad.detach().numpy()
