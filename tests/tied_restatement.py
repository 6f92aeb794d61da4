"""Torch restatement of tied sampling with PSSM terms (tmpnn_sample_tied; the reference's ProteinMPNN.tied_sample,
protein_mpnn_utils.py:1385-1494) on the oracle's primitives: a step loop per chain with an explicit h_V stack and h_S.

A chain's schedule is order [L] (a permutation) and close [L] (1 = the step is the last member of its group). Members of a group
are walked in step order; the first member with mask == 0 kills the group (the members before it stay decoded, the ones after it
never are, the group takes S_fixed there and its probs rows stay 0). A live member t is decoded through the three decoder layers
with the neighbours of lower step visible: their h_V stack rows, and h_S — which is still ZERO for the earlier members of the same
group, and the group's letter for earlier groups. acc += weight[t] * logits_t. At the closing member t1 of a live group

    probs = softmax(acc / temperature + bias[t1]);  mix: probs = (1 - mix[t1]) probs + mix[t1] pssm_bias[t1];
    keep: pm = probs keep[t1] + 0.001 probs, probs = pm / sum(pm);  allowed: pm = probs allowed[t1], probs = pm / sum(pm);
    the draw rule of sample_restatement.draw on u[n, t1];  letter = the pick where free[n, t1] * mask[t1] == 1, else S_fixed[n, t1];

and every member gets the letter, the probs row and h_S = W_s[letter]. ``margin``: a draw closer than that to a cumulative boundary
has its uniform redrawn from ``rng`` — u is returned as used, with the smallest margin and the smallest renormalising denominator met."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import thermompnn_oracle as orc
from sample_restatement import draw


def encode(W, g, E_idx):
    """The encoder, once -> (mp, mask [1,L], E_idx [1,L,K], h_E, h_V_enc, h_EXV_encoder)."""
    t = torch.from_numpy
    mp, _ = ({k: v.float() for k, v in part.items()} for part in orc.split_weights(W))
    X, mask = t(np.ascontiguousarray(g["X"])).float()[None], t(np.ascontiguousarray(g["mask"])).float()[None]
    ridx, cenc = t(g["residue_idx"].astype(np.int64))[None], t(g["chain_enc"].astype(np.int64))[None]
    ei = t(np.ascontiguousarray(E_idx).astype(np.int64))[None]
    with torch.no_grad():
        E, E_idx_t, _ = orc.protein_features(mp, X, mask, ridx, cenc, 48, ei)
        h_V = torch.zeros(E.shape[0], E.shape[1], E.shape[-1])
        h_E = orc.linear(E, mp, "W_e")
        mask_attend = mask.unsqueeze(-1) * orc.gather_nodes(mask.unsqueeze(-1), E_idx_t).squeeze(-1)
        for i in range(3):
            h_V, h_E = orc.enc_layer(mp, f"encoder_layers.{i}", h_V, h_E, E_idx_t, mask, mask_attend)
        h_EXV = orc.cat_neighbors_nodes(h_V, orc.cat_neighbors_nodes(torch.zeros_like(h_V), h_E, E_idx_t), E_idx_t)
    return mp, mask, E_idx_t, h_E, h_V, h_EXV


def sample_tied_chains(W, g, order, close, S_fixed, free, u, temperature=1.0, weight=None, bias=None, allowed=None, pssm_mix=None,
                       pssm_bias=None, pssm_keep=None, E_idx=None, margin=None, rng=None):
    """-> dict(S [N,L] int64, probs [N,L,21] fp32, u [N,L] as used, min_margin, min_den). weight [N,L] by residue or None;
    bias / allowed / pssm_bias / pssm_keep [L,21], pssm_mix [L], or None."""
    order, close, S_fixed = (np.asarray(a).astype(np.int64) for a in (order, close, S_fixed))
    free, u = np.asarray(free, dtype=np.float32), np.array(u, dtype=np.float32)
    N, L = order.shape
    assert (close[:, -1] == 1).all()
    f32 = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float32))
    bias, allowed, pssm_mix, pssm_bias, pssm_keep, weight = (f32(a) for a in (bias, allowed, pssm_mix, pssm_bias, pssm_keep, weight))
    mp, mask, ei, h_E, h_V_enc, h_EXV = encode(W, g, g["E_idx"] if E_idx is None else E_idx)
    mask_np = mask[0].numpy()
    S, probs = np.zeros((N, L), np.int64), np.zeros((N, L, 21), np.float32)
    min_margin, min_den = np.inf, 1.0
    with torch.no_grad():
        for n in range(N):
            rank = torch.empty(L, dtype=torch.int64)
            rank[torch.from_numpy(order[n])] = torch.arange(L)
            vis = (rank[ei[0]] < rank[:, None]).float()[None, :, :, None]                       # [1,L,K,1]
            mask_bw, mask_fw = mask.view(1, L, 1, 1) * vis, mask.view(1, L, 1, 1) * (1.0 - vis)
            h_S = torch.zeros_like(h_V_enc)
            stack = [h_V_enc] + [torch.zeros_like(h_V_enc) for _ in range(3)]
            members, dead, t_dead, acc = [], False, -1, torch.zeros(21)
            for s in range(L):
                t = int(order[n, s])
                members.append(t)
                if not dead and mask_np[t] == 0:
                    dead, t_dead = True, t
                if not dead:
                    sl = slice(t, t + 1)
                    h_ES_t = orc.cat_neighbors_nodes(h_S, h_E[:, sl], ei[:, sl])
                    enc_t = mask_fw[:, sl] * h_EXV[:, sl]
                    for l in range(3):
                        h_ESV = mask_bw[:, sl] * orc.cat_neighbors_nodes(stack[l], h_ES_t, ei[:, sl]) + enc_t
                        stack[l + 1][:, t] = orc.dec_layer(mp, f"decoder_layers.{l}", stack[l][:, sl], h_ESV, mask[:, sl])[:, 0]
                    logits = orc.linear(stack[3][0, t], mp, "W_out")
                    acc = acc + (1.0 if weight is None else weight[n, t]) * logits
                if not close[n, s]:
                    continue
                if dead:
                    letter = int(S_fixed[n, t_dead])
                else:
                    z = acc / float(temperature)
                    if bias is not None:
                        z = z + bias[t]
                    p = F.softmax(z, dim=-1)
                    if pssm_mix is not None:
                        p = (1 - pssm_mix[t]) * p + pssm_mix[t] * pssm_bias[t]
                    if pssm_keep is not None:
                        pm = p * pssm_keep[t] + p * 0.001
                        min_den = min(min_den, float(pm.sum()))
                        p = pm / pm.sum()
                    if allowed is not None:
                        pm = p * allowed[t]
                        min_den = min(min_den, float(pm.sum()))
                        p = pm / pm.sum()
                    p = p.numpy().astype(np.float32)
                    pick, mg = draw(p, u[n, t])
                    while margin is not None and mg < margin:
                        u[n, t] = np.float32(rng.random())
                        pick, mg = draw(p, u[n, t])
                    min_margin = min(min_margin, mg)
                    letter = pick if free[n, t] * mask_np[t] == 1 else int(S_fixed[n, t])
                    probs[n, members] = p
                S[n, members] = letter
                h_S[0, members] = mp["W_s.weight"][letter]
                members, dead, t_dead, acc = [], False, -1, torch.zeros(21)
    return {"S": S, "probs": probs, "u": u, "min_margin": min_margin, "min_den": min_den}
