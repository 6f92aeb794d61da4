"""Torch restatement of autoregressive sampling (the reference's ProteinMPNN.sample, protein_mpnn_utils.py:1279-1383) on top of the
order-masked decoder's restatement (ordered_restatement.py): one teacher-forced decode of the partly filled sequences per step,

    t = order[n, s];  probs = softmax(log_probs[n, t] / temperature + bias[t])   (log_softmax differs from the logits by a per-row
    constant, which the softmax drops);  with allowed: probs = probs * allowed[t] / sum(probs * allowed[t]);
    c_a = fp32 running sum of probs in index order; the pick is the smallest a with c_a > u[n, t] * c_20, or the largest a with
    probs_a > 0 when rounding leaves none;
    S[n, t] = the pick where free[n, t] * mask[t] == 1, S_fixed[n, t] elsewhere; the probs row is probs there and 0 elsewhere.

The residues a chain has not decoded yet are invisible to the decoder, so whatever S holds there does not matter. O(L) decodes: for
tests at small L (the encoder runs once). ``margin``: every draw whose u * c_20 lies closer than that to a cumulative boundary (0
and every c_a) has its uniform redrawn from ``rng`` — u is returned as used, with the smallest margin met."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import thermompnn_oracle as orc


def cumulative(p):
    """fp32 running sum in index order."""
    c, run = np.zeros(len(p), np.float32), np.float32(0.0)
    for a in range(len(p)):
        run = np.float32(run + np.float32(p[a]))
        c[a] = run
    return c


def draw(p, u):
    """-> (pick, margin) of the draw rule for probabilities p [21] (fp32) and one uniform."""
    c = cumulative(p)
    thr = np.float32(np.float32(u) * c[-1])
    above = np.nonzero(c > thr)[0]
    pick = int(above[0]) if len(above) else int(np.nonzero(np.asarray(p) > 0)[0][-1])
    margin = float(np.abs(np.concatenate([[0.0], c.astype(np.float64)]) - float(thr)).min())
    return pick, margin


def inverse_orders(order):
    """order [N,L] (order[n,s] = residue decoded at step s) -> ranks [N,L] (rank[n,t] = step of residue t)."""
    order = np.asarray(order).astype(np.int64)
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(order.shape[1]), order.shape), axis=1)
    return ranks


def make_decoder(W, g, E_idx):
    """The order-masked decoder of ordered_restatement.ordered_decode with the encoder hoisted: -> decode(S [V,L], ranks [V,L]) ->
    log_probs [V,L,21] (numpy fp32)."""
    t = torch.from_numpy
    mp, _ = ({k: v.float() for k, v in part.items()} for part in orc.split_weights(W))
    X, mask = t(np.ascontiguousarray(g["X"])).float()[None], t(np.ascontiguousarray(g["mask"])).float()[None]
    ridx, cenc = t(g["residue_idx"].astype(np.int64))[None], t(g["chain_enc"].astype(np.int64))[None]
    ei = t(np.ascontiguousarray(E_idx).astype(np.int64))[None]
    with torch.no_grad():
        E, E_idx_t, _ = orc.protein_features(mp, X, mask, ridx, cenc, 48, ei)
        h_V_enc = torch.zeros(E.shape[0], E.shape[1], E.shape[-1])
        h_E = orc.linear(E, mp, "W_e")
        mask_attend = mask.unsqueeze(-1) * orc.gather_nodes(mask.unsqueeze(-1), E_idx_t).squeeze(-1)
        for i in range(3):
            h_V_enc, h_E = orc.enc_layer(mp, f"encoder_layers.{i}", h_V_enc, h_E, E_idx_t, mask, mask_attend)
        h_EXV_encoder = orc.cat_neighbors_nodes(h_V_enc, orc.cat_neighbors_nodes(torch.zeros_like(h_V_enc), h_E, E_idx_t), E_idx_t)
    mask_1D = mask.view(1, -1, 1, 1)

    def decode(S_var, ranks):
        out = []
        with torch.no_grad():
            for S, rank in zip(np.asarray(S_var), np.asarray(ranks)):
                r = t(rank.astype(np.int64))[None]
                vis = (torch.gather(r.unsqueeze(1).expand(-1, r.shape[1], -1), 2, E_idx_t) < r.unsqueeze(-1)).float().unsqueeze(-1)
                mask_bw, mask_fw = mask_1D * vis, mask_1D * (1.0 - vis)
                h_S = F.embedding(t(S.astype(np.int64))[None], mp["W_s.weight"])
                h_ES = orc.cat_neighbors_nodes(h_S, h_E, E_idx_t)
                h_EXV_encoder_fw = mask_fw * h_EXV_encoder
                h_V = h_V_enc
                for i in range(3):
                    h_ESV = mask_bw * orc.cat_neighbors_nodes(h_V, h_ES, E_idx_t) + h_EXV_encoder_fw
                    h_V = orc.dec_layer(mp, f"decoder_layers.{i}", h_V, h_ESV, mask)
                out.append(F.log_softmax(orc.linear(h_V, mp, "W_out"), dim=-1)[0])
        return torch.stack(out).numpy()
    return decode


def probs_of(log_probs_row, temperature, bias_row=None, allowed_row=None):
    """The sampler's distribution from one row of log-probabilities (fp32 torch arithmetic, the reference's expressions)."""
    z = torch.as_tensor(np.asarray(log_probs_row, dtype=np.float32)) / float(temperature)
    if bias_row is not None:
        z = z + torch.as_tensor(np.asarray(bias_row, dtype=np.float32))
    p = F.softmax(z, dim=-1)
    if allowed_row is not None:
        pm = p * torch.as_tensor(np.asarray(allowed_row, dtype=np.float32))
        p = pm / torch.sum(pm, dim=-1, keepdim=True)
    return p.numpy()


def sample_chains(W, g, order, S_fixed, free, u, temperature=1.0, bias=None, allowed=None, E_idx=None, margin=None, rng=None):
    """-> dict(S [N,L] int64, probs [N,L,21] fp32, u [N,L] as used, min_margin). bias / allowed: [L,21] or None."""
    order, S_fixed = np.asarray(order).astype(np.int64), np.asarray(S_fixed).astype(np.int64)
    free, u = np.asarray(free, dtype=np.float32), np.array(u, dtype=np.float32)
    N, L = order.shape
    mask = np.asarray(g["mask"], dtype=np.float32)
    decode = make_decoder(W, g, g["E_idx"] if E_idx is None else E_idx)
    ranks = inverse_orders(order)
    S, probs, min_margin = S_fixed.copy(), np.zeros((N, L, 21), np.float32), np.inf
    for s in range(L):
        ts = order[:, s]
        if (mask[ts] == 0).all():
            continue
        lp = decode(S, ranks)
        for n in range(N):
            t = int(ts[n])
            p = probs_of(lp[n, t], temperature, None if bias is None else bias[t], None if allowed is None else allowed[t])
            pick, mg = draw(p, u[n, t])
            while margin is not None and mg < margin:
                u[n, t] = np.float32(rng.random())
                pick, mg = draw(p, u[n, t])
            min_margin = min(min_margin, mg)
            if free[n, t] * mask[t] == 1:
                S[n, t], probs[n, t] = pick, p
    return {"S": S, "probs": probs, "u": u, "min_margin": min_margin}
