"""Torch restatement of ProteinMPNN's order-masked decoder (the reference's protein_mpnn_utils.py:1247-1272 without the overwrite
of :1259, as conditional_probs / unconditional_probs :1496-1587 run it), built on the oracle's encoder and layer functions:

    vis(i, j)  = rank[j] < rank[i]                      (rank = inverse permutation of the reference's decoding_order)
    h_ESV_ij   = mask_i * (vis ? [h_E_ij, h_S_j, h_V_j of this layer] : [h_E_ij, 0, h_V_j of the encoder])

One encoder pass, then one full decode per (sequence, rank) pair. ``E_idx_override`` pins the neighbour graph slot by slot (the
device's graph, or a fixture's); ``f64`` evaluates everything in float64 (the truth of the hot draws)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import thermompnn_oracle as orc


def ordered_decode(W, g, S_var, ranks, E_idx, f64=False):
    """W: full synthetic state dict (prot_mpnn.* keys); g: a golden fixture (X, mask, residue_idx, chain_enc); S_var, ranks [V,L];
    E_idx [L,K], K <= 48 -> dict(hidden [V,3,L,128], log_probs [V,L,21], ddg [V,L,21]) as numpy arrays. ddg is the oracle's
    head_table on the restated decoder states as ssm_table calls it (reversed hidden list, the variant's own h_S and S)."""
    t = torch.from_numpy
    dt = torch.float64 if f64 else torch.float32
    orig_float, orig_default = torch.Tensor.float, torch.get_default_dtype()
    if f64:
        torch.Tensor.float = lambda self, *a, **k: self.double()      # the oracle's explicit .float() casts -> float64
        torch.set_default_dtype(torch.float64)
    try:
        mp, hd = ({k: v.to(dt) for k, v in part.items()} for part in orc.split_weights(W))
        X, mask = t(np.ascontiguousarray(g["X"])).to(dt)[None], t(np.ascontiguousarray(g["mask"])).to(dt)[None]
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
            hidden, log_probs, ddg = [], [], []
            for S, rank in zip(np.asarray(S_var), np.asarray(ranks)):
                r = t(rank.astype(np.int64))[None]
                vis = (torch.gather(r.unsqueeze(1).expand(-1, r.shape[1], -1), 2, E_idx_t) < r.unsqueeze(-1)).to(dt).unsqueeze(-1)
                mask_bw, mask_fw = mask_1D * vis, mask_1D * (1.0 - vis)
                h_S = F.embedding(t(S.astype(np.int64))[None], mp["W_s.weight"])
                h_ES = orc.cat_neighbors_nodes(h_S, h_E, E_idx_t)
                h_EXV_encoder_fw = mask_fw * h_EXV_encoder
                h_V, hs = h_V_enc, []
                for i in range(3):
                    h_ESV = mask_bw * orc.cat_neighbors_nodes(h_V, h_ES, E_idx_t) + h_EXV_encoder_fw
                    h_V = orc.dec_layer(mp, f"decoder_layers.{i}", h_V, h_ESV, mask)
                    hs.append(h_V)
                hidden.append(torch.cat(hs))
                ddg.append(orc.head_table(hd, hs[::-1], h_S, t(S.astype(np.int64))[None])[1][0])
                log_probs.append(F.log_softmax(orc.linear(h_V, mp, "W_out"), dim=-1)[0])
    finally:
        torch.Tensor.float = orig_float
        torch.set_default_dtype(orig_default)
    return {"hidden": torch.stack(hidden).numpy(), "log_probs": torch.stack(log_probs).numpy(), "ddg": torch.stack(ddg).numpy()}


def conditional_ranks(randn, idx, L, backbone_only=False):
    """The ranks conditional_probs decodes position idx under: the reference's expression (:1526-1534), inverted."""
    order_mask = torch.ones(L) if backbone_only else torch.zeros(L)
    order_mask[idx] = 0.0 if backbone_only else 1.0
    order = torch.argsort((order_mask[None,] + 0.0001) * (torch.abs(torch.as_tensor(randn).float().reshape(1, L))))[0]
    rank = torch.empty(L, dtype=torch.int64)
    rank[order] = torch.arange(L)
    return rank.numpy()
