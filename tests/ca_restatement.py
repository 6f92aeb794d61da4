"""Torch restatement of the C-alpha-only edge featurizer (test helper, never imported by the product), written from its specification:

  per edge (i, j = E_idx[i,k]) of a SEGMENT of n rows: [posenc 16 | 9 x 16 RBF | dU 3 | Q 4] -> edge_embedding (no bias) -> norm_edges
  * Ca_0[t] = Ca[t-1], Ca_1 = Ca, Ca_2[t] = Ca[t+1], with (0,0,0) in front of row 0 and behind row n-1;
  * RBF blocks (a,b) of sqrt(|Ca_a[i] - Ca_b[j]|^2 + 1e-6) in the order (1,1) = the k-NN's masked distance, (0,0), (2,2), (0,1), (0,2),
    (1,0), (1,2), (2,0), (2,1); centres linspace(2,22,16), sigma 1.25;
  * dX[m] = Ca[m+1] - Ca[m], zeroed unless 3.6 < |dX| < 4.0; U = normalize(dX); for 1 <= i <= n-3: o = normalize(U[i-1] - U[i]),
    nrm = normalize(U[i-1] x U[i]), O_i = rows (o, nrm, o x nrm); O = 0 on rows 0, n-2, n-1 (and everywhere for n < 3);
  * dU = normalize(O_i (Ca_j - Ca_i)); R = O_i^T O_j; Q = normalize(sign(R21-R12, R02-R20, R10-R01) * 0.5 sqrt|1 + (Rxx-Ryy-Rzz,
    -Rxx+Ryy-Rzz, -Rxx-Ryy+Rzz)|, 0.5 sqrt(relu(1 + tr R))); normalize(x) = x / max(|x|, 1e-12);
  * positional index: clip(residue_idx_i - residue_idx_j + 32, 0, 64) inside a chain, 65 across chains.

Runs in the dtype of ``Ca`` (float32 or float64) on a given E_idx. ``edge_terms`` gives the quantities whose sign / square root makes an
edge ill-conditioned in fp32, and ``well_conditioned`` the rule the GPU tests use."""
import torch


def normalize(x):
    return x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12)


def frames(Ca):
    """One segment: Ca [n,3] -> O [n,9]."""
    n = Ca.shape[0]
    O = torch.zeros((n, 9), dtype=Ca.dtype)
    if n < 3:
        return O
    dX = Ca[1:] - Ca[:-1]
    norm = torch.sqrt((dX * dX).sum(-1))
    dX = dX * ((3.6 < norm) & (norm < 4.0)).to(Ca.dtype)[:, None]
    U = normalize(dX)
    u0, u1 = U[: n - 3], U[1: n - 2]                   # rows i = 1 .. n-3: U[i-1], U[i]
    o = normalize(u0 - u1)
    nrm = normalize(torch.cross(u0, u1, dim=-1))
    O[1: n - 2] = torch.cat([o, nrm, torch.cross(o, nrm, dim=-1)], -1)
    return O


def frames_packed(Ca, offsets):
    """Packed residue axis: Ca [T,3], offsets [N+1] -> O [T,9], one segment per protein."""
    return torch.cat([frames(Ca[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])]) if len(offsets) > 1 else Ca.new_zeros((0, 9))


def rotations(O, E_idx):
    """R = O_i^T O_j [n,K,3,3]."""
    Oi = O.view(-1, 3, 3)
    return torch.einsum("ima,ikmb->ikab", Oi, Oi[E_idx])


def edge_terms(O, E_idx):
    """-> dict(rad [n,K,3], diff [n,K,3], tr1 [n,K]): the radicands 1 + (...), the sign differences and 1 + tr R."""
    R = rotations(O, E_idx)
    xx, yy, zz = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    rad = 1 + torch.stack([xx - yy - zz, -xx + yy - zz, -xx - yy + zz], -1)
    diff = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return dict(rad=rad, diff=diff, tr1=1 + xx + yy + zz)


def well_conditioned(O64, E_idx, line=1e-3):
    """[n,K] bool: in float64, each of the three radicands, the three sign differences and 1 + tr R is exactly 0 or at least ``line``
    in magnitude."""
    t = edge_terms(O64, E_idx)
    v = torch.cat([t["rad"], t["diff"], t["tr1"][..., None]], -1).abs()
    return ((v == 0) | (v >= line)).all(-1)


def masked_neighbor_distance(Ca, mask, E_idx):
    """The k-NN's adjusted distance of the listed neighbours: D = m_i m_j sqrt(|Ca_i - Ca_j|^2 + 1e-6), D + (1 - m_i m_j) max_j D."""
    m2 = mask[:, None] * mask[None, :]
    d = Ca[:, None] - Ca[None, :]
    D = m2 * torch.sqrt((d * d).sum(-1) + 1e-6)
    D_adj = D + (1 - m2) * D.max(-1, keepdim=True)[0]
    return torch.gather(D_adj, 1, E_idx)


def edge_inputs(Ca, mask, residue_idx, chain_enc, E_idx, pos_w, pos_b):
    """One segment -> the 167 inputs [n,K,167]."""
    n = Ca.shape[0]
    z = Ca.new_zeros((1, 3))
    shifted = [torch.cat([z, Ca[:-1]]), Ca, torch.cat([Ca[1:], z])]
    mu = torch.linspace(2.0, 22.0, 16, dtype=Ca.dtype)
    rbf = lambda D: torch.exp(-(((D[..., None] - mu) / 1.25) ** 2))
    blocks = [rbf(masked_neighbor_distance(Ca, mask, E_idx))]
    for a, b in ((0, 0), (2, 2), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)):
        d = shifted[a][:, None] - shifted[b][E_idx]
        blocks.append(rbf(torch.sqrt((d * d).sum(-1) + 1e-6)))
    O = frames(Ca)
    Oi = O.view(n, 3, 3)
    dU = normalize(torch.einsum("irc,ikc->ikr", Oi, Ca[E_idx] - Ca[:, None]))
    t = edge_terms(O, E_idx)
    xyz = torch.sign(t["diff"]) * 0.5 * torch.sqrt(t["rad"].abs())
    w = 0.5 * torch.sqrt(torch.relu(t["tr1"]))[..., None]
    Q = normalize(torch.cat([xyz, w], -1))
    off = residue_idx[:, None] - residue_idx[E_idx]
    same = chain_enc[:, None] == chain_enc[E_idx]
    d = torch.where(same, (off + 32).clamp(0, 64), torch.full_like(off, 65))
    pos = torch.nn.functional.one_hot(d, 66).to(Ca.dtype) @ pos_w.T + pos_b
    return torch.cat([pos] + blocks + [dU, Q], -1)


def edge_features(W, Ca, mask, residue_idx, chain_enc, E_idx):
    """One segment: Ca [n,3], mask [n], residue_idx / chain_enc [n] int64, E_idx [n,K] int64 (local rows) -> E [n,K,128] in Ca's
    dtype with the weights ``W`` (a ca_only state dict)."""
    dt = Ca.dtype
    g = lambda k: W[k].to(dt)
    x = edge_inputs(Ca, mask.to(dt), residue_idx, chain_enc, E_idx, g("features.embeddings.linear.weight"), g("features.embeddings.linear.bias"))
    y = x @ g("features.edge_embedding.weight").T
    return torch.nn.functional.layer_norm(y, (128,), g("features.norm_edges.weight"), g("features.norm_edges.bias"), 1e-5)
