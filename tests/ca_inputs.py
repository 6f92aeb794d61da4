"""Crafted C-alpha inputs that the host and the GPU tests of the CA featurizer share (test helper, imported like masked_backbones.py;
never imported by the product), with the conditions they have to meet and the float64 truth they are judged against.

A member is a dict(Ca [n,3] float32, S [n] int64, mask [n] float32, ridx [n] int64, cenc [n] int64); a missing C-alpha has
coordinates 0 and mask 0. A pack is a list of members, laid along the packed residue axis one segment each.
  * long_pack(n): tiny_backbones.many_short(n) as CA input — more rows than three (n = 70) or eight (n = 260) times the compute units
    of an MI355X, lengths 8 .. 16 (Keff = L), every third member with a missing middle C-alpha;
  * short_pack(): a 12-row member, segments of 1, 2, 3, 4, 5 and 7 rows, a 16-row member with a missing C-alpha;
  * window_pack(): segments of 7 rows whose float32 steps ARE, bit for bit, the lengths on and next to the 3.6 / 4.0 window.

Conditioning. ca_restatement.well_conditioned looks at the quaternion's radicands and sign differences. One more source of
ill-conditioning sits in the frame itself: where a framed row's two steps are parallel or antiparallel, normalize(U[i-1] x U[i])
normalizes rounding noise (tiny_member(5, 55, masked=2): the missing C-alpha at (0,0,0) coincides with row 0 of a walk that starts
at the origin, row 1's two steps are 3.8 A and antiparallel, and the float32 and float64 restatements differ by 1.17 on edges
well_conditioned accepts). ``frame_conditioned`` is that rule: a framed row passes when |U[i-1] - U[i]| and |U[i-1] x U[i]| are each
exactly 0 or at least 1e-3. An edge of the inputs here is well-conditioned when well_conditioned holds and both of its rows pass."""
import numpy as np
import torch

import ca_restatement as car
from tiny_backbones import many_short, tiny_member

ILL_CAP = 0.10
WINDOW_MARGIN = 1e-3


def member(X, S, mask, ridx, cenc, shift=None):
    """A tiny_member / layout_arrays tuple as a CA member: slot 1, optionally translated, the C-alpha of a mask-0 residue zeroed."""
    Ca = X[:, 1].astype(np.float32)
    if shift is not None:
        Ca = (Ca + np.asarray(shift, np.float32)).astype(np.float32)
    Ca[mask == 0] = 0.0
    return dict(Ca=Ca, S=S.astype(np.int64), mask=mask.astype(np.float32), ridx=ridx.astype(np.int64), cenc=cenc.astype(np.int64))


def long_pack(n):
    return [member(*m) for m in many_short(n)]


def short_pack():
    """The ragged pack of short segments. The 16-row member is translated away from the origin before its C-alpha 9 is zeroed: the
    two steps that touch the missing atom are then ~28 A long and dropped by the window, instead of landing on row 0."""
    out = [member(*tiny_member(12, 301))]
    out += [member(*tiny_member(n, 310 + n)) for n in (1, 2, 3, 4, 5, 7)]
    out.append(member(*tiny_member(16, 302, masked=9), shift=(20.0, 12.0, -15.0)))
    return out


def offsets_of(pack):
    return np.concatenate([[0], np.cumsum([len(m["S"]) for m in pack])]).astype(np.int64)


# ---- the window's edges --------------------------------------------------------------------------------------------------------
def window_lengths():
    """name -> float32 step length: 3.6f, 4.0f, their float32 neighbours on both sides, and 3.8f. Every one is a multiple of 2^-22."""
    f, inf = np.float32, np.float32(np.inf)
    return {"below_3.6": np.nextafter(f(3.6), -inf), "3.6": f(3.6), "above_3.6": np.nextafter(f(3.6), inf), "3.8": f(3.8),
            "below_4.0": np.nextafter(f(4.0), -inf), "4.0": f(4.0), "above_4.0": np.nextafter(f(4.0), inf)}


# the six steps of each 7-row segment, along x, y, z, x, y, z. The lengths under test stand at steps 1 and 3 (each is U[i] of one
# framed row and U[i-1] of the next, beside a 3.8 step that is always kept), the last segment puts two of them side by side
WINDOW_SEGMENTS = (("3.8", "below_3.6", "3.8", "3.6", "3.8", "3.8"),
                   ("3.8", "above_3.6", "3.8", "below_4.0", "3.8", "3.8"),
                   ("3.8", "4.0", "3.8", "above_4.0", "3.8", "3.8"),
                   ("3.8", "3.8", "3.6", "4.0", "above_3.6", "3.8"),
                   ("below_4.0", "above_4.0", "below_3.6", "3.8", "3.8", "3.8"))
WINDOW_KEPT = ("above_3.6", "3.8", "below_4.0")


def window_pack():
    """-> (pack, steps [n_seg,6,3] float32: the step vectors the segments are built from). Every segment starts at the origin;
    an axis coordinate goes 0 -> +s -> s - s' (its two steps of the segment), so every coordinate is a multiple of 2^-22 below 4 + 2^-21
    in magnitude: representable, and every difference of consecutive rows is the step itself."""
    lengths = window_lengths()
    pack, steps = [], []
    for names in WINDOW_SEGMENTS:
        p = np.zeros(3, np.float64)
        rows, seg = [p.copy()], []
        for m, name in enumerate(names):
            v = np.zeros(3, np.float64)
            v[m % 3] = float(lengths[name]) * (1.0 if m < 3 else -1.0)
            p = p + v                                        # float64: exact for multiples of 2^-22 of this size
            rows.append(p.copy())
            seg.append(v)
        Ca64 = np.stack(rows)
        Ca = Ca64.astype(np.float32)
        assert np.array_equal(Ca.astype(np.float64), Ca64), "a coordinate is not representable in float32"
        n = len(rows)
        pack.append(dict(Ca=Ca, S=np.arange(n, dtype=np.int64) % 20, mask=np.ones(n, np.float32), ridx=np.arange(n, dtype=np.int64),
                         cenc=np.ones(n, np.int64)))
        steps.append(np.stack(seg).astype(np.float32))
    return pack, np.stack(steps)


def kept_steps(Ca):
    """[n-1] bool: the steps the window keeps, in Ca's dtype, by the expression of ca_restatement.frames."""
    dX = Ca[1:] - Ca[:-1]
    norm = torch.sqrt((dX * dX).sum(-1))
    return (3.6 < norm) & (norm < 4.0)


# ---- conditions ------------------------------------------------------------------------------------------------------------------
def window_margin(Ca):
    """smallest distance of a step length of one segment (float64, missing atoms at 0 as the kernels see them) from 3.6 and 4.0"""
    if len(Ca) < 2:
        return np.inf
    n = np.linalg.norm(np.diff(np.asarray(Ca, np.float64), axis=0), axis=-1)
    return float(np.abs(n[:, None] - np.array([3.6, 4.0])).min())


def frame_conditioned(Ca64, line=1e-3):
    """[n] bool for one segment Ca64 [n,3] float64: a framed row (1 .. n-3) passes when |U[i-1] - U[i]| and |U[i-1] x U[i]| are each
    exactly 0 or at least ``line``; the rows without a frame pass."""
    n = Ca64.shape[0]
    ok = torch.ones(n, dtype=torch.bool)
    if n < 4:
        return ok
    dX = Ca64[1:] - Ca64[:-1]
    U = car.normalize(dX * kept_steps(Ca64).to(Ca64.dtype)[:, None])
    u0, u1 = U[: n - 3], U[1: n - 2]
    a = torch.sqrt(((u0 - u1) ** 2).sum(-1))
    c = torch.sqrt((torch.cross(u0, u1, dim=-1) ** 2).sum(-1))
    ok[1: n - 2] = ((a == 0) | (a >= line)) & ((c == 0) | (c >= line))
    return ok


def host_graph(m, K=48):
    """The stable top-k of the masked distance in float32 (lowest index first among equals, the engine's rule) -> [n, min(K, n)] int64."""
    Ca, mask = torch.from_numpy(m["Ca"]), torch.from_numpy(m["mask"])
    m2 = mask[:, None] * mask[None, :]
    d = Ca[:, None] - Ca[None, :]
    D = m2 * torch.sqrt((d * d).sum(-1) + 1e-6)
    D_adj = D + (1 - m2) * D.max(-1, keepdim=True)[0]
    return torch.sort(D_adj, dim=-1, stable=True)[1][:, : min(K, len(mask))].contiguous()


def member_truth(W, m, ei):
    """One member on its local graph ``ei`` [n,Keff] int64 -> dict(E64 [n,Keff,128] float64 numpy, d32 [n,Keff]: the float32
    restatement's distance from the float64 one per edge, well [n,Keff] bool)."""
    t = torch.from_numpy
    Ca, mask, ridx, cenc = t(m["Ca"]), t(m["mask"]), t(m["ridx"]), t(m["cenc"])
    E64 = car.edge_features(W, Ca.double(), mask.double(), ridx, cenc, ei)
    E32 = car.edge_features(W, Ca, mask, ridx, cenc, ei)
    fc = frame_conditioned(Ca.double())
    well = car.well_conditioned(car.frames(Ca.double()), ei) & fc[:, None] & fc[ei]
    return dict(E64=E64.numpy(), d32=(E32.double() - E64).abs().amax(-1).numpy(), well=well.numpy())


def pack_truth(W, pack, graphs):
    """member_truth over a pack (``graphs``: one local E_idx per member) -> dict(members: the list, ill_share over the pack's valid
    edges, ref_well / ref_ill: the float32 restatement's largest distance from float64 on the well- / ill-conditioned edges)."""
    members = [member_truth(W, m, ei) for m, ei in zip(pack, graphs)]
    well = np.concatenate([x["well"].ravel() for x in members])
    d = np.concatenate([x["d32"].ravel() for x in members])
    return dict(members=members, ill_share=float((~well).mean()), ref_well=float(d[well].max()),
                ref_ill=float(d[~well].max()) if (~well).any() else 0.0, edges=int(well.size))
