"""The contract of tmpnn_select_hits (include/tmpnn.h) restated in numpy: the candidate rule, then np.lexsort((aa, pos, value + 0.0)).
Shared by tests/test_hits_host.py, tests/test_gpu_hits.py and tests/test_gpu_hits_network.py; every device comparison against it is
exact."""
import numpy as np

CYS = 1          # 'C' in ACDEFGHIKLMNPQRSTVWYX


def hits_reference(table, S, offsets, k, cutoff=None, include_cys=False, one_per_position=False):
    """table [T, >= 20] float32, S [T], offsets [P + 1] -> dict(hit_ddg [P, k] float32 padded with NaN (the table's own bits),
    hit_pos / hit_aa [P, k] int32 padded with -1, hit_count [P] int32)."""
    table = np.asarray(table, dtype=np.float32)
    S = np.asarray(S).astype(np.int64)
    offsets = np.asarray(offsets).astype(np.int64)
    P = len(offsets) - 1
    cut = np.float32(np.inf if cutoff is None else cutoff)
    out = dict(hit_ddg=np.full((P, k), np.nan, np.float32), hit_pos=np.full((P, k), -1, np.int32),
               hit_aa=np.full((P, k), -1, np.int32), hit_count=np.zeros(P, np.int32))
    for b in range(P):
        t0, t1 = int(offsets[b]), int(offsets[b + 1])
        v = table[t0:t1, :20]
        s = S[t0:t1]
        pos, aa = np.meshgrid(np.arange(t1 - t0), np.arange(20), indexing="ij")
        with np.errstate(invalid="ignore"):
            ok = ((s >= 0) & (s < 20))[:, None] & (aa != s[:, None]) & ~np.isnan(v) & (v <= cut)
        if not include_cys:
            ok &= aa != CYS
        if one_per_position:                         # the first minimum of each position, as idxmin (NaN never wins)
            with np.errstate(invalid="ignore"):      # (a signalling NaN in the table: the cast quiets it, `ok` keeps it out)
                w = np.where(ok, v.astype(np.float64), np.inf)
            first = ok & (w == w.min(axis=1, keepdims=True))      # the minimum's places among the candidates (+inf may be one)
            keep = np.zeros_like(ok)
            keep[np.arange(t1 - t0), np.argmax(first, axis=1)] = True
            ok = first & keep
        vals, pp, aas = v[ok], pos[ok], aa[ok]
        order = np.lexsort((aas, pp, vals + np.float32(0.0)))[:k]
        n = len(order)
        out["hit_ddg"][b, :n] = vals[order]
        out["hit_pos"][b, :n] = pp[order]
        out["hit_aa"][b, :n] = aas[order]
        out["hit_count"][b] = n
    return out


def assert_hits_equal(got, want):
    """Exact: the value BITS, positions, letters and counts."""
    g = {k_: np.asarray(v.cpu() if hasattr(v, "cpu") else v) for k_, v in got.items()}
    np.testing.assert_array_equal(g["hit_count"], want["hit_count"])
    np.testing.assert_array_equal(g["hit_pos"], want["hit_pos"])
    np.testing.assert_array_equal(g["hit_aa"], want["hit_aa"])
    np.testing.assert_array_equal(g["hit_ddg"].view(np.uint32), want["hit_ddg"].view(np.uint32))
