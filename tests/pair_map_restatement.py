"""The contract of tmpnn_pair_map (include/tmpnn.h) restated in numpy: every candidate of a call, the np.float32 sum and difference,
their integer order keys, minima per (row, position); the |e| sum as an explicit loop over b and then over v with np.float32 adds
(np.sum is pairwise, so it is not the contract). A state is the five arrays and takes part in the next call. Shared by
tests/test_pair_map_host.py and tests/test_gpu_pair_map.py; every device comparison against it is exact."""
import numpy as np

from pair_hits_restatement import CYS, NONE, ord32, unord32

MAX_LEN = 2048
STATE = (("best", np.uint64), ("eps_lo", np.uint64), ("eps_hi", np.uint64), ("eps_abs_sum", np.float32), ("count", np.int32))


def empty_state(R, L):
    return dict(best=np.full((R, L), NONE, np.uint64), eps_lo=np.full((R, L), NONE, np.uint64), eps_hi=np.full((R, L), NONE, np.uint64),
                eps_abs_sum=np.zeros((R, L), np.float32), count=np.zeros((R, L), np.int32))


def _key(o, letter, b):
    return (o.astype(np.uint64) << np.uint64(32)) | (letter.astype(np.uint64) << np.uint64(5)) | b.astype(np.uint64)


def pair_map_reference(ddg, S_var, base, row, letter, skip, wt, R, include_cys=False, upper=False, state=None):
    """One call. ``state``: None (a map starts: the whole state is empty first) or the dict an earlier call returned (not modified).
    -> dict(best, eps_lo, eps_hi uint64 [R, L], eps_abs_sum float32 [R, L], count int32 [R, L])."""
    ddg = np.asarray(ddg, dtype=np.float32)[:, :, :20]
    V, L = ddg.shape[:2]
    wt = np.asarray(wt, dtype=np.float32).reshape(L, -1)[:, :20]
    s = np.asarray(S_var).astype(np.int64).reshape(V, L)[:, :, None]
    base = np.asarray(base, dtype=np.float32).reshape(V)
    row, letter = np.asarray(row).astype(np.int64).reshape(V), np.asarray(letter).astype(np.int64).reshape(V)
    skip = np.full(V, -1, np.int64) if skip is None else np.asarray(skip).astype(np.int64).reshape(V)
    out = empty_state(R, L) if state is None else {k: np.array(np.asarray(state[k]).view(dt) if dt == np.uint64 else state[k], dtype=dt)
                                                   for k, dt in STATE}
    q = np.arange(L, dtype=np.int64)[None, :, None]
    b = np.arange(20, dtype=np.int64)[None, None, :]
    ok = ((letter >= 0) & (letter < 20))[:, None, None] & (s >= 0) & (s < 20) & (b != s)
    ok = ok & ((q > skip[:, None, None]) if upper else (q != skip[:, None, None]))
    if not include_cys:
        ok = ok & (b != CYS)
    with np.errstate(invalid="ignore", over="ignore"):                  # inf - inf: the NaN is the point
        val = base[:, None, None] + ddg                                 # np.float32 + np.float32: one IEEE add
        e = ddg - wt[None]                                              # one IEEE subtract
    assert val.dtype == np.float32 and e.dtype == np.float32
    let3, b3 = np.broadcast_to(letter[:, None, None] & 31, val.shape), np.broadcast_to(b, val.shape)
    o_val, o_e = ord32(val.view(np.uint32)), ord32(e.view(np.uint32))
    k_best = np.where(ok & ~np.isnan(val), _key(o_val, let3, b3), NONE).min(axis=2) if L else np.zeros((V, 0), np.uint64)
    e_ok = ok & ~np.isnan(e)
    k_lo = np.where(e_ok, _key(o_e, let3, b3), NONE).min(axis=2) if L else np.zeros((V, 0), np.uint64)
    k_hi = np.where(e_ok, _key(~o_e, let3, b3), NONE).min(axis=2) if L else np.zeros((V, 0), np.uint64)
    inner, cnt = np.zeros((V, L), np.float32), np.zeros((V, L), np.int32)
    mag = np.abs(e)
    with np.errstate(invalid="ignore", over="ignore"):
        for bb in range(20):                                            # ascending b, one np.float32 add per candidate
            inner = np.where(e_ok[:, :, bb], inner + mag[:, :, bb], inner)
            cnt = cnt + e_ok[:, :, bb]
        assert inner.dtype == np.float32
        for v in range(V):                                              # ascending v, one np.float32 add per variant
            r = row[v]
            if not 0 <= r < R:
                continue
            out["best"][r] = np.minimum(out["best"][r], k_best[v])
            out["eps_lo"][r] = np.minimum(out["eps_lo"][r], k_lo[v])
            out["eps_hi"][r] = np.minimum(out["eps_hi"][r], k_hi[v])
            out["eps_abs_sum"][r] = out["eps_abs_sum"][r] + inner[v]
            out["count"][r] = out["count"][r] + cnt[v]
    return out


def decode_reference(state):
    """What decode_pair_map returns, from the key layout of include/tmpnn.h, entry by entry."""
    out = {}
    for name, key, inverted in (("best", "best", False), ("eps_min", "eps_lo", False), ("eps_max", "eps_hi", True)):
        k = np.asarray(state[key]).view(np.uint64)
        none = k == NONE
        o = (k >> np.uint64(32)).astype(np.uint32)
        val = unord32(~o if inverted else o).view(np.float32).copy()
        val[none] = np.nan
        out["best_ddG" if name == "best" else name] = val
        out[name + "_a"] = np.where(none, -1, (k >> np.uint64(5)) & np.uint64(31)).astype(np.int32)
        out[name + "_b"] = np.where(none, -1, k & np.uint64(31)).astype(np.int32)
    count = np.asarray(state["count"])
    with np.errstate(invalid="ignore", divide="ignore"):
        out["eps_abs_mean"] = np.where(count == 0, np.float32(np.nan),
                                       np.asarray(state["eps_abs_sum"], np.float32) / np.maximum(count, 1).astype(np.float32)).astype(np.float32)
    out["count"] = count
    return out


def _np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def assert_pair_map_equal(got, want):
    """Exact: the three key arrays, the counts, and the BITS of the |e| sums."""
    for name, dt in STATE:
        g, w = _np(got[name]), _np(want[name])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if dt == np.uint64:
            np.testing.assert_array_equal(g.view(np.uint64), w.view(np.uint64), err_msg=name)
        elif dt == np.float32:
            assert g.dtype == np.float32
            np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=name)
        else:
            np.testing.assert_array_equal(g, w, err_msg=name)
