"""The contract of tmpnn_ensemble_stats (include/tmpnn.h) restated in numpy float32: per ensemble a loop over the members in ascending
m — that order IS the contract, np.sum is pairwise and is not — with one np.float32 add per participant for the sum, then one subtract,
one multiply and one add per participant for the squared deviations (every one an elementwise IEEE operation over the [L, 20] entries),
np.float32 divides and np.sqrt (both correctly rounded), every NaN written as 0x7fc00000; the extremes by hits_ord keys, first member
first. ``ensemble_brute`` says the same with Python scalars, entry by entry, and carries float64 figures beside it. Shared by
tests/test_ensemble_host.py and tests/test_gpu_ensemble.py; every device comparison against the restatement is exact."""
import math

import numpy as np

from pair_hits_restatement import ord32

MAX_LEN, MAX_E = 8192, 65535
CANON = np.uint32(0x7fc00000)
FLOATS = ("mean", "spread", "lo", "hi")
INTS = ("lo_member", "hi_member", "count", "below")
ARRAYS = FLOATS + INTS


def is_nan_bits(bits):
    return (np.asarray(bits, np.uint32) & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def canon(x):
    """float32 array -> the same with every NaN written as 0x7fc00000."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b[is_nan_bits(b)] = CANON
    return b.view(np.float32)


def filled(T_out, bits=0xdeadbeef):
    """Outputs prefilled with a sentinel bit pattern (a NaN as a float): what a call must leave where it writes nothing."""
    out = {name: np.full((T_out, 20), bits, np.uint32).view(np.float32) for name in FLOATS}
    out.update({name: np.full((T_out, 20), bits, np.uint32).view(np.int32) for name in INTS})
    return out


def desc_ok(row0, M, L, out0, T, T_out, max_len):
    return min(row0, M, L, out0) >= 0 and L <= max_len and row0 + M * L <= T and out0 + L <= T_out      # (Python ints: no overflow)


def ensemble_reference(ddg, S, desc, T_out, max_len, cutoff=None, out=None, fma=False, order=None):
    """One call. ddg [T, >= 20] float32, S [T], desc [E, 4] = (row0, M, L, out_row0). ``out``: prefilled outputs (not modified; rows
    of ensembles that fail the descriptor check keep them), default ``filled(T_out)``. -> dict of the eight arrays and status [E].
    ``fma``: t = fma(d, d, t) in place of multiply-then-add, ``order``: a permutation of the members to sum in — the two ways a
    kernel could break the contract, for the conditions of tests/test_ensemble_host.py only."""
    ddg = np.asarray(ddg, dtype=np.float32)
    T = ddg.shape[0]
    ddg = ddg[:, :20]
    S = np.asarray(S).astype(np.int64).reshape(T)
    desc = np.asarray(desc).astype(np.int64).reshape(-1, 4)
    cut = np.float32(np.inf if cutoff is None else cutoff)
    assert not np.isnan(cut)
    res = {k: np.array(v) for k, v in (filled(T_out) if out is None else out).items()}
    status = np.zeros(len(desc), np.int32)
    for e, (row0, M, L, out0) in enumerate(tuple(int(v) for v in d) for d in desc):
        if not desc_ok(row0, M, L, out0, T, T_out, max_len):
            status[e] = -1
            continue
        x = ddg[row0:row0 + M * L].reshape(M, L, 20)
        s_own = S[row0:row0 + M * L].reshape(M, L, 1)
        live = (s_own >= 0) & (s_own < 20) & ~is_nan_bits(x.view(np.uint32))
        o = ord32(x.view(np.uint32))
        members = range(M) if order is None else [int(m) for m in order]
        s = np.zeros((L, 20), np.float32)
        n, below = np.zeros((L, 20), np.int32), np.zeros((L, 20), np.int32)
        o_lo, o_hi = np.zeros((L, 20), np.uint32), np.zeros((L, 20), np.uint32)
        x_lo, x_hi = np.full((L, 20), CANON, np.uint32), np.full((L, 20), CANON, np.uint32)
        m_lo, m_hi = np.full((L, 20), -1, np.int32), np.full((L, 20), -1, np.int32)
        with np.errstate(all="ignore"):
            for m in members:                                           # ascending m: the order of the sum is the contract
                p = live[m]
                s = np.where(p, s + x[m], s)
                first = p & (n == 0)
                lower, higher = first | (p & (o[m] < o_lo)), first | (p & (o[m] > o_hi))
                o_lo, x_lo, m_lo = np.where(lower, o[m], o_lo), np.where(lower, x[m].view(np.uint32), x_lo), np.where(lower, m, m_lo)
                o_hi, x_hi, m_hi = np.where(higher, o[m], o_hi), np.where(higher, x[m].view(np.uint32), x_hi), np.where(higher, m, m_hi)
                n = n + p
                below = below + (p & (x[m] <= cut))
            assert s.dtype == np.float32
            fn = np.maximum(n, 1).astype(np.float32)
            mean = s / fn                                               # np.float32 / np.float32: one IEEE divide
            t = np.zeros((L, 20), np.float32)
            for m in members:
                d = x[m] - mean
                if fma:                                                 # d * d is exact in float64 (48 bits), so this is the fused form up
                    step = (d.astype(np.float64) * d.astype(np.float64) + t.astype(np.float64)).astype(np.float32)   # to a double rounding
                else:
                    dd = d * d
                    step = t + dd
                t = np.where(live[m], step, t)
            assert t.dtype == np.float32 and mean.dtype == np.float32
            spread = np.sqrt(t / fn)
        none = n == 0
        sl = slice(out0, out0 + L)
        res["mean"][sl] = canon(np.where(none, np.float32(np.nan), mean))
        res["spread"][sl] = canon(np.where(none, np.float32(np.nan), spread))
        res["lo"][sl], res["hi"][sl] = x_lo.view(np.float32), x_hi.view(np.float32)
        res["lo_member"][sl], res["hi_member"][sl], res["count"][sl], res["below"][sl] = m_lo, m_hi, n, below
    res["status"] = status
    return res


def ensemble_brute(ddg, S, row0, M, L, cutoff=None):
    """ONE good ensemble, the contract read aloud: Python loops over (q, b, m) with np.float32 scalars and (value, m) tuples.
    -> the eight [L, 20] arrays, and in float64: mean64, spread64 (population form, from the exact inputs), sum_abs."""
    ddg = np.asarray(ddg, dtype=np.float32)
    cut = np.float32(np.inf if cutoff is None else cutoff)
    out = {name: np.zeros((L, 20), np.float32) for name in FLOATS}
    out.update({name: np.zeros((L, 20), np.int32) for name in INTS})
    out.update({name: np.full((L, 20), np.nan) for name in ("mean64", "spread64", "sum_abs")})
    nan = np.uint32(CANON).view(np.float32)
    with np.errstate(all="ignore"):
        for q in range(L):
            for b in range(20):
                part = []
                for m in range(M):
                    row = row0 + m * L + q
                    x = ddg[row, b]
                    if 0 <= int(S[row]) < 20 and not math.isnan(float(x)):
                        part.append((m, x))
                n = len(part)
                out["count"][q, b] = n
                out["below"][q, b] = sum(1 for _, x in part if x <= cut)
                if n == 0:
                    for name in FLOATS:
                        out[name][q, b] = nan
                    out["lo_member"][q, b] = out["hi_member"][q, b] = -1
                    continue
                s = np.float32(0.0)
                for _, x in part:
                    s = np.float32(s + x)
                mean = np.float32(s / np.float32(n))
                t = np.float32(0.0)
                for _, x in part:
                    d = np.float32(x - mean)
                    t = np.float32(t + np.float32(d * d))
                spread = np.float32(np.sqrt(np.float32(t / np.float32(n))))
                out["mean"][q, b] = nan if math.isnan(float(mean)) else mean
                out["spread"][q, b] = nan if math.isnan(float(spread)) else spread
                m_lo, x_lo = min(part, key=lambda mx: (float(mx[1]) + 0.0, mx[0]))       # (-0.0 == +0.0 in the compare: ties to the first)
                m_hi, x_hi = min(part, key=lambda mx: (-(float(mx[1]) + 0.0), mx[0]))
                out["lo"][q, b], out["hi"][q, b], out["lo_member"][q, b], out["hi_member"][q, b] = x_lo, x_hi, m_lo, m_hi
                v = np.array([float(x) for _, x in part], np.float64)
                out["mean64"][q, b], out["spread64"][q, b], out["sum_abs"][q, b] = v.mean(), v.std(), np.abs(v).sum()
    return out


def _np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def assert_ensemble_equal(got, want, rows=None, want_rows=None):
    """Exact: the four float arrays as uint32 BITS, the four int arrays as they are (``rows`` / ``want_rows``: slices to compare)."""
    for name in ARRAYS:
        g, w = _np(got[name]), _np(want[name])
        g, w = (g if rows is None else g[rows]), (w if want_rows is None else w[want_rows])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if name in FLOATS:
            assert g.dtype == np.float32 and w.dtype == np.float32, name
            np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32), err_msg=name)
        else:
            assert g.dtype == np.int32, name
            np.testing.assert_array_equal(g, w, err_msg=name)
