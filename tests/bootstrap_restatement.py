"""tmpnn_bootstrap_metrics (include/tmpnn.h) restated in numpy, its fixtures and its tolerances; no GPU and no library needed.

``bootstrap_reference`` follows the contract to the letter: per resample one histogram over the tie groups, one prefix sum,
X = P[g - 1] + P[g] + 1, the three rank sums in exact int64, spearman from those integers, the value metrics in float64 centred on the
resample's own means, degeneracy decided on the integers. ``bootstrap_exact`` is independent of all of that: it sorts the gathered
values, averages the ranks of ties and evaluates every metric in rational arithmetic (``fractions``); only the final square roots
and the conversion to float round. ``bootstrap_brute`` is metrics.get_metrics on the gathered arrays."""
import math
from fractions import Fraction

import numpy as np

METRICS = ("r2", "mse", "rmse", "spearman", "pearson")
LDS_N, MAX_N, MAX_B, MAX_M = 16384, 1 << 20, 1 << 20, 8
HOST_SIZES = (1, 2, 3, 19, 257, 1000)
SPEARMAN_TOL = 1e-14            # three int -> double conversions, two roots, a multiply, a divide: <= 7 * 2^-53


def value_tol(N, want):
    """Float64 sums of N terms: a backward error of N 2^-53; 16 covers the centring and the few operations behind the sums."""
    return max(1e-13, 16.0 * N * 2.0 ** -53) * np.maximum(1.0, np.abs(want))


def dense_rank(values):
    """gid [C, N] int32 of values [C, N]: the 0-based rank among the column's distinct values, equality being IEEE =="""
    v = np.asarray(values, np.float32)
    return np.stack([np.unique(v[c], return_inverse=True)[1].reshape(-1) for c in range(v.shape[0])]).astype(np.int32)


def bootstrap_reference(values, gid, idx, out=None):
    """-> dict(metrics [B, M, 5] float64, ranks [B, M, 3] int64, status [B] int32). ``out``: the arrays a call finds in place
    (a resample whose status is not 0 leaves its rows of them alone)."""
    values, gid, idx = np.asarray(values, np.float32), np.asarray(gid, np.int32), np.asarray(idx, np.int32)
    C, N = values.shape
    B, M = idx.shape[0], C - 1
    assert gid.shape == (C, N) and idx.shape == (B, N) and 1 <= M <= MAX_M and N <= MAX_N and B <= MAX_B
    if out is None:
        out = dict(metrics=np.full((B, M, 5), np.nan), ranks=np.zeros((B, M, 3), np.int64), status=np.zeros(B, np.int32))
    metrics, ranks, status = out["metrics"], out["ranks"], out["status"]
    base = N * (N + 1) * (N + 1)
    for b in range(B):
        row = idx[b].astype(np.int64)
        if ((row < 0) | (row >= N)).any():
            status[b] = -1
            continue
        g = gid[:, row].astype(np.int64)                               # [C, N]: only the entries this resample meets
        if ((g < 0) | (g >= N)).any():
            status[b] = -2
            continue
        status[b] = 0
        X = np.empty((C, N), np.int64)
        for c in range(C):
            cnt = np.bincount(g[c], minlength=N).astype(np.int64)
            P = np.cumsum(cnt)
            X[c] = (2 * P - cnt + 1)[g[c]]                             # P[g - 1] + P[g] + 1 at every draw
        t = values[0, row].astype(np.float64)
        Syy = int((X[0] * X[0]).sum())
        tc = t - t.sum() / N
        stt = (tc * tc).sum()
        for m in range(M):
            p = values[m + 1, row].astype(np.float64)
            Sxy, Sxx = int((X[m + 1] * X[0]).sum()), int((X[m + 1] * X[m + 1]).sum())
            ranks[b, m] = (Sxy, Sxx, Syy)
            pc = p - p.sum() / N
            see = ((p - t) ** 2).sum()
            mse = see / N
            x_const, y_const = Sxx == base, Syy == base
            metrics[b, m, 0] = np.nan if y_const else 1.0 - see / stt
            metrics[b, m, 1] = mse
            metrics[b, m, 2] = np.sqrt(mse)
            if x_const or y_const:
                metrics[b, m, 3] = metrics[b, m, 4] = np.nan
            else:
                metrics[b, m, 3] = float(Sxy - base) / (math.sqrt(float(Sxx - base)) * math.sqrt(float(Syy - base)))
                metrics[b, m, 4] = (pc * tc).sum() / np.sqrt((pc * pc).sum() * stt)
    return out


def _rank_fractions(x, ordinal=False):
    """1-based ranks of a list of Fractions; ties share their average unless ``ordinal`` (then: the order of appearance)"""
    order = sorted(range(len(x)), key=lambda i: (x[i], i))
    r = [Fraction(0)] * len(x)
    i = 0
    while i < len(x):
        j = i
        while not ordinal and j + 1 < len(x) and x[order[j + 1]] == x[order[i]]:
            j += 1
        for k in range(i, j + 1):
            r[order[k]] = Fraction(i + j, 2) + 1
        i = j + 1
    return r


def _corr_exact(a, b):
    n = len(a)
    ma, mb = sum(a) / n, sum(b) / n
    saa, sbb = sum((x - ma) ** 2 for x in a), sum((y - mb) ** 2 for y in b)
    if saa == 0 or sbb == 0:
        return float("nan")
    sab = sum((x - ma) * (y - mb) for x, y in zip(a, b))
    return math.copysign(math.sqrt(float(sab * sab / (saa * sbb))), sab)


def bootstrap_exact(values, row, ordinal=False):
    """[M, 5] float64 of ONE resample from rational arithmetic on the gathered values (float32 values are rationals)."""
    values = np.asarray(values, np.float32)
    row = np.asarray(row, np.int64)
    n = len(row)
    t = [Fraction(float(v)) for v in values[0, row]]
    mt = sum(t) / n
    stt = sum((y - mt) ** 2 for y in t)
    rt = _rank_fractions(t, ordinal)
    out = np.empty((values.shape[0] - 1, 5))
    for m in range(values.shape[0] - 1):
        p = [Fraction(float(v)) for v in values[m + 1, row]]
        see = sum((x - y) ** 2 for x, y in zip(p, t))
        out[m, 0] = float(1 - see / stt) if stt != 0 else np.nan
        out[m, 1] = float(see / n)
        out[m, 2] = math.sqrt(float(see / n))
        out[m, 4] = _corr_exact(p, t)
        out[m, 3] = _corr_exact(_rank_fractions(p, ordinal), rt) if not math.isnan(out[m, 4]) else np.nan
    return out


def bootstrap_brute(values, row):
    """[M, 5] of ONE resample: metrics.get_metrics on the gathered arrays"""
    from thermompnn_amd.metrics import get_metrics
    values = np.asarray(values, np.float32)
    row = np.asarray(row, np.int64)
    out = np.empty((values.shape[0] - 1, 5))
    for m in range(values.shape[0] - 1):
        r = get_metrics(values[m + 1, row], values[0, row])
        out[m] = [r[k] for k in METRICS]
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def fixture_values(N, M=3, seed=0):
    """values [1 + M, N] float32, tie-heavy and well conditioned (|mean| <= 3 std, |r2| <= 3): the measured column ~ N(-0.7, 1.5)
    rounded to 0.5, predictions 0.6 truth + N(0, 1) rounded to 0.25. With M >= 3 the last three columns are special: the one
    before the last two holds +0.0 / -0.0 and floats one ulp apart, then a column of two values, then a column of one value."""
    rng = np.random.default_rng(1000 * seed + N)
    raw = rng.normal(-0.7, 1.5, N)
    cols = [np.round(raw * 2) / 2]
    for m in range(M):
        cols.append(np.round((0.6 * raw + rng.normal(0.0, 1.0, N)) * 4) / 4)
    v = np.stack(cols).astype(np.float32)
    if M >= 3:
        c = v[M - 2]
        zero, one = np.flatnonzero(c == 0), np.flatnonzero(np.abs(c - 1.0) <= 0.25)
        c[zero[::2]] = np.float32(-0.0)
        c[one] = np.float32(1.0)
        c[one[::2]] = np.nextafter(np.float32(1.0), np.float32(2.0))
        if N >= 2:                                                     # the special patterns are there at every size
            c[0], c[N - 1] = np.float32(-0.0), np.float32(0.0)
        if N >= 19:
            c[1], c[2] = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
        v[M - 1] = np.where(raw > -0.7, np.float32(0.25), np.float32(-1.5))
        v[M] = np.float32(-0.75)
    return v


def fixture_rows(N, n_random=4, seed=0):
    """idx [B, N] int32: random resamples, then the identity row, an all-one-index row and two rows of indices 0 and N - 1 only"""
    rng = np.random.default_rng(77 * seed + N)
    rows = [rng.integers(0, N, N) for _ in range(n_random)]
    rows.append(np.arange(N))
    rows.append(np.full(N, N // 2))
    ends = np.where(rng.integers(0, 2, N) == 1, N - 1, 0)
    rows.append(ends)
    rows.append(np.where(np.arange(N) % 3 == 0, 0, N - 1))
    return np.stack(rows).astype(np.int32)


def assert_bootstrap_close(got, want, N, exact_ranks=True):
    """``got`` against the restatement ``want`` (dicts): ranks and status equal, NaNs in the same places, metrics within the lines"""
    np.testing.assert_array_equal(got["status"], want["status"])
    if exact_ranks:
        np.testing.assert_array_equal(got["ranks"], want["ranks"])
    assert_metrics_close(got["metrics"], want["metrics"], N)


def assert_metrics_close(g, w, N):
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    assert g.shape == w.shape
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    live = ~np.isnan(w)
    err = np.where(live, np.abs(g - np.where(live, w, 0.0)), 0.0)
    line = np.where(np.arange(5) == 3, SPEARMAN_TOL, value_tol(N, np.where(live, w, 0.0)))
    worst = float((err / line).max()) if err.size else 0.0
    assert (err <= line).all(), f"N={N}: worst error / line = {worst:.3g}"
    return worst
