"""The contracts of tmpnn_align_global and tmpnn_ensemble_stats_rows (include/tmpnn.h) restated in numpy; no GPU, no torch.

Alignment: ``datasets.global_alignment_map``'s rule on int32 letter codes. score[i][j] is the LCS length of a[i:], b[j:], filled by
anti-diagonals into a skewed array (sk[i + j, i] = score[i][j], so a diagonal is one contiguous slice), then the trace from (0, 0)
reads the scores as the function's own ``while`` does: diagonal when the codes match and score[i][j] == score[i+1][j+1] + 1, else
i += 1 when score[i][j] == score[i+1][j], else j += 1. Two codes match iff they are equal and 0 <= code < 20.
``rule="down_first"`` swaps the first two tests: an equally optimal alignment under another tie rule, for the condition of
tests/test_align_host.py that the fixtures can tell the rules apart.

Rows: the statistics of ``ensemble_restatement`` read through a row map, written out on its own (gather, then the same ascending
loop), so that tests/test_align_host.py can hold it against ``ensemble_reference`` on the gathered table.
Shared by tests/test_align_host.py, tests/test_gpu_align.py and tests/test_gpu_ensemble_rows.py; every device comparison is exact."""
import numpy as np

from ensemble_restatement import CANON, canon, filled, is_nan_bits
from pair_hits_restatement import ord32

MAX_LEN = 8192
LETTERS = "ACDEFGHIKLMNPQRSTVWY"


def codes(seq):
    """A letter string -> int32 codes: the 20 letters 0 .. 19, 'X' 20, anything else ('-') 21."""
    return np.array([LETTERS.index(c) if c in LETTERS else (20 if c == "X" else 21) for c in seq], np.int32).reshape(-1)


def _keys(a, other):
    """Codes -> keys that compare equal exactly where the codes match: a code outside [0, 20) becomes ``other`` (< 0)."""
    a = np.asarray(a).astype(np.int64).reshape(-1)
    return np.where((a >= 0) & (a < 20), a, other)


def scores(a, b):
    """-> sk [(n + m + 1), n + 1] uint16 with sk[i + j, i] = score[i][j] for 0 <= i <= n, 0 <= j <= m."""
    ka, kb = _keys(a, -1), _keys(b, -2)
    n, m = len(ka), len(kb)
    sk = np.zeros((n + m + 1, n + 1), np.uint16)
    for d in range(n + m - 2, -1, -1):
        lo, hi = max(0, d - (m - 1)), min(n - 1, d)
        match = ka[lo:hi + 1] == kb[d - hi:d - lo + 1][::-1]
        best = sk[d + 2, lo + 1:hi + 2] + match.astype(np.uint16)
        np.maximum(best, sk[d + 1, lo + 1:hi + 2], out=best)
        np.maximum(best, sk[d + 1, lo:hi + 1], out=best)
        sk[d, lo:hi + 1] = best
    return sk


def align_map(a, b, rule="contract"):
    """-> (out [n] int64: the index in b aligned to a[q], or -1; the number of aligned columns)."""
    ka, kb = _keys(a, -1), _keys(b, -2)
    n, m = len(ka), len(kb)
    out = np.full(n, -1, np.int64)
    if n == 0 or m == 0:
        return out, 0
    sk = scores(a, b)
    sc = lambda i, j: int(sk[i + j, i])
    i = j = count = 0
    while i < n and j < m:
        diagonal = ka[i] == kb[j] and sc(i, j) == sc(i + 1, j + 1) + 1
        down = sc(i, j) == sc(i + 1, j)
        if rule == "down_first":
            diagonal = diagonal and not down
        else:
            assert rule == "contract"
        if diagonal:
            out[i] = j
            count, i, j = count + 1, i + 1, j + 1
        elif down:
            i += 1
        else:
            assert sc(i, j) == sc(i, j + 1)                            # the mismatch column of global_alignment_map cannot fire
            j += 1
    return out, count


def lcs_brute(a, b):
    """The LCS length of two short code sequences by trying every subsequence of a (matching codes only)."""
    ka, kb = [int(v) for v in _keys(a, -1)], [int(v) for v in _keys(b, -2)]
    best = 0
    for mask in range(1 << len(ka)):
        sub = [ka[i] for i in range(len(ka)) if mask >> i & 1]
        if len(sub) <= best:
            continue
        j = 0
        for c in sub:
            while j < len(kb) and kb[j] != c:
                j += 1
            if j == len(kb):
                break
            j += 1
        else:
            best = len(sub)
    return best


def pair_ok(d, NA, NB, NO, max_n, max_m):
    a0, n, b0, m, out0, _ = (int(v) for v in d)
    return min(a0, n, b0, m, out0) >= 0 and n <= max_n and m <= max_m and a0 + n <= NA and b0 + m <= NB and out0 + n <= NO


def align_reference(A, B, desc, NO, max_n, max_m, out=None, aligned=None):
    """One call. A, B: code arrays, desc [P, 6] = (a0, n, b0, m, out0, add). ``out`` / ``aligned``: prefilled buffers (not modified;
    a pair that fails its check leaves its entries), default -1 / 0. -> dict(out [NO] int32, aligned [P], status [P])."""
    A, B = np.asarray(A).reshape(-1), np.asarray(B).reshape(-1)
    desc = np.asarray(desc).astype(np.int64).reshape(-1, 6)
    res_out = np.full(NO, -1, np.int32) if out is None else np.array(out, np.int32)
    res_al = np.zeros(len(desc), np.int32) if aligned is None else np.array(aligned, np.int32)
    status = np.zeros(len(desc), np.int32)
    for p, d in enumerate(desc):
        if not pair_ok(d, len(A), len(B), NO, max_n, max_m):
            status[p] = -1
            continue
        a0, n, b0, m, out0, add = (int(v) for v in d)
        mp, count = align_map(A[a0:a0 + n], B[b0:b0 + m])
        res_out[out0:out0 + n] = np.where(mp >= 0, ((mp + add + 2 ** 31) % 2 ** 32 - 2 ** 31), -1).astype(np.int32)   # (int32 add)
        res_al[p] = count
    return dict(out=res_out, aligned=res_al, status=status)


# ---- statistics through a row map ---------------------------------------------------------------------------------------------------
def rows_desc_ok(map0, M, L, out0, R, T_out, max_len):
    return min(map0, M, L, out0) >= 0 and L <= max_len and map0 + M * L <= R and out0 + L <= T_out


def gather(ddg, S, rows):
    """(ddg [T, ld], S [T], rows [R]) -> (table [R, 20], S [R]): the table a row map names, S = 20 where the entry names no row."""
    ddg, S = np.asarray(ddg, np.float32), np.asarray(S).astype(np.int64).reshape(-1)
    r = np.asarray(rows).astype(np.int64).reshape(-1)
    inside = (r >= 0) & (r < ddg.shape[0])
    at = np.where(inside, r, 0)
    if ddg.shape[0] == 0:
        return np.zeros((len(r), 20), np.float32), np.full(len(r), 20, np.int32)
    return np.ascontiguousarray(ddg[at, :20]), np.where(inside, S[at], 20).astype(np.int32)


def ensemble_rows_reference(ddg, S, rows, desc, T_out, max_len, cutoff=None, out=None):
    """tmpnn_ensemble_stats_rows, one call: desc [E, 4] = (map0, M, L, out_row0); member m's position q reads table row
    rows[map0 + m L + q] and is out where that is no row of the table. -> the eight arrays and status [E]."""
    ddg = np.asarray(ddg, dtype=np.float32)
    T = ddg.shape[0]
    S = np.asarray(S).astype(np.int64).reshape(T)
    rows = np.asarray(rows).astype(np.int64).reshape(-1)
    desc = np.asarray(desc).astype(np.int64).reshape(-1, 4)
    cut = np.float32(np.inf if cutoff is None else cutoff)
    res = {k: np.array(v) for k, v in (filled(T_out) if out is None else out).items()}
    status = np.zeros(len(desc), np.int32)
    zero = np.zeros(20, np.float32)
    for e, (map0, M, L, out0) in enumerate(tuple(int(v) for v in d) for d in desc):
        if not rows_desc_ok(map0, M, L, out0, len(rows), T_out, max_len):
            status[e] = -1
            continue
        with np.errstate(all="ignore"):
            for q in range(L):
                part = []                                                # (m, the row's 20 values, which of them take part)
                for m in range(M):
                    r = int(rows[map0 + m * L + q])
                    if 0 <= r < T and 0 <= int(S[r]) < 20:
                        x = ddg[r, :20]
                        part.append((m, x, ~is_nan_bits(x.view(np.uint32))))
                s, n, below = zero.copy(), np.zeros(20, np.int32), np.zeros(20, np.int32)
                o_lo, o_hi = np.zeros(20, np.uint32), np.zeros(20, np.uint32)
                x_lo, x_hi = np.full(20, CANON, np.uint32), np.full(20, CANON, np.uint32)
                m_lo, m_hi = np.full(20, -1, np.int32), np.full(20, -1, np.int32)
                for m, x, p in part:                                     # ascending m
                    o, xb = ord32(x.view(np.uint32)), x.view(np.uint32)
                    s = np.where(p, s + x, s)
                    lower, higher = p & ((n == 0) | (o < o_lo)), p & ((n == 0) | (o > o_hi))
                    o_lo, x_lo, m_lo = np.where(lower, o, o_lo), np.where(lower, xb, x_lo), np.where(lower, m, m_lo)
                    o_hi, x_hi, m_hi = np.where(higher, o, o_hi), np.where(higher, xb, x_hi), np.where(higher, m, m_hi)
                    n = n + p
                    below = below + (p & (x <= cut))
                fn = np.maximum(n, 1).astype(np.float32)
                mean = s / fn
                t = zero.copy()
                for m, x, p in part:
                    d = x - mean
                    dd = d * d
                    t = np.where(p, t + dd, t)
                assert s.dtype == np.float32 and t.dtype == np.float32 and mean.dtype == np.float32
                spread = np.sqrt(t / fn)
                none = n == 0
                at = out0 + q
                res["mean"][at] = canon(np.where(none, np.float32(np.nan), mean))
                res["spread"][at] = canon(np.where(none, np.float32(np.nan), spread))
                res["lo"][at], res["hi"][at] = x_lo.view(np.float32), x_hi.view(np.float32)
                res["lo_member"][at], res["hi_member"][at], res["count"][at], res["below"][at] = m_lo, m_hi, n, below
    res["status"] = status
    return res
