"""Crafted inputs for tmpnn_align_global and tmpnn_ensemble_stats_rows, shared by tests/test_align_host.py, tests/test_gpu_align.py and
tests/test_gpu_ensemble_rows.py, which therefore see the same sequences; no GPU, no torch. Kinds of a pair (a [n], b [m]):
  "two"        both over a two-letter alphabet: almost every cell ties, so the tie rule of the trace decides the map
  "twenty"     both over the 20 letters
  "identical"  b = a (m is ignored): the map must be the identity
  "disjoint"   a over letters 0 .. 9, b over 10 .. 19: nothing aligns
  "deletions"  b = a without 3 terminal (2 at the start, 1 at the end) and 2 internal residues (m is ignored; n >= 8)
  "nonmatch"   a four-letter alphabet with the codes 20, 21, -1 and INT32_MIN mixed in: they match nothing, not even themselves"""
import numpy as np

KINDS = ("two", "twenty", "identical", "disjoint", "deletions", "nonmatch")
SMALL = ((0, 0), (0, 5), (5, 0), (1, 1), (19, 70), (70, 19), (257, 256))
LONG = ((1023, 1025), (2049, 1500))     # diagonals of 1 023 cells (one short of a pass of the 1 024 threads: a last word of 15 cells)
                                        # and of 1 500 (two passes, the second partly filled); word boundaries inside both
ODD = np.array([20, 21, -1, -2 ** 31], np.int64)


def make_pair(kind, n, m, rng):
    if kind == "two":
        a, b = rng.integers(0, 2, n), rng.integers(0, 2, m)
    elif kind == "twenty":
        a, b = rng.integers(0, 20, n), rng.integers(0, 20, m)
    elif kind == "identical":
        a = rng.integers(0, 20, n)
        b = a.copy()
    elif kind == "disjoint":
        a, b = rng.integers(0, 10, n), rng.integers(10, 20, m)
    elif kind == "deletions":
        assert n >= 8
        a = rng.integers(0, 20, n)
        keep = np.ones(n, bool)
        keep[[0, 1, n - 1]] = False
        keep[rng.choice(np.arange(3, n - 2), size=2, replace=False)] = False
        b = a[keep]
    else:
        assert kind == "nonmatch"
        a, b = rng.integers(0, 4, n), rng.integers(0, 4, m)
        a = np.where(rng.random(n) < 0.2, ODD[rng.integers(0, 4, n)], a)
        b = np.where(rng.random(m) < 0.2, ODD[rng.integers(0, 4, m)], b)
    return np.asarray(a, np.int64).astype(np.int32), np.asarray(b, np.int64).astype(np.int32)


def pack(pairs, adds=None):
    """[(a, b)] -> (A, B, desc [P, 6] int32, NO): the strings back to back, every pair's out range behind the one before."""
    A = np.concatenate([p[0] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    B = np.concatenate([p[1] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    desc, a0, b0 = [], 0, 0
    for k, (a, b) in enumerate(pairs):
        desc.append((a0, len(a), b0, len(b), a0, 0 if adds is None else adds[k]))
        a0, b0 = a0 + len(a), b0 + len(b)
    return A, B, np.array(desc, np.int64).reshape(-1, 6).astype(np.int32), a0


def small_batch(seed=11):
    """Every kind at every SMALL size it is defined at, one pair each -> [(kind, n, m, a, b)]."""
    rng = np.random.default_rng(seed)
    out = []
    for n, m in SMALL:
        for kind in KINDS:
            if kind == "deletions" and n < 8:
                continue
            a, b = make_pair(kind, n, m, rng)
            out.append((kind, n, m, a, b))
    return out


def mixed_batch(P=300, seed=12):
    """P pairs of mixed kinds and sizes: mostly 0 .. 90 codes, every 50th pair 257 x 256 -> [(a, b)]."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(P):
        n, m = (257, 256) if k % 50 == 7 else (int(rng.integers(0, 91)), int(rng.integers(0, 91)))
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        if kind == "deletions" and n < 8:
            kind = "two"
        pairs.append(make_pair(kind, n, m, rng))
    return pairs


def draw_rows(c, rng):
    """A row map for a crafted ensemble batch (ensemble_inputs.crafted): per ensemble its members in a random order, then entries
    redirected to -1, T, INT32_MIN, T + 5 and to rows of other members and other ensembles (shared rows). -> rows [sum(M L)] int32
    (desc of the batch serves as (map0, M, L, out_row0) as it is)."""
    T = c["T"]
    rows = np.arange(T, dtype=np.int64)
    for row0, M, L, _ in (tuple(int(v) for v in d) for d in c["desc"]):
        if M > 0:
            rows[row0:row0 + M * L] = (row0 + rng.permutation(M)[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    kind = rng.integers(0, 10, T)
    rows = np.where(kind == 0, -1, rows)
    rows = np.where(kind == 1, T, rows)
    rows = np.where(kind == 2, -2 ** 31, rows)
    rows = np.where(kind == 3, T + 5, rows)
    rows = np.where(kind == 4, rng.integers(0, max(T, 1), T), rows)
    return rows.astype(np.int32)
