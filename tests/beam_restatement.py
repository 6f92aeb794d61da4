"""The contract of tmpnn_beam_step (include/tmpnn.h) restated in numpy: every candidate of a beam, the np.float32 sum, its integer
order key, np.lexsort over (key, member, position, letter), then the walk in that order with an exact comparison of child sets (Python
tuples in a set) until k are kept; outputs and padding. Shared by tests/test_beam_host.py and tests/test_gpu_beam.py; every device
comparison against it is exact."""
import numpy as np

from pair_hits_restatement import ord32, unord32

CYS = 1                                  # 'C' in ACDEFGHIKLMNPQRSTVWYX
MAX_LEN, MAX_V, MAX_DEPTH, MAX_KD = 2048, 65536, 8, 256
OUTPUTS = ("out_muts", "out_score", "out_parent", "out_S", "out_count")


def pack_sub(q, b):
    """A substitution's word: q << 5 | b."""
    return (np.asarray(q, dtype=np.int64) << 5) | np.asarray(b, dtype=np.int64)


def _muts(muts, V, depth):
    return np.zeros((V, 0), np.int64) if muts is None or depth == 1 else np.asarray(muts).astype(np.int64).reshape(V, depth - 1)


def ordered_candidates(ddg, S_var, score, muts, depth, allowed=None, cutoff=None, include_cys=False):
    """ddg [V, L, >= 20] float32, S_var [V, L], score [V], muts [V, depth - 1] or None -> (o uint32, v, q, b int64): every candidate
    of the step in ascending key order."""
    ddg = np.asarray(ddg, dtype=np.float32)[:, :, :20]
    V, L = ddg.shape[:2]
    s = np.asarray(S_var).astype(np.int64).reshape(V, L)[:, :, None]
    score = np.asarray(score, dtype=np.float32).reshape(V)
    muts = _muts(muts, V, depth)
    cut = np.float32(np.inf if cutoff is None else cutoff)
    with np.errstate(invalid="ignore", over="ignore"):              # inf - inf: the NaN is the point
        val = score[:, None, None] + ddg                            # np.float32 + np.float32: one IEEE add
        ok = ~np.isnan(val) & (val <= cut)
    assert val.dtype == np.float32
    q = np.arange(L, dtype=np.int64)[None, :, None]
    b = np.arange(20, dtype=np.int64)[None, None, :]
    alive = (muts >= 0).all(1)
    ok &= alive[:, None, None] & (s >= 0) & (s < 20) & (b != s)
    for c in range(muts.shape[1]):
        ok &= q != (muts[:, c] >> 5)[:, None, None]
    if allowed is not None:
        ok &= (np.asarray(allowed).reshape(L) != 0)[None, :, None]
    if not include_cys:
        ok &= b != CYS
    v_i, q_i, b_i = (x.astype(np.int64) for x in np.nonzero(ok))
    o = ord32(val[ok].view(np.uint32))
    order = np.lexsort((b_i, q_i, v_i, o))
    return o[order], v_i[order], q_i[order], b_i[order]


def child_set(muts, depth, v, q, b):
    """muts[v] with q << 5 | b added, ascending, as a tuple."""
    own = () if muts is None or depth == 1 else tuple(int(e) for e in np.asarray(muts).reshape(-1, depth - 1)[v])
    return tuple(sorted(own + (int(q) << 5 | int(b),)))


def beam_step_reference(ddg, S_var, score, muts, depth, k, allowed=None, cutoff=None, include_cys=False):
    """One step. -> dict(out_muts [k, depth] int32 padded with -1, out_score [k] float32 padded with NaN (a -0.0 sum as +0.0),
    out_parent [k] int32 padded with -1, out_S [k, L] int32 padded with 20, out_count [1] int32) and, for the tests of the fixtures,
    ``dropped`` (the duplicates the walk passed over before it stopped) and ``walked`` (the candidates it looked at)."""
    S_var = np.asarray(S_var).astype(np.int64)
    V, L = S_var.shape
    o, v, q, b = ordered_candidates(ddg, S_var, score, muts, depth, allowed, cutoff, include_cys)
    out = dict(out_muts=np.full((k, depth), -1, np.int32), out_score=np.full(k, np.nan, np.float32), out_parent=np.full(k, -1, np.int32),
               out_S=np.full((k, L), 20, np.int32), out_count=np.zeros(1, np.int32))
    seen, n, dropped, i = set(), 0, 0, 0
    while i < len(o) and n < k:
        cs = child_set(muts, depth, v[i], q[i], b[i])
        if cs in seen:
            dropped += 1
        else:
            seen.add(cs)
            out["out_muts"][n] = cs
            out["out_score"][n] = unord32(o[i:i + 1]).view(np.float32)[0]
            out["out_parent"][n] = v[i]
            out["out_S"][n] = S_var[v[i]]
            out["out_S"][n, q[i]] = b[i]
            n += 1
        i += 1
    out["out_count"][0] = n
    out["dropped"], out["walked"] = dropped, i
    return out


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def assert_beam_equal(got, want):
    """Exact: the count, every substitution, parent and sequence row, padding included, and the score BITS (a NaN is a NaN)."""
    g = {name: _np(got[name]) for name in OUTPUTS}
    np.testing.assert_array_equal(g["out_count"].reshape(-1), want["out_count"])
    for name in ("out_muts", "out_parent", "out_S"):
        assert g[name].shape == want[name].shape, name
        np.testing.assert_array_equal(g[name], want[name], err_msg=name)
    a, b = g["out_score"].astype(np.float32).view(np.uint32), want["out_score"].view(np.uint32)
    nan_a, nan_b = (a & 0x7fffffff) > 0x7f800000, (b & 0x7fffffff) > 0x7f800000
    np.testing.assert_array_equal(nan_a, nan_b)
    np.testing.assert_array_equal(a[~nan_a], b[~nan_b])
    assert not (a == 0x80000000).any()                              # a -0.0 sum comes back as +0.0


# ---- the duplicate fixture --------------------------------------------------------------------------------------------------------
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
FILL = np.array([-0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, np.nan, np.inf], np.float32)         # a pool member's other entries: ties, none below zero
LOOSE = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, np.nan, np.inf], np.float32)   # the unrelated members' entries


def duplicate_fixture(depth, V, L, seed, n_pool=6, ld=21):
    """A beam whose best children are reached by ``depth`` paths each. Its first members are ALL (depth - 1)-subsets of a pool of
    ``n_pool`` substitutions at ``n_pool`` sites (weights -4, -3.75, ...; a member's score is the sum of its weights plus a few ulps
    of path dependence, and its table holds, at each pool site it lacks, that substitution's weight plus a few ulps: the bottom of the
    finite range — every other entry of such a member is >= 0, +inf or NaN). A child set made of pool substitutions has ``depth``
    parents in the beam. Unrelated distinct members (entries >= -3, scores >= -1; one dead, one with a NaN score) fill the beam up to
    V. Letters < 0 and >= 20 occur away from the pool sites. -> dict(ddg, S_var, score, muts, depth, pool)."""
    from itertools import combinations
    rng = np.random.default_rng(seed)
    sites = np.linspace(0, L - 1, n_pool).astype(np.int64)                                   # the first and the last row among them
    assert len(set(sites.tolist())) == n_pool
    letters = np.array([(3 + 2 * i) % 20 for i in range(n_pool)], np.int64)                 # none is cysteine
    assert (letters != CYS).all()
    weight = (-4.0 + 0.25 * np.arange(n_pool)).astype(np.float32)
    members = list(combinations(range(n_pool), depth - 1))
    assert len(members) <= V and (depth > 1 or V == 1)                                       # (depth 1: the wild type alone)
    ddg = LOOSE[rng.integers(0, len(LOOSE), size=(V, L, ld))]
    S_var = rng.integers(-2, 22, size=(V, L)).astype(np.int32)
    score = np.array([0.0, 1.0, -1.0, 0.25], np.float32)[rng.integers(0, 4, size=V)]
    muts = np.zeros((V, depth - 1), np.int32)
    tiny = np.float32(2.0 ** -10)
    for v, mem in enumerate(members):
        ddg[v] = FILL[rng.integers(0, len(FILL), size=(L, ld))]
        S_var[v, sites] = (letters + 1 + rng.integers(0, 18, size=n_pool)) % 20              # a letter, and not the pool's
        S_var[v, sites[list(mem)]] = letters[list(mem)]
        muts[v] = pack_sub(sites[list(mem)], letters[list(mem)])
        score[v] = np.float32(weight[list(mem)].sum(dtype=np.float32) + tiny * np.float32(rng.integers(-1, 2)))
        for z in range(n_pool):
            if z not in mem:
                ddg[v, sites[z], letters[z]] = weight[z] + np.float32(0.5) * tiny * np.float32(rng.integers(0, 2))
    free = np.setdiff1d(np.arange(L), sites)
    taken = set()
    for v in range(len(members), V):                                                         # unrelated members: distinct sets away from the pool
        while True:
            pos = np.sort(rng.choice(free, size=depth - 1, replace=False))
            let = rng.integers(0, 20, size=depth - 1)
            if tuple(pack_sub(pos, let)) not in taken:
                break
        taken.add(tuple(pack_sub(pos, let)))
        S_var[v, pos] = let
        muts[v] = pack_sub(pos, let)
    if V > len(members) + 1 and depth > 1:
        muts[V - 1, -1] = -1                                                                 # a dead member
        score[V - 2] = np.nan                                                                # and one that contributes nothing
    alive = [tuple(m) for m in muts.tolist() if min(m, default=0) >= 0]
    assert len(set(alive)) == len(alive)                                                     # the caller's promise
    if depth > 1:
        top = np.sort(weight)[-depth:].sum() + 2 * tiny                                      # the worst pool child lies under every other candidate
        assert top < min(float(np.nanmin(score[:len(members)])), -4.0)
    return dict(ddg=ddg, S_var=S_var, score=score, muts=muts if depth > 1 else None, depth=depth,
                pool=set(int(x) for x in pack_sub(sites, letters)))
