"""The inputs of tests/test_gpu_variant_rounding.py (tests/variant_inputs.py), the parts that need no GPU: the honesty conditions of
every input — sums that round, winners that rounded, specials at candidate sites, summation orders that show; the three numpy
restatements held to the plain Python loops of the sibling host tests and to the float64 sum rounded once, on these inputs; and the
SENSITIVITY of the inputs: a pair map summed in descending b or folded in descending v, a sum whose denormal result is flushed to a
signed zero, and a NaN test made by the cutoff compare of the order words alone each differ from the restatement on the very inputs
the GPU tests use. That is how a subtly wrong kernel is shown to fail those tests without building one."""
import numpy as np
import pytest

import variant_inputs as vi
from beam_restatement import assert_beam_equal, ordered_candidates
from hits_inputs import assert_table_is_hostile
from pair_hits_restatement import CYS, MAX_TAG, NONE, ord32, pack_low
from pair_map_restatement import assert_pair_map_equal
from test_beam_host import _brute as brute_beam
from test_pair_hits_host import _brute as brute_hits
from test_pair_map_host import _brute as brute_map, _fresh

ROWS_A = np.repeat([2, 0, 4, 1, 3], [1, 19, 5, 11, 1]).astype(np.int32)
ROWS_B = np.repeat([0, 3, 1, 4, 2], [20, 1, 1, 14, 1]).astype(np.int32)
ROWS_C = np.repeat([2, 0, vi.PMAP_R, 1, -1], [1, 19, 5, 11, 1]).astype(np.int32)
INF_IMAGE = int(ord32(np.array([0x7f800000], np.uint32))[0])


@pytest.fixture(scope="module")
def hits_cases():
    return vi.hits_rounding_cases()


@pytest.fixture(scope="module")
def beams():
    return {d: vi.rounding_beam(d) for d in sorted(vi.BEAM_POOL)}


# ---- honesty ----------------------------------------------------------------------------------------------------------------------
def test_rounding_tables_are_what_they_say():
    ddg, base, wt = vi.rounding_table(37, 300, 11)
    for x in (ddg, base, wt):
        bits = x.view(np.uint32)
        expo = (bits >> 23) & 0xff
        assert x.dtype == np.float32 and np.isfinite(x).all() and expo.min() == vi.EXP_LO and expo.max() == vi.EXP_HI
    assert (ddg < 0).mean() > 0.4 and (ddg > 0).mean() > 0.4 and len(np.unique(ddg.view(np.uint32) & 0x7fffff)) > 200000
    assert vi.assert_table_rounds(ddg, base) >= 0.7                          # (0.82 measured)
    assert vi.inexact(ddg[:, :, :20], wt[None, :, :20], minus=True).mean() >= 0.7
    h, hb = vi.hostile_table(12, 70, 21)
    assert h.shape == (12, 70, 21) and hb.shape == (12,) and np.isnan(h).mean() > 0.2


def test_hits_inputs_meet_their_conditions(hits_cases):
    dense, sparse, planted = hits_cases
    vi.assert_table_rounds(dense["ddg"], dense["base"])
    assert len(set(dense["tag"].tolist())) == 37 and (dense["S_var"] < 0).any() and (dense["S_var"] == 20).any()
    special = {(v, q, b) for v, q, b, _ in planted["sites"]}
    assert planted["n_top"] <= vi.TOP_LIMIT_K // 4 and len(special) == len(planted["sites"]) == 17
    for c in (dense, sparse):
        vi.assert_specials_are_candidates(c["ddg"], c["base"], c["S_var"], planted, planted["blocked"])
    v_of = {int(t): v for v, t in enumerate(dense["tag"])}
    for i, k in enumerate(vi.HITS_KS):
        kw = vi.hits_flags(i)
        want = vi.hits_ref(dense, k, **kw)
        assert int(want["hit_count"][0]) == k
        mine = sum((v_of[int(t)], int(q), int(b)) in special for t, q, b in zip(want["hit_tag"], want["hit_pos"], want["hit_aa"]))
        assert mine <= min(k, 2) or mine <= k // 4, (k, mine)                 # the specials lead and do not fill the list
        if k >= 32:
            assert vi.winners_inexact(dense, want).mean() >= 1 / 3, k
        assert not np.isnan(want["hit_ddg"]).any()
    full = vi.hits_ref(sparse, 256, include_cys=True)
    n = int(full["hit_count"][0])
    bits = full["hit_ddg"][:n].view(np.uint32)
    assert 64 < n < 256 and ((bits & 0x7fffffff > 0) & (bits & 0x7fffffff < 0x00800000)).sum() == 3              # every denormal sum is listed
    assert (bits == 0xff800000).sum() == 2 and (bits == 0x7f800000).sum() >= 2 and (bits == 0).sum() >= 17 and not (bits == 0x80000000).any()
    hostile = vi.hits_hostile_case()
    assert_table_is_hostile(hostile["ddg"].reshape(-1, 21), hostile["S_var"].reshape(-1))
    for m in (2, 4, 8, 16, 32, 64, 128, 256):
        c = vi.hits_cap_case(m)
        V = len(c["tag"])
        want = vi.hits_ref(c, m)
        assert V == 8192 // m + 5 and set(want["hit_tag"][:min(m, 6)].tolist()) <= set(c["tag"][V - 6:].tolist())
        assert vi.winners_inexact(c, want)[:min(m, 6)].any()


def test_pair_map_inputs_meet_their_conditions():
    for (L, ld), c in vi.pmap_crafted().items():
        assert c["ddg"].shape == (37, L, ld) and vi.inexact(c["ddg"][:, :, :20], c["wt"][None, :, :20], minus=True).mean() >= 0.5
        for rows, kw in ((ROWS_A, dict()), (ROWS_B, dict(upper=True)), (ROWS_C, dict(no_skip=True))):
            share_b, share_v = vi.assert_pair_map_order_shows(c, rows, vi.PMAP_R, **kw)
            assert share_b >= 0.5                                             # (0.64 measured on such draws)
        want = vi.pmap_ref(c, ROWS_A, vi.PMAP_R)
        busy = want["count"] >= 20
        finite = busy & np.isfinite(want["eps_abs_sum"])
        assert finite.sum() >= 20 and np.isinf(want["eps_abs_sum"]).any() and not np.isnan(want["eps_abs_sum"]).any()
    for L, (c, rows, R) in vi.pmap_short_cases().items():
        vi.assert_pair_map_order_shows(c, rows, R, runs=L <= 2)
    c, rows, R = vi.pmap_long_run_case()
    vi.assert_pair_map_order_shows(c, rows, R)


def test_beam_inputs_meet_their_conditions(beams):
    assert sorted({max(2, 1 << (d * k - 1).bit_length()) for d, k in vi.BEAM_PAIRS}) == [2, 4, 8, 16, 32, 64, 128, 256]
    for d, k in vi.BEAM_PAIRS:
        fx = beams[d]
        alive = [tuple(m) for m in fx["muts"].tolist()] if d > 1 else []
        assert len(set(alive)) == len(alive)                                  # the caller's promise
        for cys in (False, True):
            want = vi.beam_ref(fx, k, include_cys=cys)
            assert int(want["out_count"][0]) == k
            # the -inf child's second path is dropped at once; from k = 4 on the walk also passes the leading pool child's d paths
            assert d == 1 or want["dropped"] >= (d if k >= 4 else 1), (d, k, want["dropped"])
            if k >= 32:
                assert vi.beam_winners_inexact(fx, want).mean() >= 1 / 3, (d, k)
    for d, fx in beams.items():
        if d == 1:
            continue
        vi.assert_specials_are_candidates(fx["ddg"], fx["score"], fx["S_var"], fx["planted"], fx["blocked"])
        assert vi.inexact(fx["score"][:, None, None], fx["ddg"][:, :, :20]).mean() >= 0.5
    for k, V, L in ((16, 261, 16), (2, 2053, 104)):
        fx = vi.beam_cap_case(k, V, L)
        want = vi.beam_ref(fx, k)
        assert int(want["out_parent"][0]) >= V - 6 and int(want["out_count"][0]) == k
    fx = vi.hostile_beam()
    assert_table_is_hostile(fx["ddg"].reshape(-1, 21), fx["S_var"].reshape(-1))
    assert len({int(e) for e in fx["muts"][:, 0]}) == 12


# ---- the restatements against independent statements, on these inputs -------------------------------------------------------------
def test_float32_sums_are_the_float64_sums_rounded_once():
    ddg, base, wt = vi.rounding_table(37, 300, 11)
    dense, _, _ = vi.hits_rounding_cases()
    for d, b in ((ddg, base), (dense["ddg"], dense["base"])):
        with np.errstate(invalid="ignore", over="ignore"):
            s = b[:, None, None] + d
        want = vi.rounded_once(b[:, None, None], d)
        ok = ~np.isnan(s)
        assert s.dtype == np.float32 and np.array_equal(s[ok].view(np.uint32), want[ok].view(np.uint32)) and np.isnan(want[~ok]).all()
    e = ddg - wt[None]
    assert e.dtype == np.float32 and np.array_equal(e.view(np.uint32), vi.rounded_once(ddg, wt[None], minus=True).view(np.uint32))


def test_hits_restatement_equals_a_plain_loop_on_these_inputs(hits_cases):
    dense, sparse, _ = hits_cases
    for c in (dense, sparse, vi.hits_hostile_case()):
        for kw in (dict(include_cys=False, upper=True), dict(include_cys=True, upper=False)):
            with np.errstate(over="ignore"):                                  # (3e38 + 3e38: the overflow is the point)
                loop, _ = brute_hits(c["ddg"], c["S_var"], c["base"], c["tag"], c["skip"], 256, None, kw["include_cys"], kw["upper"], [])
            n = int(loop["hit_count"][0])
            for k in (1, 5, 33, 100, 256):
                want = vi.hits_ref(c, k, **kw)
                m = min(k, n)
                assert int(want["hit_count"][0]) == m
                for name in ("hit_tag", "hit_pos", "hit_aa"):
                    np.testing.assert_array_equal(want[name][:m], loop[name][:m], err_msg=name)
                a, b = want["hit_ddg"][:m].view(np.uint32).copy(), loop["hit_ddg"][:m].view(np.uint32).copy()
                a[a == 0x80000000], b[b == 0x80000000] = 0, 0
                np.testing.assert_array_equal(a, b)


def test_pair_map_restatement_equals_a_plain_loop_on_these_inputs():
    crafted = vi.pmap_crafted()
    short = vi.pmap_short_cases()
    cases = [(crafted[19, 21], ROWS_A, vi.PMAP_R, dict()), (crafted[19, 20], ROWS_C, vi.PMAP_R, dict(include_cys=True, upper=True)),
             (crafted[70, 20], ROWS_B, vi.PMAP_R, dict(upper=True)), (short[1][0], short[1][1], 4, dict()), (short[2][0], short[2][1], 4, dict(upper=True)),
             (short[257][0], short[257][1], 4, dict(include_cys=True))]
    for c, rows, R, kw in cases:
        L = c["S_var"].shape[1]
        want = vi.pmap_ref(c, rows, R, **kw)
        loop, _ = brute_map(dict(c, row=rows), slice(None), R, kw.get("include_cys", False), kw.get("upper", False), _fresh(R, L))
        assert_pair_map_equal(want, loop)
    c, rows, R = vi.pmap_long_run_case()
    want = vi.pmap_ref(c, rows, R)
    state, carried = None, _fresh(R, 5)
    for v0, v1 in ((0, 1), (1, 299), (299, 599), (599, 612)):                 # the GPU test's cuts, a state carried by both
        state = vi.pmap_ref(c, rows, R, sl=slice(v0, v1), state=state)
        loop, carried = brute_map(dict(c, row=rows), slice(v0, v1), R, False, False, carried)
        assert_pair_map_equal(state, loop)
    assert_pair_map_equal(state, want)


def test_beam_restatement_equals_a_plain_loop_on_these_inputs(beams):
    with np.errstate(over="ignore"):                                          # (3e38 + 3e38: the overflow is the point)
        _beam_loops(beams)


def _beam_loops(beams):
    for d, k in vi.BEAM_PAIRS:
        fx = beams[d]
        for cys in (False, True):
            assert_beam_equal(vi.beam_ref(fx, k, include_cys=cys), brute_beam(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], d, k, None, None, cys))
    thin, allowed = vi.sparse_beam(beams[3])
    assert_beam_equal(vi.beam_ref(thin, 85, allowed=allowed), brute_beam(thin["ddg"], thin["S_var"], thin["score"], thin["muts"], 3, 85, allowed, None, False))
    fx = vi.hostile_beam()
    assert_beam_equal(vi.beam_ref(fx, 64), brute_beam(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], 2, 64, None, None, False))
    fx = vi.beam_cap_case(16, 261, 16)
    assert_beam_equal(vi.beam_ref(fx, 16), brute_beam(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], 2, 16, None, None, False))


# ---- sensitivity: subtly wrong kernels, restated ------------------------------------------------------------------------------------
def _images(ddg, base, how):
    """-> (order words [V, L, 20], the sums a kernel's NaN test removes) for a kernel that is right (None), that flushes a denormal sum
    to a signed zero ("flush"), or whose only NaN test is the cutoff compare of the order words ("le": a NEGATIVE NaN's word is near
    zero and passes it)."""
    with np.errstate(invalid="ignore", over="ignore"):
        val = np.asarray(base, np.float32)[:, None, None] + ddg[:, :, :20]
    if how == "flush":
        val = _flushed(val)
    o = ord32(val.view(np.uint32))
    return o, (np.isnan(val) if how != "le" else np.zeros(val.shape, bool))


def _flushed(x):
    bits = x.view(np.uint32)
    tiny = (bits & 0x7fffffff > 0) & (bits & 0x7fffffff < 0x00800000)
    return np.where(tiny, (bits & np.uint32(0x80000000)).view(np.float32), x).astype(np.float32)


def _hits_keys(c, k, how, include_cys=False, upper=False):
    """The k smallest keys of a call (no cutoff: the compare is against +inf's word), by a kernel of the given kind."""
    o, gone = _images(c["ddg"], c["base"], how)
    V, L = c["S_var"].shape
    s, q, b = c["S_var"].astype(np.int64)[:, :, None], np.arange(L)[None, :, None], np.arange(20)[None, None, :]
    skip, tag = c["skip"].astype(np.int64)[:, None, None], c["tag"].astype(np.int64)
    ok = ~gone & (o <= INF_IMAGE) & ((tag >= 0) & (tag <= MAX_TAG))[:, None, None] & (s >= 0) & (s < 20) & (b != s)
    ok &= ((q > skip) if upper else (q != skip)) & (include_cys | (b != CYS))
    v_i, q_i, b_i = np.nonzero(ok)
    keys = np.sort((o[ok].astype(np.uint64) << np.uint64(32)) | pack_low(tag[v_i], q_i, b_i))[:k]
    return np.concatenate([keys, np.full(k - len(keys), NONE, np.uint64)])


def _beam_keys(fx, how, include_cys=False, allowed=None):
    """Every candidate key of a step in ascending order (hits word << 32 | v << 16 | q << 5 | b), by a kernel of the given kind."""
    o, gone = _images(fx["ddg"], fx["score"], how)
    V, L = fx["S_var"].shape
    s, q, b = fx["S_var"].astype(np.int64)[:, :, None], np.arange(L)[None, :, None], np.arange(20)[None, None, :]
    muts = np.zeros((V, 0), np.int64) if fx["muts"] is None else fx["muts"].astype(np.int64)
    ok = ~gone & (o <= INF_IMAGE) & (muts >= 0).all(1)[:, None, None] & (s >= 0) & (s < 20) & (b != s) & (include_cys | (b != CYS))
    for col in range(muts.shape[1]):
        ok &= q != (muts[:, col] >> 5)[:, None, None]
    if allowed is not None:
        ok &= (allowed != 0)[None, :, None]
    v_i, q_i, b_i = (x.astype(np.uint64) for x in np.nonzero(ok))
    return np.sort((o[ok].astype(np.uint64) << np.uint64(32)) | (v_i << np.uint64(16)) | (q_i << np.uint64(5)) | b_i)


def _true_beam_keys(fx, include_cys=False, allowed=None):
    o, v, q, b = ordered_candidates(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], fx["depth"], allowed, None, include_cys)
    return (o.astype(np.uint64) << np.uint64(32)) | (v.astype(np.uint64) << np.uint64(16)) | (q.astype(np.uint64) << np.uint64(5)) | b.astype(np.uint64)


def test_a_flushed_denormal_or_a_nan_test_by_compare_changes_the_hit_lists(hits_cases):
    dense, sparse, _ = hits_cases
    hostile = vi.hits_hostile_case()
    for i, k in enumerate(vi.HITS_KS):
        kw = vi.hits_flags(i)
        for c in (dense, sparse, hostile):
            want = vi.hits_ref(c, k, **kw)["state"]
            np.testing.assert_array_equal(_hits_keys(c, k, None, **kw), want)            # the scaffold itself is right
            assert not np.array_equal(_hits_keys(c, k, "le", **kw), want), k             # a negative NaN would lead every list
        if k >= 100:                                                                     # the sparse lists reach the denormal sums
            assert not np.array_equal(_hits_keys(sparse, k, "flush", **kw), vi.hits_ref(sparse, k, **kw)["state"]), k
    # ... and at the cutoff test's own call
    assert not np.array_equal(_hits_keys(sparse, 256, "flush", include_cys=True), vi.hits_ref(sparse, 256, include_cys=True)["state"])


def test_a_flushed_denormal_or_a_nan_test_by_compare_changes_the_beam(beams):
    for d, k in vi.BEAM_PAIRS:
        if d == 1:
            continue                                                          # (the wild type alone carries no specials)
        fx = beams[d]
        for cys in (False, True):
            true = _true_beam_keys(fx, cys)
            np.testing.assert_array_equal(_beam_keys(fx, None, cys), true)
            assert _beam_keys(fx, "le", cys)[0] != true[0]                    # the first key is always kept: the first output row differs
        if k >= 64:
            thin, allowed = vi.sparse_beam(fx)
            true, wrong = _true_beam_keys(thin, False, allowed), _beam_keys(thin, "flush", False, allowed)
            np.testing.assert_array_equal(_beam_keys(thin, None, False, allowed), true)
            n = int(vi.beam_ref(thin, k, allowed=allowed)["out_count"][0])    # distinct members away from the pool: no duplicates, the
            assert len(true) >= n and not np.array_equal(wrong[:n], true[:n]), (d, k)      # first n keys ARE the output
            assert vi.beam_ref(thin, k, allowed=allowed)["dropped"] == 0
    fx = vi.hostile_beam()
    true = _true_beam_keys(fx)
    np.testing.assert_array_equal(_beam_keys(fx, None), true)
    assert _beam_keys(fx, "le")[0] != true[0]


def test_a_reversed_order_a_flushed_denormal_or_a_nan_test_by_compare_changes_the_pair_map():
    """The reversed orders are vi.assert_pair_map_order_shows (above, on every input). Here the other two, by feeding the restatement
    tables that make it compute what the wrong kernel would: a denormal e flushed = the entry set to wt's (e = +0.0; the value
    base + entry keeps its bits); a negative NaN e let through the NaN test is counted = the entry set to a number."""
    for (L, ld), c in vi.pmap_crafted().items():
        with np.errstate(invalid="ignore", over="ignore"):
            e = c["ddg"][:, :, :20] - c["wt"][None, :, :20]
            val = c["base"][:, None, None] + c["ddg"][:, :, :20]
        eb = e.view(np.uint32)
        tiny = (eb & 0x7fffffff > 0) & (eb & 0x7fffffff < 0x00800000)
        neg_nan = np.isnan(e) & (eb >> 31 == 1)
        assert tiny.sum() >= 1 and neg_nan.sum() >= 1
        flushed, counted = c["ddg"].copy(), c["ddg"].copy()
        flushed[:, :, :20] = np.where(tiny, np.broadcast_to(c["wt"][None, :, :20], e.shape), c["ddg"][:, :, :20])
        with np.errstate(invalid="ignore", over="ignore"):
            same = (c["base"][:, None, None] + flushed[:, :, :20]).view(np.uint32) == val.view(np.uint32)
        assert (same | np.isnan(val)).all()
        counted[:, :, :20] = np.where(neg_nan, np.float32(1.0), c["ddg"][:, :, :20])
        for rows in (ROWS_A, ROWS_B):
            for kw in (dict(), dict(include_cys=True), dict(upper=True), dict(include_cys=True, upper=True), dict(no_skip=True)):
                want = vi.pmap_ref(c, rows, vi.PMAP_R, **kw)
                wrong = vi.pmap_ref(dict(c, ddg=flushed), rows, vi.PMAP_R, **kw)
                assert not np.array_equal(wrong["eps_lo"], want["eps_lo"]) or not np.array_equal(wrong["eps_hi"], want["eps_hi"]) or \
                    not np.array_equal(wrong["eps_abs_sum"].view(np.uint32), want["eps_abs_sum"].view(np.uint32)), (L, ld, kw)
                assert not np.array_equal(vi.pmap_ref(dict(c, ddg=counted), rows, vi.PMAP_R, **kw)["count"], want["count"]), (L, ld, kw)
