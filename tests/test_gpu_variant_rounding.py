"""The three reductions over variant tables on the device — Engine.select_variant_hits, Engine.pair_map, Engine.beam_step — on inputs
whose float work decides places: sums and differences that ROUND, denormal, overflowing, inf - inf and -0.0 sums at candidate sites,
tables of arbitrary bit patterns, every sort width m = 2 .. 256, the workgroup cap at every width with an LDS image of exactly 8 192
keys, runs of 600 variants, proteins of one and two rows, and a state that the grid-stride reset has to stride over. Every comparison
is exact against the numpy restatements (tests/pair_hits_restatement.py, pair_map_restatement.py, beam_restatement.py); the inputs come
from tests/variant_inputs.py, and tests/test_variant_inputs_host.py shows on the restatements alone that these very inputs tell a
reversed summation order, a flushed denormal and a NaN test by compare from the contract."""
import numpy as np
import pytest
import torch

import variant_inputs as vi
from beam_restatement import assert_beam_equal
from hits_inputs import assert_table_is_hostile
from pair_hits_restatement import assert_variant_hits_equal
from pair_map_restatement import STATE, assert_pair_map_equal

pytestmark = pytest.mark.gpu

NAMES = tuple(name for name, _ in STATE)
HIT_OUTPUTS = ("hit_ddg", "hit_tag", "hit_pos", "hit_aa", "hit_count")
ROWS_A = np.repeat([2, 0, 4, 1, 3], [1, 19, 5, 11, 1]).astype(np.int32)      # the row layouts of tests/test_gpu_pair_map.py
ROWS_B = np.repeat([0, 3, 1, 4, 2], [20, 1, 1, 14, 1]).astype(np.int32)
ROWS_C = np.repeat([2, 0, vi.PMAP_R, 1, -1], [1, 19, 5, 11, 1]).astype(np.int32)
PMAP_FLAGS = (dict(), dict(include_cys=True), dict(upper=True), dict(include_cys=True, upper=True), dict(no_skip=True))
LDS_KEYS = 8192                                                               # the LDS image of the sort (csrc/tmpnn_hits.h)


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _pow2(n):
    return max(2, 1 << (n - 1).bit_length())


# ---- variant hits -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hits_cases():
    """(dense, sparse, planted) of variant_inputs.hits_rounding_cases. Left unchanged by the tests that share it."""
    dense, sparse, planted = vi.hits_rounding_cases()
    vi.assert_table_rounds(dense["ddg"], dense["base"])
    for c in (dense, sparse):
        vi.assert_specials_are_candidates(c["ddg"], c["base"], c["S_var"], planted, planted["blocked"])
    return dense, sparse, planted


def _hits(engine, c, k, sl=slice(None), state=None, dev=None, **kw):
    ddg = torch.from_numpy(c["ddg"][sl]).cuda() if dev is None else dev[sl]
    return engine.select_variant_hits(ddg, c["S_var"][sl], c["base"][sl], c["tag"][sl], k, skip=c["skip"][sl], state=state, **kw)


def test_hits_rounding_table_with_specials_at_every_width(engine, hits_cases):
    dense, sparse, _ = hits_cases
    dev = torch.from_numpy(dense["ddg"]).cuda()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), dense["ddg"].view(np.uint32))      # the upload keeps every bit
    widths, seen = set(), set()
    for i, k in enumerate(vi.HITS_KS):
        kw = vi.hits_flags(i)
        widths.add((_pow2(k), kw["include_cys"], kw["upper"]))
        want = vi.hits_ref(dense, k, **kw)
        assert int(want["hit_count"][0]) == k
        if k >= 32:
            share = vi.winners_inexact(dense, want).mean()
            assert share >= 1 / 3, (k, share)                                 # places decided between sums that rounded
        assert_variant_hits_equal(_hits(engine, dense, k, dev=dev, **kw), want)
        thin = vi.hits_ref(sparse, k, **kw)
        assert_variant_hits_equal(_hits(engine, sparse, k, dev=dev, **kw), thin)
        n = int(thin["hit_count"][0])
        bits = thin["hit_ddg"][:n].view(np.uint32)
        seen |= {"denormal"} if ((bits & 0x7fffffff > 0) & (bits & 0x7fffffff < 0x00800000)).any() else set()
        seen |= {"+inf"} if (bits == 0x7f800000).any() else set()
        seen |= {"short"} if n < k else set()
    assert {m for m, _, _ in widths} == {2, 4, 8, 16, 32, 64, 128, 256}
    assert all((m, c, not c) in widths for m in (4, 32, 64, 128, 256) for c in (False, True))
    assert seen == {"denormal", "+inf", "short"}


def test_hits_any_cut_and_any_order_give_the_same_bits_on_rounding_sums(engine, hits_cases):
    dense, _, _ = hits_cases
    dev = torch.from_numpy(dense["ddg"]).cuda()
    cutoff = float(vi.hits_ref(dense, 256, upper=True)["hit_ddg"][180])
    for k, kw in ((5, dict()), (100, dict(upper=True, cutoff=cutoff)), (256, dict(include_cys=True))):
        whole = _hits(engine, dense, k, dev=dev, **kw)
        assert_variant_hits_equal(whole, vi.hits_ref(dense, k, **kw))
        cuts = ([slice(0, 1), slice(1, 37)], [slice(0, 7), slice(7, 37)], [slice(7, 37), slice(0, 7)], [slice(1, 37), slice(0, 1)],
                [slice(30, 37), slice(0, 12), slice(12, 30)])
        for cut in cuts:
            res = state = None
            for sl in cut:
                res = _hits(engine, dense, k, sl=sl, state=state, dev=dev, **kw)
                state = res["state"]
            assert res["state"].dtype == torch.int64 and torch.equal(res["state"], whole["state"]), cut
            for name in HIT_OUTPUTS:
                assert torch.equal(res[name].view(torch.int32), whole[name].view(torch.int32)), (name, cut)


def test_hits_cutoff_on_an_inexact_sum_and_one_ulp_under_it(engine, hits_cases):
    _, sparse, _ = hits_cases
    kw = dict(include_cys=True)
    full = vi.hits_ref(sparse, 256, **kw)
    n = int(full["hit_count"][0])
    assert 64 < n < 256                                                       # fewer candidates than k: the cutoff shows
    ordinary = vi.winners_inexact(sparse, full) & np.isfinite(full["hit_ddg"][:n]) & (np.abs(full["hit_ddg"][:n]) > 2.0 ** -9)
    at = int(min(np.nonzero(ordinary)[0], key=lambda i: abs(i - n // 2)))     # an inexact sum the reference places mid-list
    assert n // 4 < at < 3 * n // 4
    on = float(full["hit_ddg"][at])
    below = float(np.nextafter(np.float32(on), np.float32(-np.inf)))
    got_on, got_below = _hits(engine, sparse, 256, cutoff=on, **kw), _hits(engine, sparse, 256, cutoff=below, **kw)
    assert_variant_hits_equal(got_on, vi.hits_ref(sparse, 256, cutoff=on, **kw))
    assert_variant_hits_equal(got_below, vi.hits_ref(sparse, 256, cutoff=below, **kw))
    n_on, n_below = int(got_on["hit_count"][0]), int(got_below["hit_count"][0])
    assert n_below < n_on < n and float(got_on["hit_ddg"][n_on - 1]) == on and float(got_below["hit_ddg"][n_below - 1]) < on
    assert n_on == at + 1 + int((full["hit_ddg"][at + 1:n] == np.float32(on)).sum())             # the list parts exactly there


def test_hits_hostile_table_at_every_width(engine):
    c = vi.hits_hostile_case()
    assert_table_is_hostile(c["ddg"].reshape(-1, 21), c["S_var"].reshape(-1))
    dev = torch.from_numpy(c["ddg"]).cuda()
    short = False
    for i, k in enumerate(vi.HITS_KS):
        kw = vi.hits_flags(i)
        want = vi.hits_ref(c, k, **kw)
        n = int(want["hit_count"][0])
        short |= 0 < n < k
        assert not np.isnan(want["hit_ddg"][:n]).any() and np.isnan(want["hit_ddg"][n:]).all()
        assert_variant_hits_equal(_hits(engine, c, k, dev=dev, **kw), want)
    assert short


@pytest.mark.parametrize("m", [2, 4, 8, 16, 32, 64, 128, 256])
def test_hits_workgroup_cap_and_a_full_lds_image_at_every_width(engine, m):
    """V = 8192 / m + 5 items on W = 8192 / m - 1 workgroups: six take a second trip. Split as [5 variants] + [the rest with the
    state], the second call has W at the cap and, at k = m, a merge of W k + k = 8 192 keys: the LDS image exactly full."""
    c = vi.hits_cap_case(m)
    V = len(c["tag"])
    W = LDS_KEYS // m - 1
    assert V == W + 6 and V - 5 > W and W * m + m == LDS_KEYS
    dev = torch.from_numpy(c["ddg"]).cuda()
    last = set(c["tag"][V - 6:].tolist())
    for k in sorted({m, m // 2 + 1} if m >= 4 else {m}):
        assert _pow2(k) == m
        want = vi.hits_ref(c, k)
        assert set(want["hit_tag"][:min(k, 6)].tolist()) <= last and int(want["hit_count"][0]) == k
        fresh = _hits(engine, c, k, dev=dev)
        assert_variant_hits_equal(fresh, want)
        first = _hits(engine, c, k, sl=slice(0, 5), dev=dev)
        assert_variant_hits_equal(first, vi.hits_ref(c, k, sl=slice(0, 5)))
        both = _hits(engine, c, k, sl=slice(5, V), state=first["state"], dev=dev)
        assert_variant_hits_equal(both, want)


# ---- pair map ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pmap_crafted():
    """{(L, ld): the 37 variants} on rounding tables with the epistasis specials. Left unchanged by the tests that share it."""
    return vi.pmap_crafted()


def _pmap(engine, c, rows, R, sl=slice(None), state=None, dev=None, **kw):
    ddg, wt = dev if dev is not None else (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    return engine.pair_map(ddg[sl], c["S_var"][sl], c["base"][sl], rows[sl], c["letter"][sl], wt, R, skip=None if kw.get("no_skip") else c["skip"][sl],
                           include_cys=kw.get("include_cys", False), upper=kw.get("upper", False), state=state)


def _pmap_cut(engine, c, rows, R, cut, dev, **kw):
    state, v0 = None, 0
    for n in cut:
        state = _pmap(engine, c, rows, R, sl=slice(v0, v0 + n), state=state, dev=dev, **kw)
        v0 += n
    assert v0 == len(rows)
    return state


def test_pair_map_rounding_tables_every_flag_length_stride_and_row_layout(engine, pmap_crafted):
    R = vi.PMAP_R
    kinds = set()
    for (L, ld), c in pmap_crafted.items():
        vi.assert_pair_map_order_shows(c, ROWS_A, R)
        vi.assert_pair_map_order_shows(c, ROWS_B, R, upper=True)
        dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
        for rows in (ROWS_A, ROWS_B, ROWS_C):
            for kw in PMAP_FLAGS:
                want = vi.pmap_ref(c, rows, R, **kw)
                assert_pair_map_equal(_pmap(engine, c, rows, R, dev=dev, **kw), want)
        for v, q, b, kind in c["sites"]:                                      # each special e is there, at a live candidate site
            assert 0 <= c["S_var"][v, q] < 20 and b != c["S_var"][v, q] and b != 1 and c["skip"][v] == -1 and 0 <= c["letter"][v] < 20
            with np.errstate(invalid="ignore"):
                e = np.float32(c["ddg"][v, q, b] - c["wt"][q, b])
            eb = int(e.view(np.uint32))
            kinds |= {kind} if {"+inf": eb == 0x7f800000, "-inf": eb == 0xff800000, "inf-inf": bool(np.isnan(e)) and np.isinf(c["wt"][q, b]),
                                "-0.0": eb == 0x80000000, "denormal": 0 < (eb & 0x7fffffff) < 0x00800000, "nan": bool(np.isnan(e)) and eb >> 31 == 1}[kind] else set()
    assert kinds == {"+inf", "-inf", "inf-inf", "-0.0", "denormal", "nan"}


@pytest.mark.parametrize("L,ld", [(19, 21), (70, 20)])
def test_pair_map_any_cut_gives_the_same_bits_on_sums_that_round(engine, pmap_crafted, L, ld):
    """The 37 singles and two coarser cuts: ascending v across calls, on sums whose bits depend on the order."""
    c, R = pmap_crafted[L, ld], vi.PMAP_R
    dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    for rows, kw in ((ROWS_A, dict()), (ROWS_B, dict(include_cys=True, upper=True)), (ROWS_C, dict(no_skip=True))):
        want = vi.pmap_ref(c, rows, R, **kw)
        for cut in ((1,) * 37, (10, 27), (5, 7, 18, 7)):                      # 10, 12, 30 and most of the singles cut inside a run
            assert_pair_map_equal(_pmap_cut(engine, c, rows, R, cut, dev, **kw), want)


@pytest.mark.parametrize("L", [1, 2, 255, 256, 257])
def test_pair_map_short_proteins(engine, L):
    c, rows, R = vi.pmap_short_cases()[L]
    assert ((c["letter"] >= 0) & (c["letter"] < 20)).all() and ((c["S_var"] >= 0) & (c["S_var"] < 20)).all()
    assert c["skip"][0] == 0 and c["skip"][1] == L - 1
    for kw in (dict(), dict(include_cys=True, upper=True)):
        want = vi.pmap_ref(c, rows, R, **kw)
        assert (want["count"][:3] > 0).any() and (want["count"][3] == 0).all()
        assert_pair_map_equal(_pmap(engine, c, rows, R, **kw), want)


def test_pair_map_a_run_of_600_variants_whole_and_cut_inside(engine):
    c, rows, R = vi.pmap_long_run_case()
    share_b, share_v = vi.assert_pair_map_order_shows(c, rows, R)
    dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    want = vi.pmap_ref(c, rows, R)
    assert (want["count"][0] > 600 * 10).all()
    assert_pair_map_equal(_pmap(engine, c, rows, R, dev=dev), want)
    for cut in ((1, 611), (299, 313), (599, 13), (1, 298, 300, 13)):
        assert_pair_map_equal(_pmap_cut(engine, c, rows, R, cut, dev), want)


def test_pair_map_reset_strides_over_a_state_larger_than_one_pass(engine):
    """R = 300 rows of L = 2 048: 614 400 state entries against the 2 048 x 256 = 524 288 that the reset's workgroups cover in one
    pass of their grid-stride loop. One variant (8 tiles), no CONTINUE, sentinel patterns everywhere and a guard row behind."""
    from test_gpu_pair_map import _raw, _sentinel, _state_of
    R, L, one_pass = 300, 2048, 2048 * 256
    assert R * L - one_pass == 90112 and (R * L + 255) // 256 > 2048          # entries that only a second pass reaches exist
    c = vi.pmap_case(1, L, 91, specials=False)
    c["S_var"] = np.random.default_rng(92).integers(-1, 21, size=(1, L)).astype(np.int32)
    c["letter"][:], c["skip"][:] = 4, 17
    rows = np.array([1], np.int32)
    sent = _sentinel(L, R + 1)
    big = _state_of(sent)
    front = {name: big[name][:R] for name in NAMES}                           # [R, L] at the front of buffers of R + 1 rows
    assert _raw(engine, c, rows, front, flags=0, R=R) == 0
    want = vi.pmap_ref(c, rows, R)
    assert_pair_map_equal(front, want)
    assert (want["count"][1] > 0).sum() > 1000
    tail = {name: front[name].reshape(-1)[one_pass:] for name in NAMES}
    assert tail["count"].numel() == 90112
    assert (tail["best"] == -1).all() and (tail["eps_lo"] == -1).all() and (tail["eps_hi"] == -1).all()
    assert (tail["count"] == 0).all() and (tail["eps_abs_sum"].view(torch.int32) == 0).all()
    assert all(big[name][R].cpu().numpy().tobytes() == sent[name][R].tobytes() for name in NAMES)   # the guard row keeps every bit


# ---- beam step --------------------------------------------------------------------------------------------------------------------
def _beam(engine, fx, k, dev=None, **kw):
    ddg = torch.from_numpy(fx["ddg"]).cuda() if dev is None else dev
    return engine.beam_step(ddg, fx["S_var"], fx["score"], fx["muts"], fx["depth"], k, **kw)


@pytest.mark.parametrize("depth", sorted(vi.BEAM_POOL))
def test_beam_on_rounding_sums_at_every_width(engine, depth):
    fx = vi.rounding_beam(depth)
    dev = torch.from_numpy(fx["ddg"]).cuda()
    if depth > 1:
        vi.assert_specials_are_candidates(fx["ddg"], fx["score"], fx["S_var"], fx["planted"], fx["blocked"])
        thin, allowed = vi.sparse_beam(fx)
    for d, k in vi.BEAM_PAIRS:
        if d != depth:
            continue
        for kw in (dict(), dict(include_cys=True)):
            want = vi.beam_ref(fx, k, **kw)
            assert int(want["out_count"][0]) == k and (depth == 1 or want["dropped"] >= (depth if k >= 4 else 1)), (k, want["dropped"])
            if k >= 32:
                share = vi.beam_winners_inexact(fx, want).mean()
                assert share >= 1 / 3, (k, share)
            assert_beam_equal(_beam(engine, fx, k, dev=dev, **kw), want)
        if depth > 1 and k >= 64:                                             # few candidates: every sum shows, the denormal ones too
            want = vi.beam_ref(thin, k, allowed=allowed)
            n = int(want["out_count"][0])
            bits = want["out_score"][:n].view(np.uint32) & 0x7fffffff
            assert ((bits > 0) & (bits < 0x00800000)).any() and (bits == 0).any()
            assert_beam_equal(_beam(engine, thin, k, dev=dev, allowed=allowed), want)


def test_beam_pairs_reach_every_width():
    assert sorted({_pow2(d * k) for d, k in vi.BEAM_PAIRS}) == [2, 4, 8, 16, 32, 64, 128, 256]
    assert {d for d, _ in vi.BEAM_PAIRS} == set(vi.BEAM_POOL)


@pytest.mark.parametrize("k,V,L", [(16, 261, 16), (2, 2053, 104)])
def test_beam_workgroup_cap_at_two_widths(engine, k, V, L):
    """m = 32 with W = 255 and m = 4 with W = 2 047: V = W + 6 items, six workgroups take a second trip, the best children sit in the
    last members. (V distinct single substitutions need L x 20 >= V rows: L = 3 cannot hold them; one block of residues all the same.)"""
    m = _pow2(2 * k)
    W = LDS_KEYS // m - 1
    assert V == W + 6 and (V - 1) // 20 < L <= 256
    fx = vi.beam_cap_case(k, V, L)
    want = vi.beam_ref(fx, k)
    assert int(want["out_count"][0]) == k and int(want["out_parent"][0]) >= V - 6
    if k == 16:
        assert want["dropped"] >= 1 and (want["out_parent"][:k] < 3).any()    # the pool's children follow, by two paths each
    got = _beam(engine, fx, k)
    assert_beam_equal(got, want)
    assert int(got["out_parent"][0]) >= V - 6


def test_beam_on_a_hostile_table(engine):
    fx = vi.hostile_beam()
    assert_table_is_hostile(fx["ddg"].reshape(-1, 21), fx["S_var"].reshape(-1))
    want = vi.beam_ref(fx, 64)
    got = _beam(engine, fx, 64)
    assert_beam_equal(got, want)
    n = int(got["out_count"][0])
    assert n == int(want["out_count"][0]) > 0 and not bool(torch.isnan(got["out_score"][:n]).any())


def test_beam_round_trip_on_rounding_sums(engine):
    """The step's out_S, out_score and out_muts are the next step's beam, on freshly drawn rounding tables; the restatement is fed
    the restatement's own first step."""
    fx = vi.rounding_beam(2, specials=False)                                  # (a -inf score would make every child of its member -inf)
    k = 24
    first, want1 = _beam(engine, fx, k), vi.beam_ref(fx, k)
    assert_beam_equal(first, want1)
    assert int(want1["out_count"][0]) == k
    tables = vi.rounding_table(k, fx["S_var"].shape[1], 71)[0]
    held = want1["out_muts"]
    for r in range(k):                                                        # the pool's triples at the bottom again, three parents each
        for e in sorted(fx["pool"] - set(held[r].tolist())):
            tables[r, e >> 5, e & 31] = -np.abs(tables[r, e >> 5, e & 31]) - np.float32(300)
    nxt = dict(ddg=tables, S_var=want1["out_S"], score=want1["out_score"], muts=want1["out_muts"], depth=3)
    want2 = vi.beam_ref(nxt, 64)
    got2 = engine.beam_step(torch.from_numpy(tables).cuda(), first["out_S"], first["out_score"], first["out_muts"], 3, 64)
    assert_beam_equal(got2, want2)
    assert int(want2["out_count"][0]) == 64 and vi.beam_winners_inexact(nxt, want2).mean() >= 1 / 3
