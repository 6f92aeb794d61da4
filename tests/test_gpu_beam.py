"""The beam step on the device (tmpnn_beam_step, Engine.beam_step) and the multi-mutant search on top of it
(variant_scan.multi_mutant_search, TransferModel.multi_mutant_search, --combine) against the numpy restatement of the contract
(tests/beam_restatement.py). Every comparison is exact: counts, substitutions, parents, score bits, every row of out_S, and padding.
The tables of the step tests are synthetic (beam_restatement.duplicate_fixture, whose conditions tests/test_beam_host.py checks on
the reference alone); only the last three tests run a model."""
import numpy as np
import pytest
import torch

from beam_restatement import OUTPUTS, assert_beam_equal, beam_step_reference, duplicate_fixture

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _ref(fx, k, **kw):
    return beam_step_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], fx["depth"], k, kw.get("allowed"), kw.get("cutoff"),
                               kw.get("include_cys", False))


def _run(engine, fx, k, dev_ddg=None, **kw):
    ddg = torch.from_numpy(fx["ddg"]).cuda() if dev_ddg is None else dev_ddg
    return engine.beam_step(ddg, fx["S_var"], fx["score"], fx["muts"], fx["depth"], k, **kw)


def _same_bits(a, b):
    for name in OUTPUTS:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name     # (the bits: NaN padding compares equal)


@pytest.fixture(scope="module")
def crafted():
    """d = 3, V = 37 members of L = 300 rows: the second block of 256 residues has 44. Left unchanged by the tests that share it."""
    return duplicate_fixture(3, 37, 300, 5)


def test_duplicate_fixture_every_k_flag_cutoff_and_allowed(engine, crafted):
    dev = torch.from_numpy(crafted["ddg"]).cuda()
    on = float(_ref(crafted, 85)["out_score"][10])                        # a sum that a pool child has (the reference's eleventh)
    below = float(np.nextafter(np.float32(on), np.float32(-20)))          # and one ulp under it
    allowed = (np.arange(300) % 3 != 1).astype(np.int32)
    allowed[[e >> 5 for e in crafted["pool"]]] = 1                        # the pool's sites stay open: the duplicates stay
    counts, dropped = set(), 0
    for k in (1, 5, 32, 85):
        for cys in (False, True):
            for cutoff in (None, on, below):
                for al in (None, allowed):
                    kw = dict(cutoff=cutoff, include_cys=cys, allowed=al)
                    got, want = _run(engine, crafted, k, dev_ddg=dev, **kw), _ref(crafted, k, **kw)
                    assert_beam_equal(got, want)
                    counts.add(int(got["out_count"][0]))
                    dropped += want["dropped"]
        again, first = _run(engine, crafted, k, dev_ddg=dev), _run(engine, crafted, k, dev_ddg=dev)
        _same_bits(again, first)
    assert {1, 5, 32, 85} <= counts and min(counts) >= 1 and dropped > 500
    at, under = _ref(crafted, 85, cutoff=on), _ref(crafted, 85, cutoff=below)
    assert int(under["out_count"][0]) < int(at["out_count"][0]) < 85 and float(at["out_score"][int(at["out_count"][0]) - 1]) == on
    full = _run(engine, crafted, 85, dev_ddg=dev, include_cys=True)
    assert not torch.isin(full["out_parent"], torch.tensor([35, 36], device="cuda", dtype=torch.int32)).any()   # the NaN score, the dead member


# depth, V, L, k, pool size: the ends of the limits, each with duplicates present wherever a beam can hold any (at d = 1 the beam is
# the wild type alone and every child has one path)
LIMITS = {"d1_V1_k256": (1, 1, 300, 256, 6), "d8_k32": (8, 37, 40, 32, 9), "d2_k128": (2, 12, 40, 128, 6), "L2048_V3": (2, 3, 2048, 64, 3),
          "L19": (3, 20, 19, 32, 6), "V256_L40": (2, 256, 40, 64, 6)}


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_the_ends_of_the_limits(engine, case):
    d, V, L, k, n_pool = LIMITS[case]
    fx = duplicate_fixture(d, V, L, 7, n_pool=n_pool)
    for kw in (dict(), dict(include_cys=True, cutoff=0.25)):
        got, want = _run(engine, fx, k, **kw), _ref(fx, k, **kw)
        assert_beam_equal(got, want)
        assert d == 1 or want["dropped"] >= d - 1
    n = int(want["out_count"][0])
    if case == "d1_V1_k256":
        assert n == 256 and fx["muts"] is None
        assert_beam_equal(engine.beam_step(torch.from_numpy(fx["ddg"]).cuda(), fx["S_var"], fx["score"], np.zeros((1, 0), np.int32), 1, 256),
                          _ref(fx, 256))
    if case == "d8_k32":
        assert n == 32 and fx["muts"].shape[1] == 7 and (want["out_muts"][0] >= 0).all()
    if case == "L2048_V3":
        rows = want["out_muts"][:n] >> 5
        assert (rows == 2047).any() and (fx["muts"][:, 0] >> 5 == 2047).any() and (want["out_S"][:n, 2047] < 20).all()
    if case == "V256_L40":
        assert 256 > 8192 // 128 - 1                                      # 256 items on 63 workgroups: they loop and carry their leaders
        late = dict(fx, score=np.where(np.arange(V) < 6, fx["score"], -np.arange(V, dtype=np.float32)).astype(np.float32))
        got, want = _run(engine, late, k), _ref(late, k)
        assert_beam_equal(got, want)
        assert int(got["out_parent"][0]) >= V - 3                         # the winners sit in the LAST items


def test_leading_dimensions_and_views(engine):
    fx = duplicate_fixture(3, 20, 19, 9)
    want = _ref(fx, 32)
    dev = torch.from_numpy(fx["ddg"]).cuda()
    assert_beam_equal(_run(engine, fx, 32, dev_ddg=dev[:, :, :20].contiguous()), want)     # ld = 20
    wide = torch.full((20, 19, 24), -50.0, device="cuda")                  # a row stride above 21 is the table's leading dimension
    wide[:, :, :21] = dev
    assert_beam_equal(_run(engine, fx, 32, dev_ddg=wide[:, :, :21]), want)
    odd = torch.full((20, 19, 42), -50.0, device="cuda")                   # a view that is no such table is copied
    odd[:, :, ::2] = dev
    assert_beam_equal(_run(engine, fx, 32, dev_ddg=odd[:, :, ::2]), want)
    from thermompnn_amd._lib import TmpnnError
    for bad in (dict(depth=0), dict(depth=9), dict(k=0), dict(k=86), dict(cutoff=NAN), dict(muts=fx["muts"][:, :1]), dict(muts=None),
                dict(allowed=np.ones(18, np.int32)), dict(score=fx["score"][:5])):
        args = dict(ddg=dev, S_var=fx["S_var"], score=fx["score"], muts=fx["muts"], depth=3, k=8)
        args.update(bad)
        with pytest.raises(TmpnnError):
            engine.beam_step(**args)
    with pytest.raises(TmpnnError, match="device"):
        engine.beam_step(torch.from_numpy(fx["ddg"]), fx["S_var"], fx["score"], fx["muts"], 3, 8)
    with pytest.raises(TmpnnError, match="2048"):
        engine.beam_step(torch.zeros((1, 2049, 21), device="cuda"), np.zeros((1, 2049), np.int32), [0.0], None, 1, 4)


def test_empty_and_short_inputs(engine):
    fx = duplicate_fixture(3, 16, 8, 6)

    def nothing(got, k, L):
        assert int(got["out_count"][0]) == 0 and (got["out_muts"] == -1).all() and (got["out_parent"] == -1).all()
        assert bool(torch.isnan(got["out_score"]).all()) and (got["out_S"] == 20).all() and tuple(got["out_S"].shape) == (k, L)

    dead = dict(fx, muts=np.where(np.arange(2)[None] == 1, -1, fx["muts"]).astype(np.int32))
    got = _run(engine, dead, 7)
    assert_beam_equal(got, _ref(dead, 7))
    nothing(got, 7, 8)
    shut = np.zeros(8, np.int32)
    got = _run(engine, fx, 7, allowed=shut)
    assert_beam_equal(got, _ref(fx, 7, allowed=shut))
    nothing(got, 7, 8)
    nothing(_run(engine, fx, 7, cutoff=-INF), 7, 8)
    empty = dict(ddg=np.zeros((0, 8, 21), np.float32), S_var=np.zeros((0, 8), np.int32), score=np.zeros(0, np.float32),
                 muts=np.zeros((0, 2), np.int32), depth=3)
    got = _run(engine, empty, 7)
    assert_beam_equal(got, _ref(empty, 7))
    nothing(got, 7, 8)
    rows0 = dict(ddg=np.zeros((4, 0, 21), np.float32), S_var=np.zeros((4, 0), np.int32), score=np.zeros(4, np.float32),
                 muts=np.zeros((4, 2), np.int32), depth=3)
    nothing(_run(engine, rows0, 7), 7, 0)
    # fewer distinct sets than k: the pool's 20 triples alone pass the cutoff, by 60 paths
    got, want = _run(engine, fx, 85, cutoff=-8.5), _ref(fx, 85, cutoff=-8.5)
    assert_beam_equal(got, want)
    assert int(got["out_count"][0]) == 20 and want["dropped"] == 40
    assert (got["out_S"][20:] == 20).all() and (got["out_muts"][20:] == -1).all() and bool(torch.isnan(got["out_score"][20:]).all())


def test_padded_beam_round_trip(engine):
    """A step's padded output (20 of 32 rows) is the next step's beam as it is: tables are drawn for all 32 rows, the padded rows are
    dead by their -1 substitutions and all-20 letters, and contribute nothing."""
    fx = duplicate_fixture(3, 16, 8, 6)
    first = _run(engine, fx, 32, cutoff=-8.5)
    assert int(first["out_count"][0]) == 20
    rng = np.random.default_rng(3)
    tables = rng.standard_normal((32, 8, 21)).astype(np.float32)
    tables[20:] = -100.0                                                  # would win every rank if a padded row took part
    held = first["out_muts"].cpu().numpy()
    for r in range(20):                                                   # the pool's quadruples at the bottom: four parents each
        for e in sorted(fx["pool"] - set(held[r].tolist())):
            tables[r, e >> 5, e & 31] = -5.0 - 0.125 * (r % 3)
    nxt = dict(ddg=tables, S_var=first["out_S"].cpu().numpy(), score=first["out_score"].cpu().numpy(), muts=first["out_muts"].cpu().numpy(),
               depth=4)
    got = engine.beam_step(torch.from_numpy(tables).cuda(), first["out_S"], first["out_score"], first["out_muts"], 4, 64)
    want = _ref(nxt, 64)
    assert_beam_equal(got, want)
    n = int(got["out_count"][0])
    assert n == 64 and int(got["out_parent"][:n].max()) < 20 and want["dropped"] == 45
    live = dict(ddg=tables[:20], S_var=nxt["S_var"][:20], score=nxt["score"][:20], muts=nxt["muts"][:20], depth=4)
    assert_beam_equal(got, _ref(live, 64))


# ---- end to end: a model, the front end, the command line --------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from thermompnn_amd.custom_inference import load_model
    return load_model(None, None, 0)


@pytest.fixture()
def masked(tmp_path):
    import masked_backbones as mb
    from thermompnn_amd.pdb_io import alt_parse_PDB
    path = mb.write_layout("msk_L40", tmp_path)
    pdb = alt_parse_PDB(path, "A")
    assert "-" in pdb[0]["seq"] and len(pdb[0]["seq"]) == 40
    return path, pdb


def _subs(h):
    from thermompnn_amd.datasets import ALPHABET
    return tuple((m.position, ALPHABET.index(m.mutation)) for m in h.mutations)


def test_search_equals_a_host_loop_over_variant_tables(model, masked, monkeypatch):
    from thermompnn_amd.variant_scan import sequence_indices
    _, pdb = masked
    seq = pdb[0]["seq"]
    S, score, muts, want = sequence_indices(seq)[None], np.zeros(1, np.float32), None, []
    with torch.no_grad():
        wt = model.variant_tables(pdb, S)[0].cpu().numpy()
        for d in (1, 2, 3):
            tables = model.variant_tables(pdb, S).cpu().numpy()
            ref = beam_step_reference(tables, S, score, muts, d, 16)
            n = int(ref["out_count"][0])
            assert n == 16
            S, score, muts = ref["out_S"][:n].astype(np.int64), ref["out_score"][:n], ref["out_muts"][:n]
            want.append(ref)
    eng = model.engine()
    calls, encode = [], eng.encode
    monkeypatch.setattr(eng, "encode", lambda *a, **kw: (calls.append(1), encode(*a, **kw))[1])
    with torch.no_grad():
        levels = model.multi_mutant_search(pdb, 3, 16)
    assert len(calls) == 1                                                # the encoder ran once for the three rounds
    assert [len(lv) for lv in levels] == [16, 16, 16]
    for d, (hits, ref) in enumerate(zip(levels, want), 1):
        assert [_subs(h) for h in hits] == [tuple((int(e) >> 5, int(e) & 31) for e in row) for row in ref["out_muts"]]
        assert [h.parent for h in hits] == ref["out_parent"].tolist()
        np.testing.assert_array_equal(np.array([h.ddG for h in hits], np.float32).view(np.uint32), ref["out_score"].view(np.uint32))
        for h in hits:
            add = sum(float(wt[q, b]) for q, b in _subs(h))
            assert len(h.mutations) == d and h.ddG_additive == add and h.epistasis == h.ddG - add
            assert all(m.wildtype == seq[m.position] != "-" for m in h.mutations)
            assert [m.position for m in h.mutations] == sorted(m.position for m in h.mutations)


def test_level_two_is_the_smaller_order_of_every_pair(model, masked):
    from thermompnn_amd import variant_scan
    _, pdb = masked
    seq = pdb[0]["seq"]
    wt_idx = variant_scan.sequence_indices(seq)
    sites = [p for p, c in enumerate(seq) if c != "-"][3:17:6]
    assert len(sites) == 3
    with torch.no_grad():
        dm = variant_scan.double_mutant_table(model, pdb, positions=sites)            # [3, 20, L, 20] on the device
        levels = model.multi_mutant_search(pdb, 2, 128, positions=sites)
    assert len(levels[0]) == sum(18 + (wt_idx[p] == 1) for p in sites) < 128           # the whole first level: level 2 is exhaustive
    rows = []
    dm = dm.cpu()
    for i, p in enumerate(sites):
        for j, q in enumerate(sites):
            if j <= i:
                continue
            fwd, back = dm[i, :, q, :], dm[j, :, p, :].t()                              # [a, b]: p:a then q:b, and q:b then p:a
            both = torch.minimum(fwd, back) + 0.0                                       # (-0.0 taken as +0.0)
            ok = torch.ones(20, 20, dtype=torch.bool)
            ok[wt_idx[p]], ok[:, wt_idx[q]], ok[1], ok[:, 1] = False, False, False, False
            for a, b in ok.nonzero().tolist():
                rows.append((float(both[a, b]), ((p, a), (q, b))))
    rows.sort()
    want = rows[:128]
    got = sorted((h.ddG, _subs(h)) for h in levels[1])
    assert len(got) == 128 and got == want                                              # sets and bits
    assert [h.ddG for h in levels[1]] == [v for v, _ in want]                           # order
    made_first = [levels[0][h.parent].mutations[0].position == h.mutations[0].position for h in levels[1]]
    assert any(made_first) and not all(made_first)                                      # both orders of a pair win somewhere


def test_command_line_writes_the_front_ends_list(model, masked, tmp_path):
    from thermompnn_amd import variant_scan
    path, pdb = masked
    with torch.no_grad():
        levels = model.multi_mutant_search(pdb, 3, 16, cutoff=0.0, include_cys=True)
    out, ref = str(tmp_path / "cli.csv"), str(tmp_path / "ref.csv")
    assert variant_scan.main([path, "--chain", "A", "--combine", "3", "--beam", "16", "--cutoff", "0.0", "--include_cys", "--out", out,
                              "--synthetic_weights", "0"]) == 0
    rows = variant_scan.write_multi_hits_csv(ref, levels)
    assert open(out, "rb").read() == open(ref, "rb").read() and open(out).read().count("\n") == rows + 1 and rows > 0
