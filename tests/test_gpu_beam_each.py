"""The beam step for many proteins on the device (tmpnn_beam_step_each, Engine.beam_step_each) and the packed search on top of it
(variant_scan.multi_mutant_search_each, TransferModel.multi_mutant_search_each, combine_scan) against the numpy restatement of the
contract (tests/beam_each_restatement.py) and against the single-protein step on each protein's slice. Every comparison is exact:
counts, substitutions, parents, score bits, every column of out_S, and padding. The tables of the step tests are synthetic
(beam_each_restatement.pack_fixture, whose conditions tests/test_beam_each_host.py checks on the reference alone); only the last test
runs a model."""
import os

import numpy as np
import pytest
import torch

from beam_each_restatement import assert_beam_each_equal, beam_step_each_reference, pack_fixture, reorder_pack
from beam_restatement import OUTPUTS

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIXED = (19, 300, 0, 40, 257)


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _ref(fx, k, **kw):
    return beam_step_each_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], fx["offsets"], fx["depth"], k, **kw)


def _run(engine, fx, k, dev_ddg=None, **kw):
    ddg = torch.from_numpy(fx["ddg"]).cuda() if dev_ddg is None else dev_ddg
    return engine.beam_step_each(ddg, fx["S_var"], fx["score"], fx["muts"], fx["offsets"], fx["depth"], k, **kw)


def _part(res, p, offsets):
    """Protein p's part of a packed result, on the device, in the layout of one ``beam_step``."""
    o, e = int(offsets[p]), int(offsets[p + 1])
    return dict(out_muts=res["out_muts"][p], out_score=res["out_score"][p], out_parent=res["out_parent"][p], out_S=res["out_S"][:, o:e],
                out_count=res["out_count"][p:p + 1])


def _same_bits(a, b):
    for name in OUTPUTS:
        assert a[name].shape == b[name].shape, name
        assert torch.equal(a[name].contiguous().view(torch.int32), b[name].contiguous().view(torch.int32)), name   # (the bits: NaN padding too)


def _single(engine, fx, p, k, allowed=None, **kw):
    """Engine.beam_step on protein p's slice."""
    o, e = int(fx["offsets"][p]), int(fx["offsets"][p + 1])
    ddg = torch.from_numpy(np.ascontiguousarray(fx["ddg"][:, o:e])).cuda()
    return engine.beam_step(ddg, np.ascontiguousarray(fx["S_var"][:, o:e]), fx["score"][p], None if fx["muts"] is None else fx["muts"][p],
                            fx["depth"], k, allowed=None if allowed is None else allowed[o:e], **kw)


def _check(engine, fx, k, singles=True, **kw):
    """The packed step against the restatement and, protein by protein, against the single step's bits. -> (result, reference)."""
    got, want = _run(engine, fx, k, **kw), _ref(fx, k, **{key: val for key, val in kw.items() if key != "dev_ddg"})
    assert_beam_each_equal(got, want, fx["offsets"])
    if singles:
        own = {key: val for key, val in kw.items() if key not in ("dev_ddg", "max_len")}
        for p in range(len(fx["offsets"]) - 1):
            _same_bits(_part(got, p, fx["offsets"]), _single(engine, fx, p, k, **own))
    return got, want


@pytest.fixture(scope="module")
def mixed():
    """d = 3, V = 37, five proteins of 19, 300, 0, 40 and 257 rows. Left unchanged by the tests that share it."""
    return pack_fixture(3, 37, MIXED, 5)


def test_mixed_pack_every_k_flag_cutoff_and_allowed(engine, mixed):
    dev = torch.from_numpy(mixed["ddg"]).cuda()
    on = float(_ref(mixed, 85)["out_score"][1, 10])                       # a sum that a pool child of protein 1 has
    below = float(np.nextafter(np.float32(on), np.float32(-20)))          # and one ulp under it
    T = int(mixed["offsets"][-1])
    allowed = (np.arange(T) % 3 != 1).astype(np.int32)
    for p, part in enumerate(mixed["parts"]):
        if part is not None:
            allowed[[int(mixed["offsets"][p]) + (e >> 5) for e in part["pool"]]] = 1        # the pools' sites stay open: the duplicates stay
    counts, dropped = set(), 0
    for k in (1, 5, 32, 85):
        for cys in (False, True):
            for cutoff in (None, on, below):
                for al in (None, allowed):
                    got, want = _check(engine, mixed, k, dev_ddg=dev, cutoff=cutoff, include_cys=cys, allowed=al)
                    counts.update(got["out_count"].tolist())
                    dropped += sum(want["dropped"])
    assert {0, 1, 5, 32, 85} <= counts and min(counts) == 0 and dropped > 2000
    at, under = _ref(mixed, 85, cutoff=on), _ref(mixed, 85, cutoff=below)
    assert int(under["out_count"][1]) < int(at["out_count"][1]) < 85 and float(at["out_score"][1, int(at["out_count"][1]) - 1]) == on
    full = _run(engine, mixed, 85, dev_ddg=dev, include_cys=True)
    assert not torch.isin(full["out_parent"], torch.tensor([35, 36], device="cuda", dtype=torch.int32)).any()   # the NaN scores, the dead members
    assert int(full["out_count"][2]) == 0


def test_placement_in_the_pack_and_reruns_change_no_bit(engine, mixed):
    base = _run(engine, mixed, 32)
    _same_bits(base, _run(engine, mixed, 32))                              # a rerun
    rev = reorder_pack(mixed, [4, 3, 2, 1, 0])
    got = _check(engine, rev, 32, singles=False)[0]
    for j, p in enumerate([4, 3, 2, 1, 0]):
        _same_bits(_part(got, j, rev["offsets"]), _part(base, p, mixed["offsets"]))
    twice = reorder_pack(mixed, [1, 4, 0, 3, 2, 0, 4, 1, 2, 3])
    got = _check(engine, twice, 32, singles=False)[0]
    for j, p in enumerate([1, 4, 0, 3, 2, 0, 4, 1, 2, 3]):
        _same_bits(_part(got, j, twice["offsets"]), _part(base, p, mixed["offsets"]))
    for p in range(5):                                                    # each alone: P = 1
        alone = reorder_pack(mixed, [p])
        _same_bits(_part(_run(engine, alone, 32), 0, alone["offsets"]), _part(base, p, mixed["offsets"]))
    # max_len above the longest protein changes W's bound and the grid, and no bit
    _same_bits(base, _run(engine, mixed, 32, max_len=2048))


# depth, V, lens, k, pool size
LIMITS = {"L19_L2048": (2, 3, (19, 2048), 64, 3), "d8_k32": (8, 37, (40, 23), 32, 9), "d1_V1_k256": (1, 1, (300, 19, 0), 256, 6),
          "d2_k128": (2, 12, (40, 33), 128, 6), "V256_L40": (2, 256, (40, 40, 40), 64, 6), "P300": (2, 32, tuple(8 + (7 * i) % 17 for i in range(300)), 64, 6)}


@pytest.mark.parametrize("case", sorted(LIMITS))
def test_the_ends_of_the_limits(engine, case):
    d, V, lens, k, n_pool = LIMITS[case]
    fx = pack_fixture(d, V, lens, 7, n_pool=n_pool)
    many = case == "P300"
    for kw in (dict(), dict(include_cys=True, cutoff=0.25)):
        got, want = _check(engine, fx, k, singles=not many, **kw)
        assert d == 1 or all(n >= d - 1 for n, L in zip(want["dropped"], lens) if L > 0)
    n = want["out_count"]
    if case == "L19_L2048":
        rows = want["out_muts"][1, :n[1]] >> 5
        assert (rows == 2047).any() and (fx["muts"][1, :, 0] >> 5 == 2047).any() and (want["out_S"][:n[1], 19 + 2047] < 20).all()
    if case == "d1_V1_k256":
        assert n[0] == 256 and 0 < n[1] <= 256 and n[2] == 0 and fx["muts"] is None
        again = engine.beam_step_each(torch.from_numpy(fx["ddg"]).cuda(), fx["S_var"], fx["score"], np.zeros((3, 1, 0), np.int32), fx["offsets"], 1, 256)
        _same_bits(again, _run(engine, fx, 256))
    if case == "d8_k32":
        assert n.tolist() == [32, 32] and fx["muts"].shape == (2, 37, 7) and (want["out_muts"][:, 0] >= 0).all()
    if case == "V256_L40":
        assert 256 > 8192 // 128 - 1                                      # 256 items on 63 workgroups per protein: they loop and carry their leaders
        late = dict(fx, score=np.where(np.arange(V) < 6, fx["score"], -np.arange(V, dtype=np.float32)).astype(np.float32))
        got = _check(engine, late, k)[0]
        assert int(got["out_parent"][:, 0].min()) >= V - 3                # the winners sit in the LAST items of every protein
    if many:
        assert 300 * 32 > 8192 and min(lens) == 8 and max(lens) == 24 and (n == 64).all()       # more slots than the grid holds: it loops
        for p in (0, 1, 150, 298, 299):
            _same_bits(_part(got, p, fx["offsets"]), _single(engine, fx, p, k, include_cys=True, cutoff=0.25))


def test_leading_dimensions_and_views(engine):
    fx = pack_fixture(3, 20, (19, 40, 23), 9)
    want = _ref(fx, 32)
    dev = torch.from_numpy(fx["ddg"]).cuda()
    assert_beam_each_equal(_run(engine, fx, 32, dev_ddg=dev[:, :, :20].contiguous()), want, fx["offsets"])      # ld = 20
    wide = torch.full((20, 82, 24), -50.0, device="cuda")                  # a row stride above 21 is the table's leading dimension
    wide[:, :, :21] = dev
    assert_beam_each_equal(_run(engine, fx, 32, dev_ddg=wide[:, :, :21]), want, fx["offsets"])
    odd = torch.full((20, 82, 42), -50.0, device="cuda")                   # a view that is no such table is copied
    odd[:, :, ::2] = dev
    assert_beam_each_equal(_run(engine, fx, 32, dev_ddg=odd[:, :, ::2]), want, fx["offsets"])
    on_dev = engine.beam_step_each(dev, fx["S_var"], fx["score"], fx["muts"], torch.from_numpy(fx["offsets"]).cuda(), 3, 32, max_len=40)
    assert_beam_each_equal(on_dev, want, fx["offsets"])                    # offsets that are on the device already
    from thermompnn_amd._lib import TmpnnError
    for bad in (dict(depth=0), dict(depth=9), dict(k=0), dict(k=86), dict(cutoff=NAN), dict(muts=fx["muts"][:, :, :1]), dict(muts=fx["muts"][:2]),
                dict(muts=None), dict(allowed=np.ones(81, np.int32)), dict(score=fx["score"][:2]), dict(score=fx["score"][:, :5]),
                dict(max_len=2049), dict(offsets=torch.from_numpy(fx["offsets"]).cuda()), dict(S_var=fx["S_var"][:, :81])):
        args = dict(ddg=dev, S_var=fx["S_var"], score=fx["score"], muts=fx["muts"], offsets=fx["offsets"], depth=3, k=8)
        args.update(bad)
        with pytest.raises(TmpnnError):
            engine.beam_step_each(**args)
    with pytest.raises(TmpnnError, match="device"):
        engine.beam_step_each(torch.from_numpy(fx["ddg"]), fx["S_var"], fx["score"], fx["muts"], fx["offsets"], 3, 8)


def test_dead_proteins_and_a_padded_beam_stepped_again(engine):
    fx = pack_fixture(3, 16, (8, 12, 8), 6)
    dead = dict(fx, muts=fx["muts"].copy())
    dead["muts"][1, :, 1] = -1                                            # every member of the protein in the middle is dead
    got, want = _check(engine, dead, 7)
    assert got["out_count"].tolist() == [7, 0, 7] and (got["out_S"][:, 8:20] == 20).all() and (got["out_muts"][1] == -1).all()
    assert bool(torch.isnan(got["out_score"][1]).all()) and (got["out_parent"][1] == -1).all()
    # fewer distinct sets than k: the pools' 20 triples alone pass the cutoff, by 60 paths each protein
    first, want = _check(engine, fx, 32, cutoff=-8.5)
    assert first["out_count"].tolist() == [20, 20, 20] and want["dropped"] == [40, 40, 40]
    assert (first["out_S"][20:] == 20).all() and (first["out_muts"][:, 20:] == -1).all() and bool(torch.isnan(first["out_score"][:, 20:]).all())
    # the padded result (20 of 32 rows per protein) is the next step's beam as it stands
    rng = np.random.default_rng(3)
    tables = rng.standard_normal((32, 28, 21)).astype(np.float32)
    tables[20:] = -100.0                                                  # would win every rank if a padded row took part
    held = first["out_muts"].cpu().numpy()
    for p, part in enumerate(fx["parts"]):
        for r in range(20):                                               # the pools' quadruples at the bottom: four parents each
            for e in sorted(part["pool"] - set(held[p, r].tolist())):
                tables[r, int(fx["offsets"][p]) + (e >> 5), e & 31] = -5.0 - 0.125 * ((r + p) % 3)
    nxt = dict(ddg=tables, S_var=first["out_S"].cpu().numpy(), score=first["out_score"].cpu().numpy(), muts=held, depth=4, offsets=fx["offsets"])
    got = engine.beam_step_each(torch.from_numpy(tables).cuda(), first["out_S"], first["out_score"], first["out_muts"], fx["offsets"], 4, 64)
    want = _ref(nxt, 64)
    assert_beam_each_equal(got, want, fx["offsets"])
    assert got["out_count"].tolist() == [64, 64, 64] and int(got["out_parent"].max()) < 20 and min(want["dropped"]) >= 3
    for p in range(3):
        _same_bits(_part(got, p, fx["offsets"]), _single(engine, nxt, p, 64))


def test_the_device_refuses_bad_ranges_and_serves_their_neighbours(engine):
    """Through the C entry, with every output filled with a sentinel first."""
    from thermompnn_amd.engine import _ptr, _stream
    fx = pack_fixture(3, 20, (19, 40, 19), 11)
    T, k, d, SENT = 78, 8, 3, -7
    dev = {name: torch.from_numpy(fx[name]).cuda() for name in ("ddg", "S_var", "score", "muts")}
    lib = engine.lib
    for offsets, max_len, bad in (([-1, 19, 59, 78], 40, [0]), ([0, 19, 59, 79], 40, [2]), ([0, 19, 59, 78], 39, [1]), ([0, 19, 59, 40], 40, [2]),
                                  ([0, 19, 59, 78], 40, []), ([5, 5, 2 ** 31 - 1, 78], 2048, [1, 2]), ([-2 ** 31, 0, 19, 2 ** 31 - 1], 2048, [0, 2])):
        off = torch.tensor(offsets, dtype=torch.int32, device="cuda")
        out = dict(out_muts=torch.full((3, k, d), SENT, dtype=torch.int32, device="cuda"), out_score=torch.full((3, k), 7.0, device="cuda"),
                   out_parent=torch.full((3, k), SENT, dtype=torch.int32, device="cuda"), out_S=torch.full((k, T), SENT, dtype=torch.int32, device="cuda"),
                   out_count=torch.full((3,), SENT, dtype=torch.int32, device="cuda"))
        ws = torch.empty(lib.tmpnn_beam_step_each_workspace_bytes(3, 20, max_len, k, d), dtype=torch.uint8, device="cuda")
        rc = lib.tmpnn_beam_step_each(_ptr(dev["ddg"]), 21, _ptr(dev["S_var"]), _ptr(dev["score"]), _ptr(dev["muts"]), d, None, _ptr(off), 3, T, 20,
                                      max_len, k, INF, 0, _ptr(out["out_muts"]), _ptr(out["out_score"]), _ptr(out["out_parent"]),
                                      _ptr(out["out_S"]), _ptr(out["out_count"]), _ptr(ws), ws.numel(), _stream())
        assert rc == 0, lib.tmpnn_last_error()
        torch.cuda.synchronize()
        want = beam_step_each_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], offsets, d, k, max_len=max_len, fill=SENT)
        assert [p for p in range(3) if not want["good"][p]] == bad
        assert out["out_count"].tolist() == want["out_count"].tolist() and [p for p in range(3) if out["out_count"][p] == -1] == bad
        assert_beam_each_equal(out, want, offsets)                         # padding for the bad; every bit of the good: no bad range is written
        claimed_good = np.zeros(T, bool)
        for p in range(3):
            if want["good"][p]:
                claimed_good[offsets[p]:offsets[p + 1]] = True
        assert (out["out_S"].cpu().numpy()[:, ~claimed_good] == SENT).all()


def test_more_proteins_than_the_grid_holds(engine):
    """P = 8 200 proteins of one or two rows, d = 1, V = 1, k = 4: all three grids are capped at 8 192 workgroups, so the merge's
    protein loop (one workgroup per protein) runs a second time for the last eight, as do the other two launches' slot loops."""
    rng = np.random.default_rng(17)
    P, k = 8200, 4
    lens = 1 + (np.arange(P) % 7 == 3)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(offsets[-1])
    fx = dict(ddg=rng.standard_normal((1, T, 21)).astype(np.float32), S_var=rng.integers(0, 21, size=(1, T)).astype(np.int32),
              score=rng.standard_normal((P, 1)).astype(np.float32), muts=None, depth=1, offsets=offsets)
    assert P > 8192 and P * k > 8192
    got, want = _check(engine, fx, k, singles=False, include_cys=True)
    assert (want["out_count"][8192:] == k).any() and (want["out_count"] == 0).any()          # letter 20: a protein without a residue
    for p in (0, 3, 8191, 8192, 8195, 8199):                             # on either side of the grid's edge
        _same_bits(_part(got, p, offsets), _single(engine, fx, p, k, include_cys=True))


def test_empty_sizes(engine):
    k = 7

    def nothing(got, P, T):
        assert tuple(got["out_S"].shape) == (k, T) and (got["out_S"] == 20).all() and got["out_count"].tolist() == [0] * P
        assert (got["out_muts"] == -1).all() and (got["out_parent"] == -1).all() and bool(torch.isnan(got["out_score"]).all())
        assert tuple(got["out_muts"].shape) == (P, k, 3) and tuple(got["out_score"].shape) == (P, k) == tuple(got["out_parent"].shape)

    none = engine.beam_step_each(torch.zeros((4, 30, 21), device="cuda"), np.zeros((4, 30), np.int32), np.zeros((0, 4), np.float32),
                                 np.zeros((0, 4, 2), np.int32), [0], 3, k)
    nothing(none, 0, 30)                                                  # P = 0: nothing to do, out_S as allocated
    v0 = engine.beam_step_each(torch.zeros((0, 30, 21), device="cuda"), np.zeros((0, 30), np.int32), np.zeros((2, 0), np.float32),
                               np.zeros((2, 0, 2), np.int32), [0, 10, 30], 3, k)
    nothing(v0, 2, 30)                                                    # V = 0
    t0 = engine.beam_step_each(torch.zeros((4, 0, 21), device="cuda"), np.zeros((4, 0), np.int32), np.zeros((3, 4), np.float32),
                               np.zeros((3, 4, 2), np.int32), [0, 0, 0, 0], 3, k)
    nothing(t0, 3, 0)                                                     # T = 0
    fx = pack_fixture(3, 16, (0, 8, 0), 6)                                 # proteins without a row beside one that has some
    got = _check(engine, fx, k)[0]
    assert got["out_count"].tolist() == [0, 7, 0]
    shut = np.zeros(8, np.int32)
    nothing(_run(engine, fx, k, allowed=shut), 3, 8)
    nothing(_run(engine, fx, k, cutoff=-INF), 3, 8)


def test_c_entry_errors_before_any_launch(engine):
    from test_beam_each_host import cabi_errors_and_sizer_zeros
    cabi_errors_and_sizer_zeros(engine.lib)


# ---- end to end: a model, the front end, the command line --------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from thermompnn_amd.custom_inference import load_model
    return load_model(None, None, 0)


@pytest.fixture(scope="module")
def structures(tmp_path_factory):
    """The masked 40-residue protein of test_gpu_beam.py, 2OCJ chain A with its gap, 2OCJ chain A, a short synthetic backbone."""
    import masked_backbones as mb
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    tmp = tmp_path_factory.mktemp("each")
    X, seq = synthetic_backbone(14, 5)
    short = tmp / "short14.pdb"
    short.write_text(backbone_pdb_text(X, seq))
    paths = [mb.write_layout("msk_L40", tmp), os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"), os.path.join(GOLDEN, "2OCJ.pdb"), str(short)]
    pdbs = [alt_parse_PDB(p, "A") for p in paths]
    assert "-" in pdbs[0][0]["seq"] and len(pdbs[0][0]["seq"]) == 40 and "-" in pdbs[1][0]["seq"] and len(pdbs[3][0]["seq"]) == 14
    return paths, pdbs


def _flat(levels):
    return [[(tuple((m.position, m.wildtype, m.mutation, m.ddG, m.pdb) for m in h.mutations), np.float32(h.ddG).view(np.uint32).item(), h.ddG,
              h.ddG_additive, h.epistasis, h.parent) for h in lv] for lv in levels]


def test_packed_search_equals_the_single_search_on_every_structure(model, structures, monkeypatch, tmp_path):
    from thermompnn_amd import combine_scan, variant_scan
    paths, pdbs = structures
    entries = [p[0] for p in pdbs]
    wt = [variant_scan.sequence_indices(e["seq"]) for e in entries]
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in wt])])
    with torch.no_grad():
        enc = model._encode_structures(entries)
        packed = model._tables_over(enc, np.concatenate(wt)[None])[0]
        for p, pdb in enumerate(pdbs):                                    # the forward's batch independence: the pack's tables are each protein's own
            own = model.variant_tables(pdb, wt[p][None])[0]
            assert torch.equal(packed[offsets[p]:offsets[p + 1]].view(torch.int32), own.view(torch.int32)), p
        single = [model.multi_mutant_search(pdb, 3, 8) for pdb in pdbs]
        eng = model.engine()
        calls, encode = [], eng.encode
        monkeypatch.setattr(eng, "encode", lambda *a, **kw: (calls.append(1), encode(*a, **kw))[1])
        got = model.multi_mutant_search_each(pdbs, 3, 8)
        assert len(calls) == 1                                            # one encoder run for the pack of four
        two = model.multi_mutant_search_each(pdbs, 3, 8, pack_residues=len(wt[0]) + len(wt[1]))
        assert len(calls) == 3                                            # ... and one per pack of two
    assert [[len(lv) for lv in levels] for levels in got] == [[8, 8, 8]] * 4
    for p in range(4):
        assert _flat(got[p]) == _flat(single[p]) == _flat(two[p]), p      # sets, parents, score bits, additive sums, names
    out = str(tmp_path / "each.csv")
    argv = ["--chain", "A", "--combine", "3", "--beam", "8", "--synthetic_weights", "0"]
    assert combine_scan.main(paths + argv + ["--out", out]) == 0
    lines, at = open(out).read().split("\n"), 1
    assert lines[0] == "pdb,order,rank,mutations,ddG,ddG_additive,epistasis" and lines[-1] == ""
    for n, path in enumerate(paths):
        one = str(tmp_path / f"one{n}.csv")
        assert variant_scan.main([path] + argv + ["--out", one]) == 0
        rows = open(one).read().split("\n")[1:-1]
        name = os.path.splitext(os.path.basename(path))[0]
        assert len(rows) == 24 and lines[at:at + 24] == [name + "," + r for r in rows], path
        at += 24
    assert at == len(lines) - 1
