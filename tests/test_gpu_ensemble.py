"""Statistics over conformer ensembles on the device (tmpnn_ensemble_stats, Engine.ensemble_stats) and the front ends on top of them
(TransferModel.ensemble_table / ensemble_hits, python -m thermompnn_amd.ensemble_scan) against the numpy restatement of the contract
(tests/ensemble_restatement.py). Every comparison with the restatement is exact: the bits of the four float arrays and the four int
arrays. The tables of the reduction tests are crafted (tests/ensemble_inputs.py, whose conditions tests/test_ensemble_host.py
asserts); only the end-to-end test runs a model."""
import csv

import numpy as np
import pytest
import torch

from ensemble_inputs import DRAWS, SHAPES, crafted, pack, ulp_cutoff, write_models
from ensemble_restatement import ARRAYS, FLOATS, MAX_LEN, assert_ensemble_equal, ensemble_reference, filled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


@pytest.fixture(scope="module")
def cases():
    """{draw: the crafted batch of E = 5 ensembles}; left unchanged by the tests that share it."""
    return {draw: crafted(draw) for draw in DRAWS}


def _ref(c, **kw):
    return ensemble_reference(c["ddg"], c["S"], c["desc"], c["T_out"], c["max_len"], **kw)


def _run(engine, c, table=None, cutoff=None):
    table = torch.from_numpy(c["ddg"]).cuda() if table is None else table
    return engine.ensemble_stats(table, c["S"], c["members"], c["lengths"], cutoff=cutoff)


def _raw(c, desc, T_out, max_len, out, T=None, cutoff=float("inf")):
    """The C entry itself on caller-made descriptors and prefilled outputs -> (outputs, status) as numpy."""
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import _ptr, _stream
    lib = _lib.load()
    ddg, S = torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["S"]).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32)).cuda()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in out.items()}
    status = torch.full((len(desc),), 77, dtype=torch.int32, device="cuda")
    rc = lib.tmpnn_ensemble_stats(_ptr(ddg), int(ddg.stride(0)), _ptr(S), _ptr(d), len(desc), c["T"] if T is None else T, T_out, max_len,
                                  cutoff, *[_ptr(dev[name]) for name in ARRAYS], _ptr(status), _stream())
    assert rc == 0, lib.tmpnn_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}, status.cpu().numpy()


@pytest.mark.parametrize("draw", DRAWS)
def test_crafted_batch_every_stride_and_cutoff(engine, cases, draw):
    c = cases[draw]
    T = c["T"]
    below_cut, value = ulp_cutoff(c)
    wide = torch.zeros((T, 24), device="cuda")
    wide[:, :21] = torch.from_numpy(c["ddg"]).cuda()
    spaced = torch.zeros((T, 42), device="cuda")
    spaced[:, ::2] = torch.from_numpy(c["ddg"]).cuda()
    tables = {"ld21": torch.from_numpy(c["ddg"]).cuda(), "ld20": torch.from_numpy(np.ascontiguousarray(c["ddg"][:, :20])).cuda(),
              "strided24": wide[:, :21], "every_other": spaced[:, ::2]}
    assert tables["strided24"].stride(0) == 24 and tables["every_other"].stride(1) == 2 and tables["ld20"].stride(0) == 20
    for cutoff in (None, -0.5, below_cut, value):
        want = _ref(c, cutoff=cutoff)
        for name, table in tables.items():
            got = _run(engine, c, table, cutoff)
            assert_ensemble_equal(got, want)
            assert got["status"].tolist() == [0] * len(SHAPES) and got["offsets"].tolist() == [0, 19, 89, 108, 178, 183], name
    at_value, under = _ref(c, cutoff=value), _ref(c, cutoff=below_cut)
    assert (at_value["below"] - under["below"]).sum() >= 1                # the ulp decides at least the entry it was taken from
    # a rerun has identical bits
    first, again = _run(engine, c), _run(engine, c)
    for name in ARRAYS:
        assert torch.equal(first[name].view(torch.int32), again[name].view(torch.int32)), name


@pytest.mark.parametrize("draw", DRAWS)
def test_an_ensemble_alone_equals_its_rows_in_the_batch(engine, cases, draw):
    c = cases[draw]
    batch = _run(engine, c, cutoff=0.25)
    table = torch.from_numpy(c["ddg"]).cuda()
    for (row0, M, L, out0) in c["desc"].tolist():
        alone = engine.ensemble_stats(table[row0:row0 + M * L], c["S"][row0:row0 + M * L], [M], [L], cutoff=0.25)
        assert alone["mean"].shape == (L, 20)
        assert_ensemble_equal(alone, batch, want_rows=slice(out0, out0 + L))
    # ... and in another place of another batch: the order of the ensembles reversed
    shapes = SHAPES[::-1]
    desc, T, T_out, max_len = pack(shapes)
    rows = np.concatenate([np.arange(r0, r0 + M * L) for (r0, M, L, _) in c["desc"].tolist()[::-1]]).astype(np.int64)
    moved = engine.ensemble_stats(table[torch.from_numpy(rows).cuda()], c["S"][rows], [M for M, _ in shapes], [L for _, L in shapes], cutoff=0.25)
    for (_, M, L, out0), (_, _, _, new0) in zip(c["desc"].tolist()[::-1], desc.tolist()):
        assert_ensemble_equal(moved, batch, rows=slice(new0, new0 + L), want_rows=slice(out0, out0 + L))


def test_bad_descriptors_write_status_and_nothing_else(engine, cases):
    c = cases["rounding"]
    T, T_out, max_len = c["T"], c["T_out"], c["max_len"]
    good = _ref(c)
    bad = {"row0 + M L > T": (3, 1, 18), "row0 + M L > T by one row": (3, 0, c["desc"][3, 0] + 1), "out_row0 + L > T_out": (4, 3, T_out - 4),
           "L > max_len": (1, 2, 71), "row0 < 0": (0, 0, -1), "M < 0": (2, 1, -3), "L < 0": (2, 2, -19), "out_row0 < 0": (1, 3, -70),
           "M L beyond 32 bits": (3, 1, 0x7fffffff)}
    for what, (e, col, value) in bad.items():
        desc = c["desc"].copy()
        desc[e, col] = value
        out = filled(T_out, 0x7fc12345 + e)
        want = ensemble_reference(c["ddg"], c["S"], desc, T_out, max_len, out=out)
        assert want["status"][e] == -1 and (np.delete(want["status"], e) == 0).all(), what
        got, status = _raw(c, desc, T_out, max_len, out)
        assert status.tolist() == want["status"].tolist(), what
        assert_ensemble_equal(got, want)                                  # the sentinel rows keep every bit, the neighbours are exact
        _, _, L, out0 = c["desc"][e].tolist()
        assert all((got[name][out0:out0 + L].view(np.uint32) == 0x7fc12345 + e).all() for name in ARRAYS), what
        for k, (_, _, Lk, outk) in enumerate(c["desc"].tolist()):
            if k != e:
                assert_ensemble_equal(got, good, rows=slice(outk, outk + Lk), want_rows=slice(outk, outk + Lk))
    # max_len below every L but the last: four ensembles refused in one call, and a T that cuts the last members off
    got, status = _raw(c, c["desc"], T_out, 5, filled(T_out))
    assert status.tolist() == [-1, -1, -1, -1, 0] and (got["count"][:178].view(np.uint32) == 0xdeadbeef).all() and (got["count"][178:] == 0).all()
    got, status = _raw(c, c["desc"], T_out, max_len, filled(T_out), T=T - 1)
    assert status.tolist() == [0, 0, 0, -1, -1]                            # (the M = 0 ensemble starts at row T, beyond T - 1)


@pytest.mark.parametrize("draw", DRAWS)
def test_long_member_loop_and_longest_protein(engine, draw):
    many = crafted(draw, seed=11, shapes=((256, 3),))                       # M = 256: the loop over the members
    assert_ensemble_equal(_run(engine, many, cutoff=0.0), _ref(many, cutoff=0.0))
    long = crafted(draw, seed=12, shapes=((2, MAX_LEN), (1, 3)))            # L = 8192: 640 workgroups per ensemble, the grid's bound
    got = _run(engine, long)
    assert_ensemble_equal(got, _ref(long))
    assert got["mean"].shape == (MAX_LEN + 3, 20) and (got["count"][MAX_LEN - 1] >= 0).all()


def test_empty_calls_and_refusals(engine, cases):
    from thermompnn_amd._lib import TmpnnError
    c = cases["tie"]
    table = torch.from_numpy(c["ddg"]).cuda()
    none = engine.ensemble_stats(table[:0], c["S"][:0], [], [])
    assert none["mean"].shape == (0, 20) and none["offsets"].tolist() == [0] and none["status"].numel() == 0
    for name, dt in zip(ARRAYS, ["float32"] * 4 + ["int32"] * 4):
        assert none[name].dtype == getattr(torch, dt) and none[name].is_cuda
    empty = engine.ensemble_stats(table[:0], c["S"][:0], [0, 5, 0], [4, 0, 0])        # T = 0: members without rows, rows without members
    assert empty["mean"].shape == (4, 20) and empty["status"].tolist() == [0, 0, 0] and empty["offsets"].tolist() == [0, 4, 4, 4]
    assert (empty["count"] == 0).all() and (empty["lo_member"] == -1).all()
    assert (empty["mean"].view(torch.int32) == 0x7fc00000).all() and (empty["hi"].view(torch.int32) == 0x7fc00000).all()
    for kw, word in ((dict(members=[1, 2], lengths=[19]), "one per ensemble"), (dict(members=[1], lengths=[19]), "rows"),
                     (dict(members=[-1], lengths=[19]), "non-negative"), (dict(cutoff=float("nan")), "NaN"),
                     (dict(members=[0], lengths=[MAX_LEN + 1]), "8192"), (dict(S=c["S"][:-1]), "entries")):
        args = dict(dict(ddg=table, S=c["S"], members=c["members"], lengths=c["lengths"]), **kw)
        with pytest.raises(TmpnnError, match=word):
            engine.ensemble_stats(args.pop("ddg"), args.pop("S"), **args)
    with pytest.raises(TmpnnError, match="device"):
        engine.ensemble_stats(torch.from_numpy(c["ddg"]), c["S"], c["members"], c["lengths"])


# ---- end to end: a model, the front end, the command line --------------------------------------------------------------------
def _host_hits(table, count, seq, k, min_members=None, cutoff=None):
    """A host sort (value, position, letter) of an [L, 20] table: no cysteine, not the residue's own letter, no NaN."""
    alphabet = "ACDEFGHIKLMNPQRSTVWY"
    out = []
    for q, wt in enumerate(seq):
        for b in range(20):
            v = float(table[q, b])
            if wt not in alphabet or alphabet[b] == wt or b == 1 or v != v or (min_members is not None and count[q, b] < min_members):
                continue
            if cutoff is not None and not v <= cutoff:
                continue
            out.append((v + 0.0, q, b))
    return sorted(out)[:k]


def test_front_end_and_command_line_equal_the_restatement_of_separate_tables(tmp_path):
    from thermompnn_amd import ensemble_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.ensemble import RANKS, EnsembleTable, align_members
    from thermompnn_amd.pdb_io import alt_parse_PDB, parse_pdb_models
    from thermompnn_amd.synthetic import backbone_pdb_text
    model = load_model(None, None, 0)
    path = str(tmp_path / "ens.pdb")
    X, seq = write_models(path, drop=(1, 7))                              # three conformers of 40 residues, member 1 lacks an N line
    members = parse_pdb_models(path, "A")
    L, M = 40, 3
    with torch.no_grad():
        separate = [model.ssm_table([m]).cpu().numpy() for m in members]   # three forwards of one protein each
        table = model.ensemble_table(members, cutoff=-0.1)
    assert isinstance(table, EnsembleTable) and table.seq == seq and table.names == ["ens_m1", "ens_m2", "ens_m3"]
    _, S = align_members(members)
    want = ensemble_reference(np.concatenate(separate), S.reshape(-1), [(0, M, L, 0)], L, L, cutoff=-0.1)
    got = {name: getattr(table, name) for name in ARRAYS}
    assert all(v.is_cuda and tuple(v.shape) == (L, 20) for v in got.values())
    assert_ensemble_equal(got, want)                                      # bits: a member's table does not depend on its batch
    count = want["count"]
    assert (count[7] == 2).all() and (np.delete(count, 7, axis=0) == 3).all()
    assert (want["spread"] > 0).sum() > 700 and not np.isnan(want["mean"]).any()
    # hit lists: a host sort of the table each rank names
    hits = {}
    for rank, name in RANKS.items():
        with torch.no_grad():
            hits[rank] = model.ensemble_hits(members, 25, rank=rank, cutoff=-0.1)
        ref = _host_hits(want[name], count, seq, 25, cutoff=-0.1)
        assert len(ref) >= 5, rank
        assert [(h.position, "ACDEFGHIKLMNPQRSTVWY".index(h.mutation)) for h in hits[rank]] == [(q, b) for _, q, b in ref], rank
        for h, (v, q, b) in zip(hits[rank], ref):
            assert h.wildtype == seq[q] and np.float32(h.ddG) == np.float32(v) and h.ddG == getattr(h, name)
            for stat in ARRAYS:
                x = want[stat][q, b]
                assert np.float32(getattr(h, stat)) == x if stat in FLOATS else getattr(h, stat) == int(x), (rank, stat)
    assert {name: RANKS[name] for name in ("mean", "worst", "best")} == dict(mean="mean", worst="hi", best="lo")
    with torch.no_grad():
        every = model.ensemble_hits(members, 256, rank="mean", one_per_position=True)
        full = model.ensemble_hits(members, 256, rank="mean", one_per_position=True, min_members=3)
    assert 7 in [h.position for h in every] and 7 not in [h.position for h in full] and len(full) == len(every) - 1
    ref = _host_hits(want["mean"], count, seq, 10, min_members=3)
    with torch.no_grad():
        got_hits = model.ensemble_hits(members, 10, min_members=3)
    assert [(h.position, "ACDEFGHIKLMNPQRSTVWY".index(h.mutation)) for h in got_hits] == [(q, b) for _, q, b in ref]
    with pytest.raises(ValueError, match="rank"):
        model.ensemble_hits(members, 5, rank="median")
    # the command line: the same arrays in the .npz, the same hits in the CSV
    out = str(tmp_path / "stats.npz")
    assert ensemble_scan.main([path, "--chain", "A", "--out", out, "--cutoff", "-0.1", "--synthetic_weights", "0"]) == 0
    z = np.load(out)
    assert_ensemble_equal({name: z[name] for name in ARRAYS}, want)
    assert z["offsets"].tolist() == [0, L] and z["seqs"].tolist() == [seq] and z["names"].tolist() == ["ens"] and z["members"].tolist() == [3]
    assert z["member_names"].tolist() == table.names
    hits_csv = str(tmp_path / "hits.csv")
    assert ensemble_scan.main([path, "--chain", "A", "--out", hits_csv, "--top", "25", "--rank", "worst", "--cutoff", "-0.1",
                               "--synthetic_weights", "0"]) == 0
    rows = list(csv.reader(open(hits_csv)))
    assert rows[0] == [""] + ensemble_scan.HIT_COLUMNS + list(ARRAYS) and len(rows) == 1 + len(hits["worst"])
    for r, (row, h) in enumerate(zip(rows[1:], hits["worst"])):
        assert row[:2] == [str(r), "ThermoMPNN"] and row[3:9] == [repr(h.ddG), str(h.position), h.wildtype, h.mutation, str(r), "ens"]
        assert row[9:] == [repr(h.mean), repr(h.spread), repr(h.lo), repr(h.hi), str(h.lo_member), str(h.hi_member), str(h.count), str(h.below)]
    table_csv = str(tmp_path / "stats.csv")
    assert ensemble_scan.main([path, "--chain", "A", "--out", table_csv, "--cutoff", "-0.1", "--synthetic_weights", "0"]) == 0
    rows = list(csv.reader(open(table_csv)))
    assert rows[0] == [""] + ensemble_scan.TABLE_COLUMNS and len(rows) == 1 + L * 19
    q, b = 7, 0 if seq[7] != "A" else 2
    line = next(r for r in rows[1:] if r[4] == "7" and r[6] == "ACDEFGHIKLMNPQRSTVWY"[b])
    assert line[3] == "ens" and line[5] == seq[7] and line[7] == repr(float(want["mean"][q, b])) and line[13] == "2"
    # --members on three single files (the ensemble cut between forwards, too) equals the multi-MODEL run
    singles = []
    for m in range(M):
        lines = [ln for ln in backbone_pdb_text(X[m], seq).split("\n")
                 if not (m == 1 and ln.startswith("ATOM") and ln[12:16] == " N  " and int(ln[22:26]) == 8)]
        singles.append(str(tmp_path / f"conf{m}.pdb"))
        with open(singles[-1], "w") as fh:
            fh.write("\n".join(lines))
    for atom, xyz in alt_parse_PDB(singles[1], "A")[0]["coords_chain_A"].items():
        np.testing.assert_array_equal(np.array(xyz), np.array(members[1]["coords_chain_A"][atom]))      # (NaN at the missing N)
    for extra in ([], ["--chunk_residues", "50"]):
        out2 = str(tmp_path / "stats2.npz")
        assert ensemble_scan.main(singles + ["--members", "--chain", "A", "--out", out2, "--cutoff", "-0.1", "--synthetic_weights", "0"] + extra) == 0
        z2 = np.load(out2)
        assert_ensemble_equal({name: z2[name] for name in ARRAYS}, want)
        assert z2["members"].tolist() == [3] and z2["member_names"].tolist() == ["conf0", "conf1", "conf2"] and z2["names"].tolist() == ["conf0"]
    # without --members the three files are three ensembles of one: spread 0, every extreme the mean
    assert ensemble_scan.main(singles + ["--chain", "A", "--out", out2, "--synthetic_weights", "0"]) == 0
    z3 = np.load(out2)
    assert z3["offsets"].tolist() == [0, 40, 80, 120] and z3["members"].tolist() == [1, 1, 1]
    for m in range(M):
        np.testing.assert_array_equal(z3["mean"][40 * m:40 * m + 40].view(np.uint32)[S[m] < 20], separate[m][:, :20].view(np.uint32)[S[m] < 20])
    assert (z3["spread"][z3["count"] > 0] == 0).all() and (z3["count"][47] == 0).all() and np.isnan(z3["mean"][47]).all()
