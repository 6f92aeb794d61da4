"""Ensemble statistics through a row map on the device (tmpnn_ensemble_stats_rows, Engine.ensemble_stats(rows=)) against the numpy
restatement (tests/align_restatement.py, held against ensemble_restatement by tests/test_align_host.py), and the aligned front ends on
top (TransferModel.ensemble_table(align=True), python -m thermompnn_amd.ensemble_scan --align). Every comparison is exact."""
import numpy as np
import pytest
import torch

from align_inputs import draw_rows
from align_restatement import align_map, codes, ensemble_rows_reference
from ensemble_inputs import DRAWS, SHAPES, crafted
from ensemble_restatement import ARRAYS, assert_ensemble_equal, filled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


@pytest.fixture(scope="module")
def cases():
    """{draw: (the crafted batch, a drawn row map, its restatement)}; left unchanged by the tests that share it."""
    out = {}
    for draw in DRAWS:
        c = crafted(draw)
        rows = draw_rows(c, np.random.default_rng(31))
        out[draw] = (c, rows, ensemble_rows_reference(c["ddg"], c["S"], rows, c["desc"], c["T_out"], c["max_len"], cutoff=-0.5))
    return out


@pytest.mark.parametrize("draw", DRAWS)
def test_drawn_row_map_every_stride(engine, cases, draw):
    c, rows, want = cases[draw]
    T = c["T"]
    assert (rows == -1).any() and (rows == T).any() and (rows == -2 ** 31).any() and len(set(rows[(rows >= 0) & (rows < T)].tolist())) < T
    wide = torch.zeros((T, 24), device="cuda")
    wide[:, :21] = torch.from_numpy(c["ddg"]).cuda()
    tables = {"ld21": torch.from_numpy(c["ddg"]).cuda(), "ld20": torch.from_numpy(np.ascontiguousarray(c["ddg"][:, :20])).cuda(),
              "strided24": wide[:, :21]}
    assert tables["strided24"].stride(0) == 24 and tables["ld20"].stride(0) == 20
    for name, table in tables.items():
        got = engine.ensemble_stats(table, c["S"], c["members"], c["lengths"], cutoff=-0.5, rows=rows)
        assert_ensemble_equal(got, want)
        assert got["status"].tolist() == want["status"].tolist() == [0] * len(SHAPES), name
    again = engine.ensemble_stats(tables["ld21"], c["S"], c["members"], c["lengths"], cutoff=-0.5, rows=torch.from_numpy(rows).cuda())
    for name in ARRAYS:
        assert torch.equal(got[name].view(torch.int32), again[name].view(torch.int32)), name


@pytest.mark.parametrize("draw", DRAWS)
def test_identity_rows_equal_the_plain_entry(engine, cases, draw):
    c = cases[draw][0]
    table = torch.from_numpy(c["ddg"]).cuda()
    plain = engine.ensemble_stats(table, c["S"], c["members"], c["lengths"], cutoff=0.25)
    mapped = engine.ensemble_stats(table, c["S"], c["members"], c["lengths"], cutoff=0.25, rows=np.arange(c["T"], dtype=np.int32))
    for name in ARRAYS + ("status", "offsets"):
        assert torch.equal(plain[name].view(torch.int32), mapped[name].view(torch.int32)), name


def _raw(c, rows, desc, T_out, max_len, out, R=None):
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import _ptr, _stream
    lib = _lib.load()
    ddg, S = torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["S"]).cuda()
    r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32)).cuda()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in out.items()}
    status = torch.full((max(len(desc), 1),), 77, dtype=torch.int32, device="cuda")
    rc = lib.tmpnn_ensemble_stats_rows(_ptr(ddg), int(ddg.stride(0)), _ptr(S), _ptr(r) if len(rows) else None, len(rows) if R is None else R,
                                       _ptr(d), len(desc), c["T"], T_out, max_len, float("inf"), *[_ptr(dev[name]) for name in ARRAYS],
                                       _ptr(status), _stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in dev.items()}, status.cpu().numpy()


def test_map_range_failures_and_empty_calls(engine, cases):
    c, rows, _ = cases["rounding"]
    T_out, max_len = c["T_out"], c["max_len"]
    good = ensemble_rows_reference(c["ddg"], c["S"], rows, c["desc"], T_out, max_len)
    # map0 + M L > R: the map cut one entry short refuses the last ensemble with members, (17, 70), and the empty one behind it
    out = filled(T_out, 0x7fc54321)
    R = len(rows) - 1
    want = ensemble_rows_reference(c["ddg"], c["S"], rows[:R], c["desc"], T_out, max_len, out=out)
    assert want["status"].tolist() == [0, 0, 0, -1, -1]
    rc, got, status = _raw(c, rows, c["desc"], T_out, max_len, out, R=R)
    assert rc == 0 and status.tolist() == [0, 0, 0, -1, -1]
    assert_ensemble_equal(got, want)
    assert all((got[name][108:].view(np.uint32) == 0x7fc54321).all() for name in ARRAYS)
    assert_ensemble_equal(got, good, rows=slice(0, 108), want_rows=slice(0, 108))
    desc = c["desc"].copy()
    desc[1, 0] = len(rows) - 2 * 70 + 1                                              # one ensemble's map0 + M L > R by one
    want = ensemble_rows_reference(c["ddg"], c["S"], rows, desc, T_out, max_len, out=out)
    rc, got, status = _raw(c, rows, desc, T_out, max_len, out)
    assert rc == 0 and status.tolist() == want["status"].tolist() == [0, -1, 0, 0, 0]
    assert_ensemble_equal(got, want)
    # host-side refusals, and the empty calls
    from thermompnn_amd import _lib
    rc, _, status = _raw(c, rows, c["desc"], T_out, max_len, out, R=-1)
    assert rc == -1 and status[0] == 77
    rc, _, status = _raw(c, rows[:0], c["desc"], T_out, max_len, out, R=5)           # rows NULL with R > 0
    assert rc == -1 and status[0] == 77
    rc, got, status = _raw(c, rows[:0], np.array([(0, 0, 4, 0), (0, 3, 0, 4)]), T_out, max_len, out)     # R = 0: M = 0 and L = 0 pass
    assert rc == 0 and status.tolist() == [0, 0] and (got["count"][:4] == 0).all() and (got["count"][4:].view(np.uint32) == 0x7fc54321).all()
    rc, got, status = _raw(c, rows, np.zeros((0, 4), np.int32), T_out, max_len, out)                     # E = 0: a no-op
    assert rc == 0 and status.tolist() == [77] and (got["count"].view(np.uint32) == 0x7fc54321).all()
    table = torch.from_numpy(c["ddg"]).cuda()
    none = engine.ensemble_stats(table, c["S"], [], [], rows=np.zeros(0, np.int32))
    assert none["mean"].shape == (0, 20) and none["status"].numel() == 0
    empty = engine.ensemble_stats(table, c["S"], [0, 5], [4, 0], rows=np.zeros(0, np.int32))
    assert empty["status"].tolist() == [0, 0] and (empty["count"] == 0).all() and (empty["mean"].view(torch.int32) == 0x7fc00000).all()
    with pytest.raises(_lib.TmpnnError, match="map entries"):
        engine.ensemble_stats(table, c["S"], c["members"], c["lengths"], rows=rows[:-1])


# ---- end to end: members of unequal length, the front end, the command line ---------------------------------------------------
def _conformers(tmp_path):
    """Three conformers of the 40-residue synthetic backbone as three files, from ensemble_inputs.write_models' ingredients: one full;
    one renumbered from 101, with 3 N-terminal and 2 internal residues (10, 25) removed; one with a point substitution at 17."""
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    L, seed = 40, 3
    X0, seq = synthetic_backbone(L, seed)
    rng = np.random.default_rng(seed + 50)
    X = np.round(X0[None] + rng.normal(0.0, 0.25, size=(3,) + X0.shape), 3)
    keep = np.array([q for q in range(L) if q not in (0, 1, 2, 10, 25)])
    sub = "A" if seq[17] != "A" else "G"
    seqs = [seq, "".join(seq[q] for q in keep), seq[:17] + sub + seq[18:]]
    coords = [X[0], X[1][keep], X[2]]
    paths = []
    for m in range(3):
        lines = [ln for ln in backbone_pdb_text(coords[m], seqs[m]).split("\n") if ln.startswith("ATOM")]
        if m == 1:                                                                   # renumbered: residue k of the file is 101 + k
            lines = [ln[:22] + f"{int(ln[22:26]) + 100:4d}" + ln[26:] for ln in lines]
        paths.append(str(tmp_path / f"conf{m}.pdb"))
        with open(paths[-1], "w") as fh:
            fh.write("\n".join(lines + ["TER", "END", ""]))
    return paths, seqs, keep


def test_aligned_front_end_and_command_line(tmp_path):
    from thermompnn_amd import ensemble_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.ensemble import EnsembleTable
    from thermompnn_amd.pdb_io import alt_parse_PDB
    model = load_model(None, None, 0)
    paths, seqs, keep = _conformers(tmp_path)
    members = [alt_parse_PDB(p, "A")[0] for p in paths]
    assert [m["seq"] for m in members] == seqs and [len(s) for s in seqs] == [40, 35, 40]
    with pytest.raises(ValueError, match="alignment is out of scope"):               # align=False: the parent's refusal, unchanged
        model.ensemble_table(members)
    with torch.no_grad():
        separate = [model.ssm_table([m]).cpu().numpy() for m in members]
        table = model.ensemble_table(members, cutoff=-0.1, align=True)
    assert isinstance(table, EnsembleTable) and table.seq == seqs[0]
    L, lens = 40, [40, 35, 40]
    starts = np.concatenate([[0], np.cumsum(lens)])
    maps = [align_map(codes(seqs[0]), codes(s)) for s in seqs]
    rows = np.concatenate([np.where(mp >= 0, mp + starts[m], -1) for m, (mp, _) in enumerate(maps)]).astype(np.int32)
    S = np.concatenate([codes(s) for s in seqs])
    want = ensemble_rows_reference(np.concatenate(separate), S, rows, [(0, 3, L, 0)], L, L, cutoff=-0.1)
    got = {name: getattr(table, name) for name in ARRAYS}
    assert all(v.is_cuda and tuple(v.shape) == (L, 20) for v in got.values())
    assert_ensemble_equal(got, want)                                                 # bits: maps and statistics
    count = want["count"]
    for q in (0, 1, 2, 10, 25, 17):
        assert (count[q] == 2).all(), q                                              # the deleted and the substituted columns
    assert (np.delete(count, [0, 1, 2, 10, 25, 17], axis=0) == 3).all()
    np.testing.assert_array_equal(table.aligned.cpu().numpy(), np.stack([mp for mp, _ in maps]).astype(np.int32))
    assert table.aligned[1].cpu().numpy()[keep].tolist() == list(range(35))
    np.testing.assert_allclose(table.identity.cpu().numpy(), [1.0, 1.0, 39 / 40])
    # a longer reference: the extra columns have no participants
    ref = "MK" + seqs[0] + "HHH"
    with torch.no_grad():
        longer = model.ensemble_table(members, cutoff=-0.1, align=True, reference=ref)
    assert longer.seq == ref and tuple(longer.count.shape) == (45, 20)
    cnt = longer.count.cpu().numpy()
    assert (cnt[:2] == 0).all() and (cnt[42:] == 0).all() and (cnt[2:42] == count).all()
    assert_ensemble_equal({name: getattr(longer, name)[2:42] for name in ARRAYS}, want)
    fasta = str(tmp_path / "ref.fasta")
    with open(fasta, "w") as fh:
        fh.write(">ref some words\n" + ref[:30] + "\n" + ref[30:] + "\n")
    # unrelated proteins are refused, not scattered along the axis
    rng = np.random.default_rng(4)
    perm = rng.permutation(40)
    shuffled = dict(members[2])
    shuffled["seq"] = "".join(seqs[2][q] for q in perm)
    shuffled["seq_chain_A"] = shuffled["seq"]
    with pytest.raises(ValueError, match=r"member 2 .*identity 0\.\d+"):
        model.ensemble_table([members[0], members[1], shuffled], align=True)
    with torch.no_grad():
        model.ensemble_table([members[0], members[1], shuffled], align=True, min_identity=0.0)
        hits = model.ensemble_hits(members, 10, cutoff=-0.1, align=True)
    assert len(hits) >= 3 and all(h.count in (2, 3) for h in hits)
    # the command line
    out = str(tmp_path / "stats.npz")
    assert ensemble_scan.main(paths + ["--members", "--align", "--chain", "A", "--out", out, "--cutoff", "-0.1", "--synthetic_weights", "0"]) == 0
    z = np.load(out)
    assert_ensemble_equal({name: z[name] for name in ARRAYS}, want)
    np.testing.assert_array_equal(z["aligned"].reshape(3, L), np.stack([mp for mp, _ in maps]).astype(np.int32))
    np.testing.assert_allclose(z["identity"], [1.0, 1.0, 39 / 40])
    assert ensemble_scan.main(paths + ["--members", "--align", "--reference", fasta, "--chain", "A", "--out", out, "--cutoff", "-0.1",
                                       "--synthetic_weights", "0"]) == 0
    z = np.load(out)
    assert z["seqs"].tolist() == [ref] and (z["count"][:2] == 0).all() and z["aligned"].shape == (3 * 45,)
    with pytest.raises(ValueError, match="alignment is out of scope"):
        ensemble_scan.main(paths + ["--members", "--chain", "A", "--out", out, "--synthetic_weights", "0"])
