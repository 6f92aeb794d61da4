"""tmpnn_superpose on the device (Engine.superpose, csrc/tmpnn_superpose.hip) against the numpy restatement
(tests/superpose_restatement.py, held against a second method by tests/test_superpose_host.py), and the superposing front ends on top
(TransferModel.ensemble_table(superpose=True), python -m thermompnn_amd.ensemble_scan --superpose).

The lines, on every shape: n_fit, col_count and status exact; NaNs in the same places with the canonical bits; rmsd, dev and rmsf within
2^-23 |want| + 1e-9 A; R within 1e-11 and t within 1e-11 max(1, max|coordinate|); R R^T = I within 1e-12 and det R = +1; a rerun, every
ensemble alone and another batch order with other member slots: the same bits, float64 included. The kernel computes in float64 and
rounds once, and a float64 error of 1e-13 can flip that rounding: hence one fp32 ulp. The floor covers results that are differences of
nearly equal numbers (identical members); it is 3 000 x the disagreement of two float64 methods on the host and a millionth of the
PDB format's 0.001 A."""
import functools

import numpy as np
import pytest
import torch

from superpose_inputs import SHAPES, bad_descriptors, crafted, drawn_map, long_pair, special, subset
from superpose_restatement import ARRAYS, assert_conditioned, assert_superpose_close, filled, superpose_reference

pytestmark = pytest.mark.gpu
NAMES = [name for name, _ in ARRAYS]
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


@functools.lru_cache(maxsize=None)
def _main():
    """(the crafted batch, a drawn map, the restatement through the identity map and through the drawn one); left unchanged."""
    c = crafted()
    rows = drawn_map(c, np.random.default_rng(31))
    return c, rows, _reference(c, c["rows"]), _reference(c, rows)


def _reference(c, rows, **kw):
    return superpose_reference(c["X"], c["mask"], rows, c["desc"], c["R"], c["T"], c["NM"], c["T_out"], c["max_len"], **kw)


def _raw(c, rows, out=None, desc=None, R=None, E=None):
    """One call of the entry itself on sentinel-filled outputs -> (rc, outputs, status), on the device."""
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import _ptr, _stream
    lib = _lib.load()
    desc = c["desc"] if desc is None else desc
    X, mask = torch.from_numpy(c["X"]).cuda(), torch.from_numpy(c["mask"]).cuda()
    r = None if rows is None or len(rows) == 0 else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 6)).cuda()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in (filled(c) if out is None else out).items()}
    status = torch.full((max(len(desc), 1),), 77, dtype=torch.int32, device="cuda")
    ptr = lambda t: _ptr(t) if t is not None and t.numel() else None
    rc = lib.tmpnn_superpose(ptr(X), ptr(mask), ptr(r), c["R"] if R is None else R, ptr(d), len(desc) if E is None else E, c["T"], c["NM"],
                             c["T_out"], c["max_len"], *[ptr(dev[name]) for name in NAMES], _ptr(status), _stream())
    torch.cuda.synchronize()
    return rc, dev, status


def _words(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b, names=NAMES):
    return all(torch.equal(_words(a[n]), _words(b[n])) for n in names)


def _fit_targets_are_identity(c, got):
    xf, rmsd, dev = got["xform"].cpu().numpy(), got["rmsd"].cpu().numpy(), got["dev"].cpu().numpy()
    n_fit = got["n_fit"].cpu().numpy()
    for (map0, M, L, _, mem0, f) in c["desc"].tolist():
        if M == 0:
            continue
        g = mem0 + f
        assert xf[g].tolist() == IDENTITY and not np.signbit(xf[g]).any()
        block = dev[map0 + f * L:map0 + (f + 1) * L]
        assert (block.view(np.uint32)[~np.isnan(block)] == 0).all() and (~np.isnan(block)).sum() == n_fit[g]
        assert rmsd.view(np.uint32)[g] == (0 if n_fit[g] else 0x7fc00000)


def test_every_shape_in_one_call(engine):
    """(M, L) = (1, 19), (2, 3), (3, 70), (17, 257), (5, 1 025), (0, 5) and (300, 19), fit_to first, last and in between, masked rows and
    non-finite coordinates: through the identity map given as a map and as NULL, and through a map with -1, T, T + 5, INT32_MIN and two
    members on the same rows."""
    c, rows, want_id, want_map = _main()
    assert [tuple(s) for s in SHAPES] == list(zip(c["members"], c["lengths"]))
    print("relative gaps of Horn's matrix:", assert_conditioned(want_id), assert_conditioned(want_map))
    rc, got, status = _raw(c, c["rows"])
    assert rc == 0 and status.tolist() == want_id["status"].tolist() == [0] * 7
    print("identity map, worst ratio to the line:", assert_superpose_close(got, want_id, c["coord"]))
    _fit_targets_are_identity(c, got)
    rc, null, status = _raw(c, None)
    assert rc == 0 and status.tolist() == [0] * 7 and _same_bits(null, got)          # rows NULL = the identity map
    rc, again, _ = _raw(c, c["rows"])
    assert rc == 0 and _same_bits(again, got)                                         # a rerun
    rc, got, status = _raw(c, rows)
    assert rc == 0 and status.tolist() == [0] * 7
    print("drawn map, worst ratio to the line:", assert_superpose_close(got, want_map, c["coord"]))
    _fit_targets_are_identity(c, got)
    n_fit = got["n_fit"].cpu().numpy()
    assert (n_fit < np.repeat(c["lengths"], c["members"])).any() and len(set(n_fit.tolist())) > 5
    d = c["desc"][2]
    xf = got["xform"][d[4]:d[4] + 3]
    assert torch.equal(xf[1], xf[0]) and not torch.equal(xf[2], xf[0])                # members 0 and 1 name the same rows
    res = engine.superpose(torch.from_numpy(c["X"]).cuda(), c["mask"], c["members"], c["lengths"], rows=rows, fit_to=c["fit_to"])
    assert _same_bits(res, got) and res["status"].tolist() == [0] * 7                 # the wrapper makes this very call
    assert res["offsets"].tolist() == np.concatenate([[0], np.cumsum(c["lengths"])]).tolist()


def test_every_ensemble_alone_and_another_batch_order():
    """Every output bit depends on (M, L, the data) only: not on E, NM, the ensemble's place in the call or its member slots."""
    c, rows, _, _ = _main()
    rc, full, _ = _raw(c, rows)
    assert rc == 0
    for which in [[e] for e in range(7)] + [[6, 4, 2, 0, 5, 3, 1]]:
        sub, slots, cols = subset(c, which, mem_gap=3 if len(which) > 1 else 1)
        rc, got, status = _raw(sub, rows)
        assert rc == 0 and status.tolist() == [0] * len(which)
        live = torch.from_numpy(slots >= 0).cuda()
        old = torch.from_numpy(slots[slots >= 0]).cuda()
        for name in ("n_fit", "rmsd", "xform"):
            assert torch.equal(_words(got[name])[live], _words(full[name])[old]), (which, name)
            assert (_words(got[name])[~live] == 0x7fc54321).all(), (which, name)       # slots no ensemble names are left alone
        at = torch.from_numpy(cols).cuda()
        assert torch.equal(got["rmsf"].view(torch.int32), full["rmsf"][at].view(torch.int32)), which
        assert torch.equal(got["col_count"], full["col_count"][at]), which
        for e in which:
            map0, M, L = c["desc"][e][:3].tolist()
            assert torch.equal(got["dev"][map0:map0 + M * L].view(torch.int32), full["dev"][map0:map0 + M * L].view(torch.int32)), which


def test_special_cases():
    """Members with 0, 1, 2 and 3 columns in common with the fit target, a member with no valid row, fit_to = M - 1, exact copies of the
    target (through the map and in rows of their own), a mirror image, three collinear points."""
    s = special()
    want = _reference(s, s["rows"])
    assert_conditioned(want, s["loose"])
    rc, got, status = _raw(s, s["rows"])
    assert rc == 0 and status.tolist() == [0, 0, 0]
    tight_cols = np.arange(s["desc"][2][3])                                           # the collinear ensemble's columns and entries
    tight_entries = np.arange(s["desc"][2][0])                                        # hang on a rotation that is not unique
    print("special cases, worst ratio to the line:",
          assert_superpose_close(got, want, s["coord"], loose=s["loose"], cols=tight_cols, entries=tight_entries))
    _fit_targets_are_identity(s, got)
    n_fit, rmsd = got["n_fit"].cpu().numpy(), got["rmsd"].cpu().numpy()
    assert n_fit.tolist() == [10, 0, 1, 2, 3, 0, 10, 40, 40, 40, 40, 3, 3]
    assert np.isnan(rmsd[[1, 5]]).all() and rmsd[2] <= 1e-9 and rmsd[3] > 1e-6
    assert rmsd[7] <= 1e-9 and rmsd[8] <= 1e-9 and rmsd[9] > 1.0                      # the copies fit; the mirror image does not
    assert rmsd[12] <= 1e-4                                                           # (fp32 storage of coordinates near 40 A)
    assert got["col_count"].cpu().numpy()[-3:].tolist() == [2, 2, 2]
    dev = got["dev"].cpu().numpy()
    assert np.isnan(dev[12:48]).all() and (~np.isnan(dev[48:60])).sum() == 3 and np.isnan(dev[60:72]).all()


def test_the_longest_ensemble():
    c = long_pair()
    want = _reference(c, c["rows"])
    assert_conditioned(want)
    rc, got, status = _raw(c, None)
    assert rc == 0 and status.tolist() == [0]
    print("2 x 8192, worst ratio to the line:", assert_superpose_close(got, want, c["coord"]))
    _fit_targets_are_identity(c, got)
    rc, again, _ = _raw(c, c["rows"])
    assert _same_bits(again, got)


def test_bad_descriptors_write_status_and_nothing_else():
    c, rows, _, _ = _main()
    kinds = bad_descriptors(c)
    assert len(kinds) >= 9
    for kind, (row, null) in kinds.items():
        desc = c["desc"].copy()
        desc[2] = row
        out = filled(c)
        b = dict(c, desc=desc)
        if null:                                                                      # R (the size of dev) beyond T: only the T check refuses
            b["R"] = c["R"] + 8
            out["dev"] = np.concatenate([out["dev"], out["dev"][:8]])
        want = _reference(b, None if null else c["rows"], out=out)
        assert want["status"].tolist() == [0, 0, -1, 0, 0, 0, 0], kind
        rc, got, status = _raw(b, None if null else c["rows"], out=out)
        assert rc == 0 and status.tolist() == want["status"].tolist(), kind
        served = np.setdiff1d(np.arange(c["NM"]), np.arange(3, 6))
        cols = np.setdiff1d(np.arange(c["T_out"]), np.arange(22, 92))
        entries = np.setdiff1d(np.arange(c["R"]), np.arange(int(c["desc"][2][0]), int(c["desc"][2][0]) + 210))
        assert_superpose_close({k: got[k] for k in NAMES}, want, c["coord"], members=served, cols=cols, entries=entries)
        g = {k: v.cpu().numpy() for k, v in got.items()}
        for name, idx in (("n_fit", np.arange(3, 6)), ("rmsd", np.arange(3, 6)), ("rmsf", np.arange(22, 92)), ("col_count", np.arange(22, 92)),
                          ("dev", np.arange(int(c["desc"][2][0]), int(c["desc"][2][0]) + 210))):
            assert (g[name][idx].view(np.uint32) == 0x7fc54321).all(), (kind, name)
        assert (g["xform"][3:6].view(np.uint64) == 0x7fc54321).all(), kind


def test_host_side_errors_and_empty_calls(engine):
    from thermompnn_amd import _lib
    c, rows, _, _ = _main()
    rc, got, status = _raw(c, rows, E=0)                                              # E = 0: a no-op
    assert rc == 0 and status.tolist()[0] == 77 and (got["n_fit"].view(torch.int32) == 0x7fc54321).all()
    rc, _, status = _raw(c, rows, R=-1)
    assert rc == -1 and status[0] == 77
    empty = dict(c, X=np.zeros((0, 4, 3), np.float32), mask=np.zeros(0, np.float32), T=0, R=0, NM=5, T_out=4, max_len=4)
    desc = np.array([(0, 0, 4, 0, 0, 0), (0, 5, 0, 4, 0, 4)], np.int32)               # T = 0: M = 0 and L = 0 pass
    rc, got, status = _raw(empty, None, desc=desc)
    assert rc == 0 and status.tolist() == [0, 0]
    assert got["col_count"].tolist() == [0] * 4 and (got["rmsf"].view(torch.int32) == 0x7fc00000).all()
    assert got["n_fit"].tolist() == [0] * 5 and (got["rmsd"].view(torch.int32) == 0x7fc00000).all()
    assert got["xform"].tolist() == [[float(v) for v in IDENTITY]] * 5
    X = torch.from_numpy(c["X"]).cuda()
    none = engine.superpose(X[:0], c["mask"][:0], [], [])
    assert none["rmsd"].shape == (0,) and none["xform"].shape == (0, 12) and none["status"].numel() == 0
    with pytest.raises(_lib.TmpnnError, match="no CPU path"):
        engine.superpose(torch.from_numpy(c["X"]), c["mask"], c["members"], c["lengths"])
    with pytest.raises(_lib.TmpnnError, match="map entries"):
        engine.superpose(X, c["mask"], c["members"], c["lengths"], rows=rows[:-1])
    with pytest.raises(_lib.TmpnnError, match="rows, the backbone has"):
        engine.superpose(X[:-1], c["mask"][:-1], c["members"], c["lengths"])
    with pytest.raises(_lib.TmpnnError, match="fit_to"):
        engine.superpose(X, c["mask"], c["members"], c["lengths"], fit_to=1)          # the first ensemble has one member
    with pytest.raises(_lib.TmpnnError, match="exceeds 8192"):
        engine.superpose(X, c["mask"], [1], [8193], rows=np.zeros(8193, np.int32))


# ---- end to end: three conformers of unequal length with a known rigid motion, the front end, the command line ----------------------
def _conformers(tmp_path):
    """The three conformers of the aligned end-to-end test (one full; one renumbered from 101 with 3 N-terminal and 2 internal
    residues removed; one with a point substitution at 17), members 1 and 2 rotated and translated as rigid bodies, 0.3 A of noise
    on every atom, three decimals as the files hold them."""
    from superpose_inputs import rotation
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    L, seed = 40, 3
    X0, seq = synthetic_backbone(L, seed)
    rng = np.random.default_rng(seed + 60)
    X = X0[None] + rng.normal(0.0, 0.3, size=(3,) + X0.shape)
    for m, shift in ((1, (25.0, -40.0, 12.5)), (2, (-60.0, 8.0, 33.0))):
        X[m] = X[m] @ rotation(rng).T + np.array(shift)
    X = np.round(X, 3)
    keep = np.array([q for q in range(L) if q not in (0, 1, 2, 10, 25)])
    sub = "A" if seq[17] != "A" else "G"
    seqs = [seq, "".join(seq[q] for q in keep), seq[:17] + sub + seq[18:]]
    coords = [X[0], X[1][keep], X[2]]
    paths = []
    for m in range(3):
        lines = [ln for ln in backbone_pdb_text(coords[m], seqs[m]).split("\n") if ln.startswith("ATOM")]
        if m == 1:
            lines = [ln[:22] + f"{int(ln[22:26]) + 100:4d}" + ln[26:] for ln in lines]
        paths.append(str(tmp_path / f"conf{m}.pdb"))
        with open(paths[-1], "w") as fh:
            fh.write("\n".join(lines + ["TER", "END", ""]))
    return paths, seqs


def test_superposed_front_end_and_command_line(tmp_path, monkeypatch):
    import csv
    from align_restatement import align_map, codes
    from ensemble_restatement import ARRAYS as STAT_ARRAYS
    from thermompnn_amd import ensemble_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.pdb_io import alt_parse_PDB
    model = load_model(None, None, 0)
    paths, seqs = _conformers(tmp_path)
    members = [alt_parse_PDB(p, "A")[0] for p in paths]
    assert [m["seq"] for m in members] == seqs
    with torch.no_grad():
        plain = model.ensemble_table(members, cutoff=-0.1, align=True)
        table = model.ensemble_table(members, cutoff=-0.1, align=True, superpose=True)
        last = model.ensemble_table(members, cutoff=-0.1, align=True, superpose=True, fit_to=2)
    for name in STAT_ARRAYS:                                                          # the ddG statistics: the same bits
        assert torch.equal(getattr(table, name), getattr(plain, name)) and torch.equal(getattr(last, name), getattr(plain, name)), name
    assert plain.rmsd is None and plain.rmsf is None and torch.equal(table.aligned, plain.aligned)
    # the restatement on the parsed coordinates and the same map
    L, lens = 40, [40, 35, 40]
    starts = np.concatenate([[0], np.cumsum(lens)])
    maps = [align_map(codes(seqs[0]), codes(s))[0] for s in seqs]
    rows = np.concatenate([np.where(mp >= 0, mp + starts[m], -1) for m, mp in enumerate(maps)]).astype(np.int32)
    X = np.zeros((115, 4, 3), np.float32)
    for m, e in enumerate(members):
        for k, atom in enumerate(("N", "CA", "C", "O")):
            X[starts[m]:starts[m + 1], k] = np.asarray(e["coords_chain_A"][f"{atom}_chain_A"], np.float64).reshape(-1, 3)
    for fit, got in ((0, table), (2, last)):
        want = superpose_reference(X, np.ones(115, np.float32), rows, [(0, 3, L, 0, 0, fit)], 120, 115, 3, L, L)
        assert_conditioned(want)
        res = dict(n_fit=got.n_fit, rmsd=got.rmsd, xform=got.xform, dev=got.deviation.reshape(-1), rmsf=got.rmsf,
                   col_count=torch.from_numpy(want["col_count"]))
        assert tuple(got.deviation.shape) == (3, L) and tuple(got.xform.shape) == (3, 12) and got.rmsf.is_cuda
        print(f"front end, fit_to={fit}, worst ratio to the line:", assert_superpose_close(res, want, float(np.abs(X).max())))
        assert got.n_fit.tolist() == ([40, 35, 39] if fit == 0 else [39, 34, 39])       # (column 17 is out for the substituted member)
    rmsd = table.rmsd.cpu().numpy()
    assert rmsd[0] == 0 and (rmsd[1:] > 0.2).all() and (rmsd[1:] < 1.0).all()        # 0.3 A of noise per coordinate, the motion undone
    with torch.no_grad():
        hits = model.ensemble_hits(members, 10, cutoff=-0.1, align=True, superpose=True)
        bare = model.ensemble_hits(members, 10, cutoff=-0.1, align=True)
    rmsf = table.rmsf.cpu().numpy()
    assert len(hits) == len(bare) >= 3 and all(np.float32(h.rmsf) == rmsf[h.position] for h in hits) and all(np.isnan(h.rmsf) for h in bare)
    assert [(h.position, h.mutation, h.ddG) for h in hits] == [(h.position, h.mutation, h.ddG) for h in bare]
    # max_rmsd refuses the right member by name before any forward
    far = dict(members[2], name="bent")
    ca = np.asarray(far["coords_chain_A"]["CA_chain_A"], np.float64).reshape(-1, 3).copy()
    ca[20:] = ca[20:] @ np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # the second half turned by 90 degrees
    far["coords_chain_A"] = dict(far["coords_chain_A"], CA_chain_A=ca.tolist())
    calls = []
    forward = Engine.ssm_forward
    monkeypatch.setattr(Engine, "ssm_forward", lambda self, *a, **k: (calls.append(1), forward(self, *a, **k))[1])
    with pytest.raises(ValueError, match=r"member 2 \(bent\) lies \d+\.\d+ A"):
        model.ensemble_table([members[0], members[1], far], align=True, superpose=True, max_rmsd=2.0)
    assert not calls
    with torch.no_grad():
        model.ensemble_table(members, align=True, superpose=True, max_rmsd=2.0)
    assert len(calls) == 1
    with pytest.raises(ValueError, match="belong to superpose=True"):
        model.ensemble_table(members, align=True, max_rmsd=2.0)
    with pytest.raises(ValueError, match="fit_to=3"):
        model.ensemble_table(members, align=True, superpose=True, fit_to=3)
    monkeypatch.undo()
    # the command line: the .npz arrays and the rmsf column; without the flag the layouts of before
    out = str(tmp_path / "stats.npz")
    common = paths + ["--members", "--align", "--chain", "A", "--cutoff", "-0.1", "--synthetic_weights", "0"]
    assert ensemble_scan.main(common + ["--out", out]) == 0
    before = dict(np.load(out))
    assert ensemble_scan.main(common + ["--out", out, "--superpose"]) == 0
    z = dict(np.load(out))
    assert sorted(set(z) - set(before)) == ["deviation", "n_fit", "rmsd", "rmsf", "xform"]
    assert all(np.array_equal(z[k], before[k], equal_nan=z[k].dtype.kind == "f") for k in before)
    for name, ref in (("rmsd", table.rmsd), ("n_fit", table.n_fit), ("xform", table.xform), ("deviation", table.deviation.reshape(-1)),
                      ("rmsf", table.rmsf)):
        assert z[name].dtype == ref.cpu().numpy().dtype and np.array_equal(z[name], ref.cpu().numpy(), equal_nan=True), name
    assert ensemble_scan.main(common + ["--out", out, "--superpose", "--fit_to", "2"]) == 0
    assert np.array_equal(np.load(out)["rmsd"], last.rmsd.cpu().numpy())
    with pytest.raises(ValueError, match=r"member 1 .*above max_rmsd 0\.01"):
        ensemble_scan.main(common + ["--out", out, "--superpose", "--max_rmsd", "0.01"])
    with pytest.raises(SystemExit):
        ensemble_scan.main(common + ["--out", out, "--fit_to", "1"])
    top, top_sup = str(tmp_path / "hits.csv"), str(tmp_path / "hits_sup.csv")
    assert ensemble_scan.main(common + ["--out", top, "--top", "10"]) == 0
    assert ensemble_scan.main(common + ["--out", top_sup, "--top", "10", "--superpose"]) == 0
    a, b = list(csv.reader(open(top))), list(csv.reader(open(top_sup)))
    assert b[0] == a[0] + ["rmsf"] and "rmsf" not in a[0] and [r[:-1] for r in b] == a
    assert [float(r[-1]) for r in b[1:]] == [float(np.float32(h.rmsf)) for h in hits]
