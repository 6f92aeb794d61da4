"""The beam step for many proteins and the search on top of it, the parts that need no GPU: the conditions that the packed fixture of
tests/test_gpu_beam_each.py has to meet, checked on the numpy restatement alone (they are what keeps a kernel that reads the wrong
protein's rows, or takes a position word for a packed row, from passing), the front end's packs and rounds through stub table and step
functions against ``multi_mutant_search`` per protein, its errors, combine_scan's CSV, and the build's view of the file."""
import ctypes as C

import numpy as np
import pytest
import torch

from beam_each_restatement import beam_step_each_reference, pack_fixture, protein_outputs, reorder_pack
from beam_restatement import assert_beam_equal, beam_step_reference
from test_beam_host import StubStep
from test_pair_hits_host import SEQ, stub_tables

NAN, INF = float("nan"), float("inf")
MIXED = (19, 300, 0, 40, 257)                                             # the GPU test's pack: d = 3, V = 37


def _ref(fx, k, **kw):
    return beam_step_each_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], fx["offsets"], fx["depth"], k, **kw)


def _differs(a, b):
    return any(not np.array_equal(a[name], b[name], equal_nan=True) for name in ("out_muts", "out_score", "out_parent", "out_S"))


def test_packed_fixture_meets_its_conditions_on_the_reference_alone():
    fx = pack_fixture(3, 37, MIXED, 5)
    assert fx["offsets"].tolist() == [0, 19, 319, 319, 359, 616] and fx["ddg"].shape == (37, 616, 21) and fx["muts"].shape == (5, 37, 2)
    for k in (5, 32, 85):
        ref = _ref(fx, k)
        assert ref["good"] == [True] * 5 and ref["out_count"].tolist() == [k, k, 0, k, k]
        assert all(ref["dropped"][p] >= 2 for p in (0, 1, 3, 4)), ref["dropped"]           # every non-empty protein drops >= d - 1
        for p in range(5):                                                                   # the loop is beam_step on the slices
            part = fx["parts"][p]
            if part is not None:
                assert_beam_equal(protein_outputs(ref, p, fx["offsets"]),
                                  beam_step_reference(part["ddg"], part["S_var"], part["score"], part["muts"], 3, k))
    ref = _ref(fx, 1)
    assert ref["out_count"].tolist() == [1, 1, 0, 1, 1]
    assert (ref["out_S"][:, 319:319].size == 0) and (ref["out_muts"][2] == -1).all() and np.isnan(ref["out_score"][2]).all()
    # a kernel that reads another protein's score row or muts row cannot pass: either swap changes the outputs of both proteins
    base = _ref(fx, 32)
    for name in ("score", "muts"):
        for a, b in ((0, 1), (1, 3), (3, 4)):
            swapped = dict(fx, **{name: fx[name].copy()})
            swapped[name][[a, b]] = fx[name][[b, a]]
            other = _ref(swapped, 32)
            for p in (a, b):
                assert _differs(protein_outputs(base, p, fx["offsets"]), protein_outputs(other, p, fx["offsets"])), (name, a, b, p)
    # a position word is local: members of every later protein mutate its LAST row, and so do kept children
    for p in (1, 3, 4):
        last = MIXED[p] - 1
        assert (fx["muts"][p] >> 5 == last).any() and int(fx["offsets"][p]) > 0            # (its packed row is another)
        n = int(base["out_count"][p])
        assert (base["out_muts"][p, :n] >> 5 == last).any() and (base["out_muts"][p, :n] >> 5 < MIXED[p]).all()
    # the same proteins elsewhere in a pack: the restatement is placement-free by construction
    rev = reorder_pack(fx, [4, 3, 2, 1, 0])
    got = _ref(rev, 32)
    for j, p in enumerate([4, 3, 2, 1, 0]):
        assert_beam_equal(protein_outputs(got, j, rev["offsets"]), protein_outputs(base, p, fx["offsets"]))


def test_range_check_of_the_restatement():
    fx = pack_fixture(3, 20, (19, 40, 19), 11)
    T = 78
    good = _ref(fx, 8, fill=-7)
    assert good["out_count"].tolist() == [8, 8, 8] and (good["out_S"] != -7).all()
    for offsets, max_len, bad in (([-1, 19, 59, 78], 40, [0]), ([0, 19, 59, 79], 40, [2]), ([0, 19, 59, 78], 39, [1]),
                                  ([0, 19, 59, 40], 40, [2])):
        ref = beam_step_each_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], offsets, 3, 8, max_len=max_len, fill=-7)
        assert [p for p in range(3) if not ref["good"][p]] == bad and [p for p in range(3) if ref["out_count"][p] == -1] == bad
        for p in bad:
            assert (ref["out_muts"][p] == -1).all() and (ref["out_parent"][p] == -1).all() and np.isnan(ref["out_score"][p]).all()
        claimed = np.zeros(T, bool)
        for p in range(3):
            if ref["good"][p]:
                claimed[offsets[p]:offsets[p + 1]] = True
        assert (ref["out_S"][:, ~claimed] == -7).all() and (ref["out_S"][:, claimed] != -7).all()


# ---- the front end on stub tables ------------------------------------------------------------------------------------------------
def stub_tables_each(S, offsets):
    """``stub_tables`` protein by protein: a protein's table depends on its own rows alone, as the forward's does."""
    S = np.asarray(S)
    return torch.cat([stub_tables(S[:, int(o):int(e)]) for o, e in zip(offsets[:-1], offsets[1:])], dim=1)


class StubStepEach:
    """Engine.beam_step_each on the host: the restatement, round by round."""
    def __init__(self):
        self.calls = []

    def __call__(self, ddg, S_var, score, muts, offsets, depth, k, allowed=None, cutoff=None, include_cys=False, max_len=None):
        self.calls.append((int(ddg.shape[0]), len(offsets) - 1, depth))
        r = beam_step_each_reference(ddg.numpy(), np.asarray(S_var), np.asarray(score), None if muts is None else np.asarray(muts), offsets,
                                     depth, k, allowed, cutoff, include_cys, max_len)
        return {key: torch.from_numpy(np.asarray(r[key])) for key in ("out_muts", "out_score", "out_parent", "out_S", "out_count")}


SEQS = [SEQ, "ACDEFGHIKLMNPQRSTVWY", "GG-WKX", "MKTAYIAKQRQISFVKSHFSRQ", "W"]


def test_front_end_equals_the_single_search_per_protein():
    from thermompnn_amd.variant_scan import multi_mutant_search, multi_mutant_search_each
    pdbs = [[{"seq": s, "name": f"p{i}"}] for i, s in enumerate(SEQS)]
    # structure 2 may mutate one site only: its beam dies at level 2 while the others go on
    cases = (dict(), dict(include_cys=True, cutoff=-1.0), dict(positions=[[0, 4, 11], None, [3], [21, 0, 7], None], cutoff=0.5))
    for kw in cases:
        for order, beam in ((1, 7), (3, 5), (4, 40)):
            single = []
            for i, pdb in enumerate(pdbs):
                own = dict(kw, positions=kw["positions"][i]) if "positions" in kw else kw
                single.append(multi_mutant_search(None, pdb, order, beam, _tables=stub_tables, _step=StubStep(), **own))
            for pack_residues, packs in ((10 ** 6, 1), (30, 3), (1, 5)):
                step, tables_calls = StubStepEach(), []
                tables = lambda S, o: (tables_calls.append(len(o) - 1), stub_tables_each(S, o))[1]
                got = multi_mutant_search_each(None, pdbs, order, beam, pack_residues=pack_residues, _tables=tables, _step=step, **kw)
                assert got == single                                      # every field of every hit of every level of every structure
                assert len(got) == 5 and all(len(levels) == order for levels in got)
                assert len(step.calls) == len(tables_calls) <= order * packs              # one decode and one step per round and pack
                assert sum(1 for c in step.calls if c[2] == 1) == packs and all(c[0] == (1 if c[2] == 1 else beam) for c in step.calls)
                assert sorted(set(tables_calls)) == {1: [5], 3: [1, 2], 5: [1]}[packs]
    assert all(m.pdb == "p3" for lv in got[3] for h in lv for m in h.mutations)
    levels = got[2]
    assert len(levels[0]) > 0 and levels[1:] == [[], [], []] and len(got[1][3]) > 0         # it died at level 2; structure 1 went on
    assert multi_mutant_search_each(None, [], 2, 4, _tables=stub_tables_each, _step=StubStepEach()) == []
    gone = multi_mutant_search_each(None, pdbs, 3, 8, cutoff=-100.0, _tables=stub_tables_each, _step=StubStepEach())
    assert gone == [[[], [], []]] * 5


def test_front_end_errors_name_the_structure():
    from thermompnn_amd.variant_scan import multi_mutant_search_each
    pdbs = [[{"seq": SEQ, "name": "first"}], {"seq": "ACDEFGHIKL", "name": "second"}]
    run = lambda **kw: multi_mutant_search_each(None, kw.pop("pdbs", pdbs), _tables=stub_tables_each, _step=StubStepEach(), **kw)
    for bad, word in ((dict(order=0, beam=4), "order=0"), (dict(order=9, beam=4), "order=9"), (dict(order=2, beam=0), "beam=0"),
                      (dict(order=2, beam=129), "beam=129"), (dict(order=1, beam=257), "beam=257"),
                      (dict(order=2, beam=4, positions=[[3], None]), r"structure 0 \(first\): position 3"),
                      (dict(order=2, beam=4, positions=[None, [10]]), r"structure 1 \(second\): position 10"),
                      (dict(order=2, beam=4, positions=[None, [-1]]), r"structure 1 \(second\): position -1"),
                      (dict(order=2, beam=4, positions=[[0]]), "1 lists for 2 structures"),
                      (dict(order=2, beam=4, pack_residues=0), "pack_residues=0"),
                      (dict(order=2, beam=4, pdbs=pdbs + [{"seq": "A" * 2049, "name": "long"}]), r"structure 2 \(long\): 2049 residues exceed 2048")):
        with pytest.raises(ValueError, match=word):
            run(**bad)
    assert len(run(order=2, beam=4, positions=[[0], [9]])) == 2


def test_combine_scan_writes_the_single_scans_rows_behind_a_pdb_column(tmp_path, capsys):
    from thermompnn_amd import combine_scan, variant_scan
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    paths = []
    for n, (L, seed) in enumerate(((14, 5), (9, 2), (23, 7))):
        X, seq = synthetic_backbone(L, seed)
        path = tmp_path / f"s{n}.pdb"
        path.write_text(backbone_pdb_text(X, seq))
        paths.append(str(path))
    out = tmp_path / "each.csv"
    opts = ["--chain", "A", "--combine", "3", "--beam", "6", "--cutoff", "0.5", "--include_cys"]
    assert combine_scan.main(paths + opts + ["--out", str(out), "--pack_residues", "25"], _tables=stub_tables_each, _step=StubStepEach()) == 0
    assert "substitutions of 3 structures" in capsys.readouterr().out
    lines = out.read_text().split("\n")
    assert lines[0] == "pdb,order,rank,mutations,ddG,ddG_additive,epistasis" and lines[-1] == ""
    body, at = lines[1:-1], 0
    assert [ln.split(",")[0] for ln in body] == sorted(ln.split(",")[0] for ln in body)    # argument order: s0, s1, s2
    for n, path in enumerate(paths):
        one = tmp_path / f"one{n}.csv"
        assert variant_scan.main([path] + opts + ["--out", str(one)], _tables=stub_tables, _step=StubStep()) == 0
        rows = one.read_text().split("\n")[1:-1]
        assert len(rows) > 0 and body[at:at + len(rows)] == [f"s{n}," + r for r in rows]
        alone = tmp_path / f"alone{n}.csv"                               # one file: byte for byte behind the first column
        assert combine_scan.main([path] + opts + ["--out", str(alone)], _tables=stub_tables_each, _step=StubStepEach()) == 0
        assert alone.read_bytes() == ("pdb," + one.read_text().split("\n")[0] + "\n" + "".join(f"s{n},{r}\n" for r in rows)).encode()
        at += len(rows)
    assert at == len(body)
    capsys.readouterr()
    for bad, word in ((["--combine", "0", "--beam", "4"], "combine"), (["--combine", "9", "--beam", "4"], "combine"),
                      (["--combine", "3", "--beam", "86"], "beam"), (["--combine", "3"], "--beam"),
                      (["--combine", "3", "--beam", "4", "--pack_residues", "0"], "pack_residues")):
        with pytest.raises(SystemExit):
            combine_scan.main(paths + ["--out", str(out)] + bad, _tables=stub_tables_each, _step=StubStepEach())
        assert word in capsys.readouterr().err, bad


# ---- the build and the C entries, before any launch ------------------------------------------------------------------------------
def cabi_errors_and_sizer_zeros(lib):
    """The host-side error codes and the sizer of tmpnn_beam_step_each: every call fails before a launch, no pointer is dereferenced."""
    size = lib.tmpnn_beam_step_each_workspace_bytes
    assert size(4, 10, 100, 0, 2) == 0 and size(4, 10, 100, 8, 0) == 0 and size(4, 10, 100, 8, 9) == 0 and size(-1, 10, 100, 8, 2) == 0
    assert size(4, 10, 100, 257, 1) == 0 and size(4, 10, 100, 129, 2) == 0 and size(4, 10, 100, 33, 8) == 0 and size(4, 10, 100, 86, 3) == 0
    assert size(4, -1, 100, 8, 2) == 0 and size(4, 10, -1, 8, 2) == 0 and size(4, 10, 2049, 8, 2) == 0 and size(4, 65537, 10, 8, 2) == 0
    assert size(4, 10, 100, 256, 1) > 0 and size(4, 10, 100, 32, 8) > 0 and size(1, 65536, 2048, 8, 2) > 0 and size(0, 10, 100, 8, 2) > 0
    # P slots of W k d keys and k words: W = min(V ceil(max_len / 256), 8192 / m - 1)
    assert size(3, 10, 100, 8, 2) >= 3 * (10 * 16 * 8 + 8 * 4) and size(64, 64, 256, 64, 4) >= 64 * (31 * 256 * 8 + 64 * 4)
    assert size(2, 256, 40, 64, 2) >= 2 * 63 * 128 * 8 and size(300, 8, 24, 4, 2) >= 300 * 8 * 8 * 8
    assert size(5, 0, 100, 8, 2) > 0 and size(5, 10, 0, 8, 2) > 0
    d = C.c_void_p(256)                                                   # never dereferenced

    def call(ddg=d, ld=21, S=d, score=d, muts=d, depth=3, allowed=None, offsets=d, P=3, T=300, V=4, max_len=100, k=8, cutoff=INF, flags=0,
             o1=d, o2=d, o3=d, o4=d, o5=d, ws=d, nbytes=1 << 24):
        return lib.tmpnn_beam_step_each(ddg, ld, S, score, muts, depth, allowed, offsets, P, T, V, max_len, k, cutoff, flags, o1, o2, o3, o4,
                                        o5, ws, nbytes, None)

    for name in ("ddg", "S", "score", "muts", "offsets", "o1", "o2", "o3", "o4", "o5", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(k=0) == -1 and b"k=0" in lib.tmpnn_last_error() and call(k=-3) == -1
    assert call(depth=0) == -1 and b"depth=0" in lib.tmpnn_last_error() and call(depth=9) == -1 and b"depth=9" in lib.tmpnn_last_error()
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    for name in ("P", "T", "V", "max_len"):
        assert call(**{name: -1}) == -1 and b"sizes" in lib.tmpnn_last_error(), name
    assert call(flags=2) == -1 and b"flag" in lib.tmpnn_last_error() and call(flags=-1) == -1
    assert call(cutoff=NAN) == -1 and b"NaN" in lib.tmpnn_last_error()
    assert call(k=86) == -2 and b"256" in lib.tmpnn_last_error() and call(k=257, depth=1) == -2 and call(k=1 << 30, depth=8) == -2
    assert call(max_len=2049) == -2 and b"2048" in lib.tmpnn_last_error()
    assert call(V=65537) == -2 and b"65536" in lib.tmpnn_last_error()
    assert call(V=65536, T=1 << 15) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert call(V=65536, T=(1 << 15) - 1, max_len=2048, k=256, depth=1, nbytes=64) == -4      # served at the top of every field
    assert call(nbytes=64) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert call(V=0, o1=None) == -1 and call(T=0, o5=None) == -1          # an empty call still needs its outputs
    none = dict(ddg=None, S=None, score=None, muts=None, offsets=None)
    assert call(V=0, nbytes=64, **none) == -4 and call(T=0, o4=None, nbytes=64, **none) == -4 and call(depth=1, muts=None, nbytes=64) == -4
    assert call(P=0, o1=None, o2=None, o3=None, o4=None, o5=None, ws=None, nbytes=0, **none) == 0     # no protein: nothing to do


def test_build_and_c_entries_need_no_gpu():
    from thermompnn_amd import _lib, build
    assert "tmpnn_beam.hip" in build.SOURCES and build.FILE_FLAGS["tmpnn_beam.hip"] == []       # the new kernels too honour NaNs
    for name in ("tmpnn_beam_step_each", "tmpnn_beam_step_each_workspace_bytes"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.tmpnn_beam_step_workspace_bytes(10, 100, 8, 2) >= 10 * 16 * 8                    # the single step's sizer is as it was
    cabi_errors_and_sizer_zeros(lib)
