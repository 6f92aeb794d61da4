"""Ranked hit lists, the parts that need no GPU: the numpy restatement of the contract against a brute-force loop, the argument
errors of tmpnn_hits_workspace_bytes / tmpnn_select_hits (before any launch), the CSV writer and the refused option combinations."""
import ctypes as C
import math

import numpy as np
import pytest

from hits_restatement import assert_hits_equal, hits_reference

NAN, INF = float("nan"), float("inf")


def _brute(table, S, offsets, k, cutoff, include_cys, one_per_position):
    """The contract read aloud: a Python loop, a Python sort on (value, position, letter) tuples."""
    P = len(offsets) - 1
    out = dict(hit_ddg=np.full((P, k), np.nan, np.float32), hit_pos=np.full((P, k), -1, np.int32),
               hit_aa=np.full((P, k), -1, np.int32), hit_count=np.zeros(P, np.int32))
    for b in range(P):
        cands = []
        for p in range(offsets[b + 1] - offsets[b]):
            t = offsets[b] + p
            here = []
            for a in range(20):
                v = float(table[t, a])
                if not S[t] < 20 or a == S[t] or math.isnan(v) or (a == 1 and not include_cys):
                    continue
                if cutoff is not None and not v <= cutoff:
                    continue
                here.append((v + 0.0, p, a))
            if one_per_position and here:
                best = here[0]
                for c in here[1:]:
                    if c[0] < best[0]:
                        best = c
                here = [best]
            cands += here
        cands.sort()
        for r, (_, p, a) in enumerate(cands[:k]):
            out["hit_ddg"][b, r], out["hit_pos"][b, r], out["hit_aa"][b, r] = table[offsets[b] + p, a], p, a
        out["hit_count"][b] = min(k, len(cands))
    return out


def test_restatement_equals_a_brute_force_loop_on_five_residues():
    rng = np.random.default_rng(0)
    pool = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, NAN, INF, -INF], np.float32)
    table = pool[rng.integers(0, len(pool), size=(5, 21))]
    table[0, 3], table[1, 3] = -0.0, 0.0                  # a +-0 tie across positions: the position decides, the bits stay
    S = np.array([4, 1, 20, 0, 19], np.int32)             # a wild-type C, a gap
    offsets = [0, 3, 3, 5]                                # an empty protein in the middle
    for k in (1, 7, 64):
        for cutoff in (None, 0.0, -1.5, -INF, -1e30):
            for cys in (False, True):
                for one in (False, True):
                    want = _brute(table, S, offsets, k, cutoff, cys, one)
                    assert_hits_equal(hits_reference(table, S, offsets, k, cutoff, cys, one), want)
    full = hits_reference(table, S, offsets, 64)
    assert np.isnan(full["hit_ddg"][1]).all() and (full["hit_pos"][1] == -1).all()


def test_argument_errors_need_no_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    size = lib.tmpnn_hits_workspace_bytes
    assert size(1000, 4, 0) == 0 and size(1000, 4, 257) == 0 and size(-1, 4, 8) == 0 and size(1000, 0, 8) == 0 and size(1 << 31, 1, 8) == 0
    assert size(1000, 4, 8) >= ((1000 >> 8) + 4) * 8 * 8
    assert size(0, 1, 1) > 0
    d = C.c_void_p(256)                                    # never dereferenced: every call below fails before a launch

    def call(ddg=d, ld=21, S=d, off=d, P=2, T=100, k=8, cutoff=INF, flags=0, o1=d, o2=d, o3=d, o4=d, ws=d, nbytes=1 << 20):
        return lib.tmpnn_select_hits(ddg, ld, S, off, P, T, k, cutoff, flags, o1, o2, o3, o4, ws, nbytes, None)

    for name in ("ddg", "S", "off", "o1", "o2", "o3", "o4", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(k=0) == -1 and b"k=0" in lib.tmpnn_last_error()
    assert call(k=257) == -1 and b"k=257" in lib.tmpnn_last_error()
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert call(P=-1) == -1 and call(T=-1) == -1
    assert call(flags=4) == -1 and b"flag" in lib.tmpnn_last_error()
    assert call(cutoff=NAN) == -1 and b"NaN" in lib.tmpnn_last_error()
    assert call(T=1 << 31) == -2                           # TMPNN_E_UNSUPPORTED
    assert call(nbytes=64) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert call(P=0) == 0                                  # nothing to do


def test_hit_csv_writer_on_a_hand_made_hit_set(tmp_path):
    from thermompnn_amd import ssm_scan
    hits = dict(hit_ddg=np.array([[-1.5, np.float32(0.1), NAN], [NAN, NAN, NAN], [-0.0, -INF, 2.0]], np.float32),
                hit_pos=np.array([[2, 0, -1], [-1, -1, -1], [1, 0, 0]], np.int32),
                hit_aa=np.array([[0, 19, -1], [-1, -1, -1], [3, 2, 4]], np.int32),
                hit_count=np.array([2, 0, 3], np.int32))
    out = tmp_path / "hits.csv"
    n = ssm_scan.write_hits_csv(str(out), hits, ["MKV", "--", "GA"], ["1abc", "empty", "d.pdb"], "ThermoMPNN", "custom")
    assert n == 5
    assert out.read_bytes() == (b",Model,Dataset,ddG_pred,position,wildtype,mutation,rank,pdb\n"
                                b"0,ThermoMPNN,custom,-1.5,2,V,A,0,1abc\n"
                                b"1,ThermoMPNN,custom,0.10000000149011612,0,M,Y,1,1abc\n"
                                b"2,ThermoMPNN,custom,-0.0,1,A,E,0,\n"
                                b"3,ThermoMPNN,custom,-inf,0,G,D,1,\n"
                                b"4,ThermoMPNN,custom,2.0,0,G,F,2,\n")
    np.testing.assert_array_equal(ssm_scan.sequence_letters(["AC-", "XY"]), [0, 1, 20, 20, 19])


@pytest.mark.parametrize("extra,word", [(["--pick_best"], "pick_best"), (["--centrality"], "centrality"),
                                        (["--out", "x.npz"], "npz"), (["--mutations", "m.csv"], "mutations")])
def test_cli_refuses_what_a_hit_list_cannot_be_combined_with(extra, word, capsys):
    from thermompnn_amd import ssm_scan
    with pytest.raises(SystemExit):
        ssm_scan.main(["a.pdb", "--synthetic_weights", "0", "--top", "5"] + extra)
    assert word in capsys.readouterr().err


def test_cli_and_library_refusals(monkeypatch, capsys):
    from thermompnn_amd import ssm_scan
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        ssm_scan.main(["a.pdb", "--synthetic_weights", "0", "--top", "5"])
    assert "multi-rank" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "1")
    for bad in (["--top", "0"], ["--top", "257"], ["--cutoff", "0.5"], ["--one_per_position"]):
        with pytest.raises(SystemExit):
            ssm_scan.main(["a.pdb", "--synthetic_weights", "0"] + bad)
        assert "top" in capsys.readouterr().err
    # the library call refuses the same combinations before it touches the engine
    for kw, word in ((dict(pick_best=True), "pick_best"), (dict(centrality=True), "centrality")):
        with pytest.raises(ValueError, match=word):
            ssm_scan.scan_to_file(None, ["a.pdb"], ["A"], "x.csv", top=5, **kw)
    with pytest.raises(ValueError, match="npz"):
        ssm_scan.scan_to_file(None, ["a.pdb"], ["A"], "x.npz", top=5)
    with pytest.raises(ValueError, match="top=k"):
        ssm_scan.scan_to_file(None, ["a.pdb"], ["A"], "x.csv", cutoff=0.0)
