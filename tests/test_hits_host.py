"""Ranked hit lists, the parts that need no GPU: the numpy restatement of the contract against a brute-force loop and against an
integer-key model of the header's order (on eight tie-heavy values and on arbitrary bit patterns, tests/hits_inputs.py), the argument
errors of tmpnn_hits_workspace_bytes / tmpnn_select_hits (before any launch), the CSV writer and the refused option combinations."""
import ctypes as C
import math

import numpy as np
import pytest

from hits_inputs import assert_table_is_hostile, bits_table, letters
from hits_restatement import assert_hits_equal, hits_reference

NAN, INF = float("nan"), float("inf")


def _brute(table, S, offsets, k, cutoff, include_cys, one_per_position):
    """The contract read aloud: a Python loop, a Python sort on (value, position, letter) tuples."""
    P = len(offsets) - 1
    out = dict(hit_ddg=np.full((P, k), np.nan, np.float32), hit_pos=np.full((P, k), -1, np.int32),
               hit_aa=np.full((P, k), -1, np.int32), hit_count=np.zeros(P, np.int32))
    if cutoff is not None:
        cutoff = float(np.float32(cutoff))                # the entry takes a float: a Python number is rounded once
    for b in range(P):
        cands = []
        for p in range(offsets[b + 1] - offsets[b]):
            t = offsets[b] + p
            here = []
            for a in range(20):
                v = float(table[t, a])
                if not 0 <= S[t] < 20 or a == S[t] or math.isnan(v) or (a == 1 and not include_cys):
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


BELOW_MINUS_ONE = np.nextafter(np.float32(-1), np.float32(0))        # -1 + 2^-24: the float32 between -1.0 and 0 next to -1.0
HOST_CUTOFFS = (None, 0.0, -0.0, -1.0, BELOW_MINUS_ONE, 1e-40, -INF)


def _bit_pattern_case():
    """15 rows of arbitrary bit patterns in four proteins (one empty, one of a single row), letters from -2 .. 22."""
    table, S = bits_table(15, 21, 5), letters(15, 6)
    S[[2, 7, 12]] = -1, -2, -1                            # (fifteen draws need not hold a negative letter: three are set)
    assert_table_is_hostile(table, S)
    assert (S < 0).any() and (S >= 20).any()
    return table, S, [0, 5, 5, 14, 15]


def test_restatement_equals_the_brute_force_loop_on_bit_patterns():
    """Denormals, negative and signalling NaNs, +-0, -inf, -1.0 and its neighbours, random patterns; a cutoff on a table value, one
    ulp beside it, a denormal one, -0.0. The device tests rest on the restatement at such values: here it is checked itself."""
    table, S, offsets = _bit_pattern_case()
    seen = set()
    for k in (1, 3, 32, 200):
        for cutoff in HOST_CUTOFFS:
            for cys in (False, True):
                for one in (False, True):
                    got = hits_reference(table, S, offsets, k, cutoff, cys, one)
                    assert_hits_equal(got, _brute(table, S, offsets, k, cutoff, cys, one))
                    seen.add((k, str(cutoff), tuple(got["hit_count"])))
    assert_hits_equal(hits_reference(table, S, offsets, 200, 0.0), hits_reference(table, S, offsets, 200, -0.0))
    assert len({c for k, _, c in seen if k == 200}) >= 5             # the cutoffs do select different sets
    assert hits_reference(table, S, offsets, 200)["hit_count"][1] == 0


def _ord(b):
    """The order-preserving image of IEEE-754 single bits on uint32 (include/tmpnn.h: -0.0 taken as +0.0)."""
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b).astype(np.uint32)
    return b ^ np.where(b >> 31 == 1, np.uint32(0xffffffff), np.uint32(0x80000000))


def _integer_key_model(table, S, offsets, k, cutoff, include_cys, one_per_position):
    """The header's definition in integers only: key = ord(bits) << 32 | p * 32 + a, non-candidates removed by the raw-bit rules,
    np.sort of the uint64 keys. No float compare anywhere."""
    none = np.uint64(0xffffffffffffffff)
    bits = np.ascontiguousarray(table).view(np.uint32)
    cut = _ord(np.array([np.inf if cutoff is None else cutoff], np.float32).view(np.uint32))[0]
    P = len(offsets) - 1
    out = dict(hit_ddg=np.full((P, k), np.nan, np.float32), hit_pos=np.full((P, k), -1, np.int32),
               hit_aa=np.full((P, k), -1, np.int32), hit_count=np.zeros(P, np.int32))
    aa = np.arange(20, dtype=np.int64)[None, :]
    for b in range(P):
        t0, t1 = int(offsets[b]), int(offsets[b + 1])
        v, s = bits[t0:t1, :20], np.asarray(S[t0:t1]).astype(np.int64)[:, None]
        o = _ord(v)
        ok = (s >= 0) & (s < 20) & (aa != s) & ((v & np.uint32(0x7fffffff)) <= np.uint32(0x7f800000)) & (o <= cut)
        if not include_cys:
            ok = ok & (aa != 1)
        low = (np.arange(t1 - t0, dtype=np.int64)[:, None] * 32 + aa).astype(np.uint64)
        keys = np.where(ok, (o.astype(np.uint64) << np.uint64(32)) | low, none)
        if one_per_position:
            keys = keys.min(axis=1) if t1 > t0 else keys.reshape(-1)
        keys = np.sort(keys[keys != none], axis=None)[:k]
        n = len(keys)
        p, a = ((keys & np.uint64(0xffffffff)) >> np.uint64(5)).astype(np.int64), (keys & np.uint64(31)).astype(np.int64)
        out["hit_ddg"][b, :n] = table[t0 + p, a]
        out["hit_pos"][b, :n], out["hit_aa"][b, :n], out["hit_count"][b] = p, a, n
    return out


def test_integer_keys_order_as_value_position_letter_over_the_float_range():
    """Two formulations of one order: float compares and np.lexsort (the restatement) against ascending 64-bit integer keys (what
    the kernel sorts). Equal on bit-pattern tables and on a table of neighbouring floats around 0, +-1, the denormal edge and
    +-FLT_MAX, at cutoffs on, beside and between table values."""
    assert _ord(np.array([0x80000000, 0, 0xff800000, 0x7f800000, 0xffc00000, 0x7fc00000], np.uint32)).tolist() == \
        [0x80000000, 0x80000000, 0x007fffff, 0xff800000, 0x003fffff, 0xffc00000]
    table, S, offsets = _bit_pattern_case()
    edges = np.array([0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f7fffff, 0x3f800000, 0x3f800001, 0x7f7fffff, 0x7f800000],
                     np.uint32)
    grid = np.concatenate([edges, edges | np.uint32(0x80000000)])
    rng = np.random.default_rng(9)
    near = grid[rng.integers(0, len(grid), size=(40, 20))].view(np.float32)
    S_near = rng.integers(-1, 21, size=40).astype(np.int32)
    for tab, s, off in ((table, S, offsets), (near, S_near, [0, 0, 33, 40]), (bits_table(300, 20, 12), letters(300, 13), [0, 300])):
        for k in (1, 3, 32, 200):
            for cutoff in HOST_CUTOFFS + (INF, 1.0, float(np.float32(1e-45)), -3.4028235e38):
                for cys, one in ((False, False), (True, True), (False, True)):
                    assert_hits_equal(_integer_key_model(tab, s, off, k, cutoff, cys, one), hits_reference(tab, s, off, k, cutoff, cys, one))


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
