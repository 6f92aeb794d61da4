"""Per-site-pair maps, the parts that need no GPU: the numpy restatement of tmpnn_pair_map against a brute-force Python loop on
tie-dominated inputs (with a state carried over several calls), decode_pair_map's round trips, the front end's chunk loop, .npz and
command line through stub table and reduction functions held against double_mutant_table of the same stub tables, the contiguity check
of the rows, and the argument errors and sizer zeros of the two C entries (before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pair_hits_restatement import NONE, ord32, unord32
from pair_map_restatement import MAX_LEN, STATE, assert_pair_map_equal, decode_reference, empty_state, pair_map_reference

NAN, INF = float("nan"), float("inf")
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
# few values, so that sums and differences tie: +-0, +-inf (inf - inf = NaN), NaN, a denormal, and 1 beside 1 + ulp
POOL = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, NAN, INF, -INF], np.float32)


def _crafted(V, L, R, seed, ld=21):
    rng = np.random.default_rng(seed)
    ddg = POOL[rng.integers(0, len(POOL), size=(V, L, ld))]
    wt = POOL[rng.integers(0, len(POOL), size=(L, ld))]
    base = POOL[rng.integers(0, len(POOL), size=V)]
    S_var = rng.integers(-1, 22, size=(V, L)).astype(np.int32)
    row = np.sort(rng.integers(0, R, size=V)).astype(np.int32)
    letter = rng.integers(0, 20, size=V).astype(np.int32)
    skip = rng.integers(-1, L, size=V).astype(np.int32)
    return dict(ddg=ddg, S_var=S_var, base=base, row=row, letter=letter, skip=skip, wt=wt)


def _brute(c, sl, R, include_cys, upper, carried):
    """The contract read aloud: a Python loop over (v, q, b) with np.float32 arithmetic and Python tuples (value, a, b); ``carried``:
    the per-entry lists of an earlier call. -> the state as the restatement's dict, and the lists."""
    ddg, S_var, base, row, letter, skip, wt = (c[k][sl] if k != "wt" else c[k] for k in ("ddg", "S_var", "base", "row", "letter", "skip", "wt"))
    V, L = S_var.shape
    best, lo, hi, total, count = carried
    for v in range(V):
        r, a = int(row[v]), int(letter[v])
        if not 0 <= r < R:
            continue
        for q in range(L):
            s = int(S_var[v, q])
            inner, n = np.float32(0.0), 0
            if 0 <= a < 20 and 0 <= s < 20 and not (q <= skip[v] if upper else q == skip[v]):
                for b in range(20):
                    if b == s or (b == 1 and not include_cys):
                        continue
                    with np.errstate(invalid="ignore"):
                        val = float(np.float32(base[v]) + np.float32(ddg[v, q, b]))
                        e = float(np.float32(ddg[v, q, b]) - np.float32(wt[q, b]))
                    if not math.isnan(val):
                        best[r][q] = min(best[r][q], (val + 0.0, a, b))
                    if not math.isnan(e):
                        lo[r][q] = min(lo[r][q], (e + 0.0, a, b))
                        hi[r][q] = min(hi[r][q], (-(e + 0.0), a, b))
                        inner = np.float32(inner + np.float32(abs(e)))
                        n += 1
            total[r][q] = np.float32(total[r][q] + inner)
            count[r][q] += n
    out = empty_state(R, L)
    for r in range(R):
        for q in range(L):
            for name, cell, sign in (("best", best[r][q], 1.0), ("eps_lo", lo[r][q], 1.0), ("eps_hi", hi[r][q], -1.0)):
                if cell[1] == 99:
                    continue
                o = int(ord32(np.array([np.float32(sign * cell[0] + 0.0)]).view(np.uint32))[0])
                out[name][r, q] = np.uint64(((o ^ 0xffffffff if sign < 0 else o) << 32) | cell[1] << 5 | cell[2])
            out["eps_abs_sum"][r, q], out["count"][r, q] = total[r][q], count[r][q]
    return out, (best, lo, hi, total, count)


def _fresh(R, L):
    none = (INF, 99, 99)                                                  # (a live tuple with value +inf has a < 20 and sorts first)
    cell = lambda x: [[x for _ in range(L)] for _ in range(R)]
    return cell(none), cell(none), cell(none), cell(np.float32(0.0)), cell(0)


def _ref(c, R, sl=slice(None), state=None, **kw):
    return pair_map_reference(c["ddg"][sl], c["S_var"][sl], c["base"][sl], c["row"][sl], c["letter"][sl], c["skip"][sl], c["wt"], R,
                              kw.get("include_cys", False), kw.get("upper", False), state)


def test_restatement_equals_a_brute_force_loop_over_three_calls():
    from thermompnn_amd import _lib
    assert [(name, np.dtype(dt).name.replace("uint64", "int64")) for name, dt in STATE] == list(_lib.PMAP_STATE)   # the library's state, array for array
    R, L = 4, 6
    c = _crafted(11, L, 3, 0)                                            # rows 0 .. 2 named, row 3 never
    c["row"][9], c["row"][10], c["letter"][8] = 7, -1, 20                 # rows beyond both ends, a letter beyond the field
    c["base"][4] = NAN
    bits = set(c["ddg"].view(np.uint32).ravel().tolist())
    assert {0x80000000, 0, 0x7f800000, 0xff800000, 0x3f800000, 0x3f800001} <= bits and any(0 < x < 0x00800000 for x in bits)
    for cys in (False, True):
        for upper in (False, True):
            kw = dict(include_cys=cys, upper=upper)
            state, carried = None, _fresh(R, L)
            for v0, v1 in ((0, 4), (4, 5), (5, 11)):                      # the middle cut lies inside a run
                got = _ref(c, R, slice(v0, v1), state, **kw)
                want, carried = _brute(c, slice(v0, v1), R, cys, upper, carried)
                assert_pair_map_equal(got, want)
                state = got
            assert_pair_map_equal(state, _ref(c, R, **kw))                # the cut into calls does not show
            assert (state["best"][3] == NONE).all() and (state["count"][3] == 0).all() and (state["count"][:3] > 0).any()
            assert np.isnan(state["eps_abs_sum"]).sum() == 0 and np.isinf(state["eps_abs_sum"]).any()
    # the inverted word orders the other way, and ties go to the smallest (a, b) in both
    one = dict(ddg=np.zeros((2, 1, 20), np.float32), S_var=np.full((2, 1), 5, np.int32), base=np.zeros(2, np.float32),
               row=np.zeros(2, np.int32), letter=np.array([7, 3], np.int32), skip=np.full(2, -1, np.int32), wt=np.zeros((1, 20), np.float32))
    one["ddg"][0, 0, [2, 4]], one["ddg"][1, 0, [2, 9]] = (-1.0, 2.0), (-1.0, 2.0)
    d = decode_reference(_ref(one, 1))
    assert (d["best_ddG"][0, 0], d["best_a"][0, 0], d["best_b"][0, 0]) == (-1.0, 3, 2)
    assert (d["eps_min"][0, 0], d["eps_min_a"][0, 0], d["eps_min_b"][0, 0]) == (-1.0, 3, 2)
    assert (d["eps_max"][0, 0], d["eps_max_a"][0, 0], d["eps_max_b"][0, 0]) == (2.0, 3, 9)
    assert d["count"][0, 0] == 36 and d["eps_abs_mean"][0, 0] == np.float32(6.0) / np.float32(36)


def test_decode_pair_map_round_trips_on_numpy_and_torch():
    from thermompnn_amd.engine import decode_pair_map
    vals = np.array([-INF, -3.0, -1e-40, 0.0, 1e-40, 1.0, ONE_UP, INF], np.float32)
    R, L = 2, len(vals) + 1
    st = empty_state(R, L)
    o = ord32(vals.view(np.uint32)).astype(np.uint64)
    for r, (a, b) in enumerate(((0, 0), (19, 19))):
        low = np.uint64(a << 5 | b)
        st["best"][r, :-1] = (o << np.uint64(32)) | low
        st["eps_lo"][r, :-1] = (o[::-1] << np.uint64(32)) | low
        st["eps_hi"][r, :-1] = ((~o & np.uint64(0xffffffff)) << np.uint64(32)) | low
        st["eps_abs_sum"][r, :-1], st["count"][r, :-1] = np.arange(1, L, dtype=np.float32), np.arange(1, L) * 3
    want = decode_reference(st)
    np.testing.assert_array_equal(want["best_ddG"][:, :-1].view(np.uint32), np.tile(vals, (2, 1)).view(np.uint32))
    np.testing.assert_array_equal(want["eps_min"][:, :-1], np.tile(vals[::-1], (2, 1)))
    np.testing.assert_array_equal(want["eps_max"][:, :-1], np.tile(vals, (2, 1)))
    assert (want["best_a"][1, :-1] == 19).all() and (want["eps_max_b"][1, :-1] == 19).all() and (want["eps_min_a"][0, :-1] == 0).all()
    assert np.isnan(want["best_ddG"][:, -1]).all() and (want["eps_min_b"][:, -1] == -1).all() and np.isnan(want["eps_abs_mean"][:, -1]).all()
    as_torch = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in st.items()}
    for got in (decode_pair_map(st), decode_pair_map({k: v.view(np.int64) if v.dtype == np.uint64 else v for k, v in st.items()}),
                decode_pair_map(as_torch)):
        assert set(got) == set(want)
        for name, w in want.items():
            g = np.asarray(got[name])
            assert g.dtype == w.dtype and g.shape == w.shape, name
            if w.dtype == np.float32:
                np.testing.assert_array_equal(g.view(np.uint32)[~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)
                assert np.isnan(g[np.isnan(w)]).all(), name
            else:
                np.testing.assert_array_equal(g, w, err_msg=name)
    # a -0.0 comes back as +0.0: the image has one preimage
    assert unord32(ord32(np.array([0x80000000], np.uint32)))[0] == 0


# ---- the front end on stub tables -----------------------------------------------------------------------------------------------
STUB_POOL = np.array([-2.0, -1.25, -0.5, 0.0, 0.125, 0.75, 1e-40, ONE_UP], np.float32)
SEQ = "MKC-AXGWCYLE"


def stub_tables(S):
    """A table function without a model: [V, L] -> [V, L, 21] drawn from eight values by a hash of the whole sequence, the position
    and the letter (so that a background changes every row), zero at the variant's own residue, as a ddG table is."""
    S = np.asarray(S, dtype=np.int64)
    V, L = S.shape
    h = (S * (np.arange(L) * 7 + 3)[None]).sum(1)
    idx = (h[:, None, None] * 5 + np.arange(L)[None, :, None] * 11 + np.arange(21)[None, None, :] * 13 + S[:, :, None] * 17) % len(STUB_POOL)
    t = STUB_POOL[idx]
    t[np.arange(V)[:, None], np.arange(L)[None], np.minimum(S, 20)] = 0.0
    return torch.from_numpy(t)


class StubReduce:
    """Engine.pair_map on the host: the restatement, call by call, the state as int64 / float32 / int32 torch tensors."""
    def __init__(self):
        self.chunks = []

    def __call__(self, ddg, S_var, base, row, letter, wt, R, skip=None, include_cys=False, upper=False, state=None):
        from thermompnn_amd.engine import check_row_runs
        check_row_runs(row, R)
        self.chunks.append(int(ddg.shape[0]))
        old = None if state is None else {k: v.numpy() for k, v in state.items()}
        r = pair_map_reference(ddg.numpy(), S_var, base.numpy(), row, letter, skip, wt.numpy(), R, include_cys, upper, old)
        return {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in r.items()}


def _table_maps(seq, positions, include_cys, unordered):
    """The same maps from double_mutant_table of the stub tables [P, 20, L, 20] and from the backgrounds' own tables, by masked
    minima over the letter axes: the table's entries ARE the sums (the same single fp32 add)."""
    from thermompnn_amd.variant_scan import double_mutant_table, sequence_indices
    wt_idx = sequence_indices(seq)
    P, L = len(positions), len(seq)
    dm = double_mutant_table(None, [{"seq": seq}], positions=positions, chunk=7, _tables=stub_tables).numpy()
    wt = stub_tables(wt_idx[None])[0].numpy()
    a, b = np.arange(20)[None, :, None, None], np.arange(20)[None, None, None, :]
    p, q = np.array(positions)[:, None, None, None], np.arange(L)[None, None, :, None]
    ok = (a != wt_idx[positions][:, None, None, None]) & (b != wt_idx[None, None, :, None]) & (wt_idx[None, None, :, None] < 20)
    ok = ok & ((q > p) if unordered else (q != p))
    if not include_cys:
        ok = ok & (a != 1) & (b != 1)
    e = np.empty((P, 20, L, 20), np.float32)
    for k, pp in enumerate(positions):
        for aa in range(20):
            S = wt_idx.copy()
            S[pp] = aa
            e[k, aa] = stub_tables(S[None])[0].numpy()[:, :20] - wt[:, :20]
    flat = lambda x: x.transpose(0, 2, 1, 3).reshape(P, L, 400)           # [P, L, (a, b)]: argmin takes the first minimum in (a, b) order
    ok_f = flat(np.broadcast_to(ok, dm.shape))
    out = dict(count=ok_f.sum(axis=2).astype(np.int32))
    for name, x, sign in (("best_ddG", dm, 1.0), ("eps_min", e, 1.0), ("eps_max", e, -1.0)):
        m = np.where(ok_f, flat(x) * np.float32(sign) + np.float32(0.0), np.float32(INF))
        at = m.argmin(axis=2)
        val = np.take_along_axis(flat(x) + np.float32(0.0), at[:, :, None], 2)[:, :, 0]
        none = ~ok_f.any(axis=2)
        stem = "best" if name == "best_ddG" else name
        out[name] = np.where(none, np.float32(NAN), val).astype(np.float32)
        out[stem + "_a"], out[stem + "_b"] = np.where(none, -1, at // 20).astype(np.int32), np.where(none, -1, at % 20).astype(np.int32)
    total = np.where(ok_f, np.abs(flat(e)).astype(np.float64), 0.0).sum(axis=2)
    out["eps_abs_mean64"] = np.where(out["count"] > 0, total / np.maximum(out["count"], 1), np.nan)
    return out, wt


def _assert_map_is(m, want, wt, positions, seq):
    assert m.seq == seq and m.positions.tolist() == list(positions)
    np.testing.assert_array_equal(m.wt.view(np.uint32), wt.view(np.uint32))
    for name in ("best_ddG", "eps_min", "eps_max"):
        g, w = getattr(m, name), want[name]
        assert g.dtype == np.float32 and g.shape == w.shape
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        np.testing.assert_array_equal(g.view(np.uint32)[~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)], err_msg=name)   # the same fp32 add
    for name in ("best_a", "best_b", "eps_min_a", "eps_min_b", "eps_max_a", "eps_max_b", "count"):
        assert getattr(m, name).dtype == np.int32
        np.testing.assert_array_equal(getattr(m, name), want[name], err_msg=name)
    live = want["count"] > 0
    np.testing.assert_allclose(m.eps_abs_mean[live], want["eps_abs_mean64"][live], rtol=1e-6)
    assert np.isnan(m.eps_abs_mean[~live]).all()


def test_front_end_chunk_loop_on_stub_tables_equals_the_double_mutant_table():
    from thermompnn_amd.variant_scan import PairMap, double_mutant_map
    pdb = [{"seq": SEQ, "name": "stub"}]
    sites = [p for p, c in enumerate(SEQ) if c not in "-X"]
    for kw in (dict(), dict(unordered=True), dict(include_cys=True), dict(positions=[11, 0, 4], unordered=True, include_cys=True)):
        positions = sorted(kw.get("positions", sites))
        want, wt = _table_maps(SEQ, positions, kw.get("include_cys", False), kw.get("unordered", False))
        first = None
        for chunk in (1, 7, 1000):
            red = StubReduce()
            m = double_mutant_map(None, pdb, chunk=chunk, _tables=stub_tables, _reduce=red, **kw)
            assert isinstance(m, PairMap)
            _assert_map_is(m, want, wt, positions, SEQ)
            n_bg = sum(red.chunks)
            assert max(red.chunks) <= chunk and len(red.chunks) == -(-n_bg // chunk)
            per_site = 19 if kw.get("include_cys") else 18
            assert n_bg == sum(per_site + (1 if SEQ[p] == "C" and not kw.get("include_cys") else 0) for p in positions)
            if first is None:
                first = m
            for name in PairMap.ARRAYS:                                   # the chunk size does not show, not even in the mean's bits
                x, y = getattr(first, name), getattr(m, name)
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
        # a pair without a double mutant: its own site, a site without a letter, and with `unordered` every site in front
        k = positions.index(4)
        assert np.isnan(m.best_ddG[k, 4]) and m.count[k, 4] == 0 and m.count[k, 3] == 0 and m.count[k, 5] == 0 and m.best_a[k, 3] == -1
        assert (m.count[k, :4] == 0).all() == bool(kw.get("unordered")) and m.count[k, 6] > 0
    empty = double_mutant_map(None, pdb, positions=[], _tables=stub_tables, _reduce=StubReduce())
    assert empty.best_ddG.shape == (0, len(SEQ)) and empty.count.shape == (0, len(SEQ)) and empty.wt.shape == (len(SEQ), 21)
    for bad, word in ((dict(positions=[3]), "position 3"), (dict(positions=[5]), "position 5"), (dict(positions=[12]), "position 12"),
                      (dict(chunk=0), "chunk")):
        with pytest.raises(ValueError, match=word):
            double_mutant_map(None, pdb, _tables=stub_tables, _reduce=StubReduce(), **bad)
    with pytest.raises(ValueError, match="2048"):
        double_mutant_map(None, [{"seq": "A" * 2049}], _tables=stub_tables, _reduce=StubReduce())


def test_rows_of_one_call_must_be_contiguous():
    from thermompnn_amd._lib import TmpnnError
    from thermompnn_amd.engine import check_row_runs
    for ok in ([], [0], [0, 0, 1, 1, 2], [2, 2, 0, 1], np.array([3, 3, 3], np.int32), [5, 0, 5, 1, -1, 2, -1], [0, 9, 1, 9]):
        check_row_runs(ok, 4)                                             # rows outside [0, 4) name no state row
    for bad, word in (([0, 1, 0], "row 0"), ([1, 1, 2, 1], "variant 3"), (np.array([0, 5, 0]), "row 0"), ([3, 2, 1, 0, 3], "row 3")):
        with pytest.raises(TmpnnError, match=word):
            check_row_runs(bad, 4)
    with pytest.raises(TmpnnError, match="contiguous"):
        StubReduce()(torch.zeros((3, 2, 21)), np.zeros((3, 2), np.int32), torch.zeros(3), [0, 1, 0], [0, 0, 0], torch.zeros((2, 21)), 2)


def test_command_line_writes_the_npz(tmp_path, capsys):
    from thermompnn_amd import variant_scan
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    X, seq = synthetic_backbone(14, 5)
    path = tmp_path / "tiny.pdb"
    path.write_text(backbone_pdb_text(X, seq))
    pdb = alt_parse_PDB(str(path), "A")
    out = tmp_path / "map.npz"
    argv = [str(path), "--chain", "A", "--pair-map", "--unordered", "--include_cys", "--chunk", "50", "--out", str(out)]
    assert variant_scan.main(argv, _tables=stub_tables, _reduce=StubReduce()) == 0
    m = variant_scan.double_mutant_map(None, pdb, unordered=True, include_cys=True, _tables=stub_tables, _reduce=StubReduce())
    assert f"{14 * 13 // 2} site pairs of 14 residues, {14 * 13 // 2 * 361} double mutants" in capsys.readouterr().out
    want, wt = _table_maps(seq, list(range(14)), True, True)
    _assert_map_is(m, want, wt, list(range(14)), seq)
    z = np.load(out)
    assert sorted(z.files) == sorted(variant_scan.PairMap.ARRAYS + ("seq",)) and str(z["seq"]) == seq
    for name in variant_scan.PairMap.ARRAYS:
        x = getattr(m, name)
        assert z[name].dtype == x.dtype and z[name].tobytes() == x.tobytes(), name
    assert z["best_ddG"].shape == (14, 14) and z["positions"].tolist() == list(range(14))
    # --pair-map is a fourth member of the exclusive group; --include_cys / --unordered are its options too, --cutoff is not
    base = [str(path), "--out", str(out), "--synthetic_weights", "0"]
    for bad, word in ((["--pair-map", "--all-singles"], "not allowed with"), (["--pair-map", "--top-pairs", "5"], "not allowed with"),
                      (["--pair-map", "--variants", "v.txt"], "not allowed with"), (["--pair-map", "--cutoff", "1"], "--cutoff belongs to --top-pairs"),
                      (["--all-singles", "--unordered"], "--pair-map"), (["--all-singles", "--include_cys"], "--pair-map"), ([], "required")):
        with pytest.raises(SystemExit):
            variant_scan.main(base + bad, _tables=stub_tables, _reduce=StubReduce())
        assert word in capsys.readouterr().err, bad


def test_argument_errors_and_sizer_zeros_need_no_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    size = lib.tmpnn_pair_map_workspace_bytes
    assert size(-1, 100) == 0 and size(10, -1) == 0 and size(10, 2049) == 0
    assert size((1 << 31) // 2048 + 1, 2048) == 0 and size(1 << 31, 1) == 0
    assert size((1 << 31) // 2048 - 1, 2048) >= ((1 << 31) - 4096) * 32 and size(256, 256) >= 256 * 256 * 32
    assert 0 < size(0, 100) < 1024 and 0 < size(10, 0) < 1024 and size(37, 19) >= 37 * 19 * 32
    d = C.c_void_p(256)                                                   # never dereferenced: every call below fails before a launch

    def call(ddg=d, ld=21, S=d, base=d, row=d, letter=d, skip=d, wt=d, ld_wt=21, V=4, L=100, R=3, flags=0, best=d, lo=d, hi=d, total=d,
             count=d, ws=d, nbytes=1 << 20):
        return lib.tmpnn_pair_map(ddg, ld, S, base, row, letter, skip, wt, ld_wt, V, L, R, flags, best, lo, hi, total, count, ws, nbytes, None)

    for name in ("ddg", "S", "base", "row", "letter", "skip", "wt", "best", "lo", "hi", "total", "count", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert call(ld_wt=19) == -1 and b"ld_wt=19" in lib.tmpnn_last_error()
    assert call(V=-1) == -1 and b"sizes" in lib.tmpnn_last_error() and call(L=-1) == -1 and call(R=-1) == -1
    assert call(flags=8) == -1 and b"flag" in lib.tmpnn_last_error() and call(flags=-1) == -1
    assert call(L=2049) == -2 and b"2048" in lib.tmpnn_last_error()       # TMPNN_E_UNSUPPORTED
    assert call(V=(1 << 31) // 2048 + 1, L=2048) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert call(R=(1 << 31) // 100 + 1) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert call(nbytes=size(4, 100) - 257) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert call(V=0, best=None) == -1 and call(V=0, ddg=None, wt=None, ws=None) == -1    # an empty call still needs its state and workspace
    nothing = dict(best=None, lo=None, hi=None, total=None, count=None)   # an empty state has no address, and nothing is launched
    assert call(L=0, ddg=None, S=None, wt=None, **nothing) == 0 and call(R=0, **nothing) == 0 and call(R=0, flags=4, **nothing) == 0
    assert call(R=0, nbytes=64, **nothing) == -4 and call(R=0, ld=19, **nothing) == -1               # the errors come first
    assert (_lib.PMAP_INCLUDE_CYS, _lib.PMAP_UPPER, _lib.PMAP_CONTINUE, _lib.PMAP_MAX_LEN) == (1, 2, 4, MAX_LEN)
    assert [name for name, _ in _lib.PMAP_STATE] == [name for name, _ in STATE]
