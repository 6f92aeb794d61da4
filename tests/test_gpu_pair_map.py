"""Per-site-pair maps over variant tables on the device (tmpnn_pair_map, Engine.pair_map) and the double-mutant front end on top of
them (variant_scan.double_mutant_map, TransferModel.double_mutant_map, --pair-map) against the numpy restatement of the contract
(tests/pair_map_restatement.py). Every comparison with the restatement is exact: the three key arrays, the counts and the bits of the
|e| sums. The tables of the reduction tests are synthetic; only the end-to-end test runs a model.

The crafted call has V = 37 variants over 5 rows. Runs of 1, 19 and 20 variants do not fit into 37 together, so the 37 variants are
laid out twice: ROWS_A has runs of 1, 19, 5, 11 and 1, ROWS_B runs of 20, 1, 1, 14 and 1; ROWS_C is ROWS_A with two runs sent to rows
that do not exist."""
import numpy as np
import pytest
import torch

from pair_hits_restatement import NONE
from pair_map_restatement import STATE, assert_pair_map_equal, decode_reference, pair_map_reference

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
# few values, so that sums and differences tie: +-0, +-inf (inf - inf = NaN), NaN, a denormal, and 1 beside 1 + ulp
POOL = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, NAN, INF, -INF], np.float32)
NAMES = tuple(name for name, _ in STATE)
V, R = 37, 6                                                              # row 5 is never named
ROWS_A = np.repeat([2, 0, 4, 1, 3], [1, 19, 5, 11, 1]).astype(np.int32)
ROWS_B = np.repeat([0, 3, 1, 4, 2], [20, 1, 1, 14, 1]).astype(np.int32)
ROWS_C = np.repeat([2, 0, R, 1, -1], [1, 19, 5, 11, 1]).astype(np.int32)


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _draw(n, L, seed, ld=21):
    rng = np.random.default_rng(seed)
    c = dict(ddg=POOL[rng.integers(0, len(POOL), size=(n, L, ld))], wt=POOL[rng.integers(0, len(POOL), size=(L, ld))],
             base=POOL[rng.integers(0, len(POOL), size=n)], S_var=rng.integers(-2, 22, size=(n, L)).astype(np.int32),
             letter=rng.integers(0, 20, size=n).astype(np.int32), skip=rng.integers(-1, L, size=n).astype(np.int32))
    return c


@pytest.fixture(scope="module")
def crafted():
    """{(L, ld): the 37 variants}; L = 19 and 70 are no multiples of 64, and 37 x 70 = 2 590 table rows make 11 tiles of 256 whose
    borders fall inside variants. Left unchanged by the tests that share it."""
    out = {}
    for L, ld in ((19, 21), (19, 20), (70, 21), (70, 20)):
        c = _draw(V, L, L + ld, ld)
        c["letter"][[3, 20, 30]] = 20, -1, 35                             # out of range: these variants contribute nothing
        c["letter"][[0, 1]] = 0, 19
        c["skip"][[0, 1, 2, 3]] = -1, 0, L - 1, L - 1
        c["base"][5] = NAN                                                # no best value from this variant, its epistasis still counts
        bits = set(c["ddg"].view(np.uint32).ravel().tolist())
        assert {0x80000000, 0, 0x7f800000, 0xff800000, 0x3f800000, 0x3f800001} <= bits and any(0 < b < 0x00800000 for b in bits)
        assert (c["S_var"] < 0).any() and (c["S_var"] == 20).any()
        out[L, ld] = c
    return out


def _ref(c, rows, sl=slice(None), state=None, R=R, **kw):
    return pair_map_reference(c["ddg"][sl], c["S_var"][sl], c["base"][sl], rows[sl], c["letter"][sl], None if kw.get("no_skip") else c["skip"][sl],
                              c["wt"], R, kw.get("include_cys", False), kw.get("upper", False), state)


def _run(engine, c, rows, sl=slice(None), state=None, dev=None, R=R, **kw):
    ddg, wt = dev if dev is not None else (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    return engine.pair_map(ddg[sl], c["S_var"][sl], c["base"][sl], rows[sl], c["letter"][sl], wt, R, skip=None if kw.get("no_skip") else c["skip"][sl],
                           include_cys=kw.get("include_cys", False), upper=kw.get("upper", False), state=state)


def _state_of(ref):
    """A restatement's state as the device tensors Engine.pair_map continues from."""
    return {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in ref.items()}


def test_crafted_call_every_flag_length_stride_and_row_layout(engine, crafted):
    seen_none = seen_inf = False
    for (L, ld), c in crafted.items():
        dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
        for rows in (ROWS_A, ROWS_B, ROWS_C):
            for kw in (dict(), dict(include_cys=True), dict(upper=True), dict(include_cys=True, upper=True), dict(no_skip=True)):
                got, want = _run(engine, c, rows, dev=dev, **kw), _ref(c, rows, **kw)
                assert_pair_map_equal(got, want)
                for name, dt in STATE:
                    assert got[name].shape == (R, L) and got[name].is_cuda and got[name].dtype == (torch.int64 if dt == np.uint64 else getattr(torch, np.dtype(dt).name))
                seen_none |= bool((want["best"][:5] == NONE).any() and (want["best"][:5] != NONE).any())
                seen_inf |= bool(np.isinf(want["eps_abs_sum"]).any())
                assert (want["count"][5] == 0).all() and (want["count"][:2] > 0).any()
        # a rerun has the same bits
        a, b = _run(engine, c, ROWS_A, dev=dev, upper=True), _run(engine, c, ROWS_A, dev=dev, upper=True)
        assert all(torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)) for name in NAMES)
        # a row stride above the columns is the table's leading dimension, for ddg and for wt; a view that is no such table is copied
        wide_d, wide_w = torch.full((V, L, 24), -5.0, device="cuda"), torch.full((L, 27), -5.0, device="cuda")
        wide_d[:, :, :ld], wide_w[:, :ld] = dev
        assert wide_w[:, :ld].stride(0) == 27
        assert_pair_map_equal(_run(engine, c, ROWS_B, dev=(wide_d[:, :, :ld], wide_w[:, :ld])), _ref(c, ROWS_B))
        odd_d, odd_w = torch.full((V, L, 2 * ld), -5.0, device="cuda"), torch.full((L, 2 * ld), -5.0, device="cuda")
        odd_d[:, :, ::2], odd_w[:, ::2] = dev
        assert_pair_map_equal(_run(engine, c, ROWS_B, dev=(odd_d[:, :, ::2], odd_w[:, ::2])), _ref(c, ROWS_B))
    assert seen_none and seen_inf
    # the rows given as a device tensor are not checked on the host; as numpy or a list they are
    from thermompnn_amd._lib import TmpnnError
    c = crafted[19, 21]
    assert_pair_map_equal(engine.pair_map(torch.from_numpy(c["ddg"]).cuda(), c["S_var"], c["base"], torch.from_numpy(ROWS_A).cuda(), c["letter"],
                                          torch.from_numpy(c["wt"]).cuda(), R, skip=c["skip"]), _ref(c, ROWS_A))
    back = ROWS_A.copy()
    back[36] = 2
    with pytest.raises(TmpnnError, match="row 2"):
        _run(engine, c, back)
    for bad in (dict(R=-1), dict(state={"best": torch.zeros((R, 19), dtype=torch.int64, device="cuda")})):
        with pytest.raises(TmpnnError):
            _run(engine, c, ROWS_A, **bad)
    with pytest.raises(TmpnnError, match="device"):
        engine.pair_map(torch.from_numpy(c["ddg"]), c["S_var"], c["base"], ROWS_A, c["letter"], torch.from_numpy(c["wt"]).cuda(), R)
    with pytest.raises(TmpnnError, match="wt"):
        engine.pair_map(torch.from_numpy(c["ddg"]).cuda(), c["S_var"], c["base"], ROWS_A, c["letter"], torch.from_numpy(c["wt"][:5]).cuda(), R)
    with pytest.raises(TmpnnError, match="2048"):
        engine.pair_map(torch.zeros((1, 2049, 21), device="cuda"), np.zeros((1, 2049), np.int32), [0.0], [0], [0], torch.zeros((2049, 21), device="cuda"), 1)


@pytest.mark.parametrize("L,ld", [(19, 21), (70, 20)])
def test_any_cut_into_calls_gives_the_same_bits(engine, crafted, L, ld):
    c = crafted[L, ld]
    dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    cuts = ((1, 36), (10, 27), (20, 1, 16), (5, 7, 18, 7), (1,) * 37)     # order kept; 10, 12, 30 and most of the singles cut inside a run
    for rows, kw in ((ROWS_A, dict()), (ROWS_B, dict(include_cys=True, upper=True)), (ROWS_C, dict(no_skip=True))):
        whole = _run(engine, c, rows, dev=dev, **kw)
        assert_pair_map_equal(whole, _ref(c, rows, **kw))
        for cut in cuts:
            assert sum(cut) == V
            state, v0 = None, 0
            for n in cut:
                state = _run(engine, c, rows, sl=slice(v0, v0 + n), state=state, dev=dev, **kw)
                v0 += n
            for name in NAMES:
                assert torch.equal(state[name], whole[name]), (name, cut)                     # (a sum from +0.0 is never NaN)
                assert torch.equal(state[name].view(torch.int32), whole[name].view(torch.int32)), (name, cut)
    # the state of the first call of a cut is what the restatement carries
    first, want = _run(engine, c, ROWS_A, sl=slice(0, 10), dev=dev), _ref(c, ROWS_A, sl=slice(0, 10))
    assert_pair_map_equal(first, want)
    assert_pair_map_equal(_run(engine, c, ROWS_A, sl=slice(10, 37), state=first, dev=dev), _ref(c, ROWS_A, sl=slice(10, 37), state=want))


def _sentinel(L, n=R):
    """A state no reduction leaves: keys with a pattern, count 77, sum 2.5 in rows 0 .. 2 and, in the rows the tests never name, -0.0 and
    a NaN with a payload (bits that only survive untouched)."""
    st = dict(best=np.full((n, L), 0x0123456789abcdef, np.uint64), eps_lo=np.full((n, L), 0x1111111122222222, np.uint64),
              eps_hi=np.full((n, L), 0xfedcba9876543210, np.uint64), eps_abs_sum=np.full((n, L), 2.5, np.float32), count=np.full((n, L), 77, np.int32))
    st["eps_abs_sum"][3:].view(np.uint32)[:] = 0x80000000
    st["eps_abs_sum"][5].view(np.uint32)[:] = 0x7fc01234
    return st


def _raw(engine, c, rows, state, flags, n=None, L=None, nbytes=None, **over):
    """The C entry itself on device buffers: -> its return code."""
    from thermompnn_amd.engine import _ptr, _stream
    n = len(rows) if n is None else n
    L = c["S_var"].shape[1] if L is None else L
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(c, row=np.asarray(rows, np.int32)).items()}
    ws = torch.empty(max(engine.lib.tmpnn_pair_map_workspace_bytes(n, L), 256), dtype=torch.uint8, device="cuda")
    args = dict(ddg=_ptr(t["ddg"]), ld=c["ddg"].shape[2], S=_ptr(t["S_var"]), base=_ptr(t["base"]), row=_ptr(t["row"]), letter=_ptr(t["letter"]),
                skip=_ptr(t["skip"]), wt=_ptr(t["wt"]), ld_wt=c["wt"].shape[1], V=n, L=L, R=R, flags=flags)
    args.update(over)
    rc = engine.lib.tmpnn_pair_map(*args.values(), *[_ptr(state[name]) for name in NAMES], _ptr(ws), ws.numel() if nbytes is None else nbytes, _stream())
    torch.cuda.synchronize()
    return rc


def test_continue_keeps_the_rows_no_variant_names_and_a_fresh_call_resets_everything(engine, crafted):
    c = crafted[19, 21]
    rows = np.repeat([1, 0], [17, 20]).astype(np.int32)                   # rows 2 .. 5 are not named
    sent = _sentinel(19)
    state = _state_of(sent)
    got = _run(engine, c, rows, state=state)
    assert all(got[name] is state[name] for name in NAMES)                # updated in place
    want = _ref(c, rows, state=sent)
    assert_pair_map_equal(got, want)
    for name in NAMES:
        kept, before = got[name][2:].cpu().numpy(), sent[name][2:]
        assert kept.tobytes() == before.tobytes(), name                   # every bit, the -0.0 and the NaN's payload too
        assert got[name][:2].cpu().numpy().tobytes() != sent[name][:2].tobytes(), name
    assert (got["count"][:2] >= 77).all() and (got["eps_abs_sum"][:2] >= 2.5).all()
    # the C entry without CONTINUE on the same buffers: the whole state is emptied first, the rows not named too
    state = _state_of(sent)
    assert _raw(engine, c, rows, state, flags=0) == 0
    fresh = _ref(c, rows)
    assert_pair_map_equal(state, fresh)
    assert (state["best"][2:] == -1).all() and (state["count"][2:] == 0).all() and (state["eps_abs_sum"][2:].view(torch.int32) == 0).all()
    # and with it: as Engine.pair_map on a state
    state = _state_of(sent)
    assert _raw(engine, c, rows, state, flags=4) == 0
    assert_pair_map_equal(state, want)
    # a state larger than the call's tables (R L = 6 x 70 entries against one variant's 70 table rows: one tile) is emptied whole,
    # by workgroups the launch adds for it, and nothing behind it is touched
    c70 = crafted[70, 21]
    one = {k: (v[:1] if k != "wt" else v) for k, v in c70.items()}
    sent7 = _sentinel(70, R + 1)
    big = _state_of(sent7)
    front = {name: big[name][:R] for name in NAMES}                       # [R, 70] at the front of buffers of R + 1 rows
    assert _raw(engine, one, [3], front, flags=0) == 0
    assert_pair_map_equal(front, _ref(one, np.array([3], np.int32)))
    assert (front["count"][3] > 0).any() and (front["count"][[0, 1, 2, 4, 5]] == 0).all()
    assert all(big[name][R].cpu().numpy().tobytes() == sent7[name][R].tobytes() for name in NAMES)


def test_empty_calls_reset_or_keep(engine, crafted):
    c = crafted[19, 21]
    none = {k: (v[:0] if k != "wt" else v) for k, v in c.items()}
    sent = _sentinel(19)
    # V = 0
    got = _run(engine, none, ROWS_A[:0])
    assert_pair_map_equal(got, _ref(none, ROWS_A[:0]))
    assert (got["best"] == -1).all() and (got["eps_lo"] == -1).all() and (got["eps_hi"] == -1).all() and (got["count"] == 0).all()
    assert (got["eps_abs_sum"].view(torch.int32) == 0).all()
    state = _state_of(sent)
    kept = _run(engine, none, ROWS_A[:0], state=state)
    assert all(kept[name].cpu().numpy().tobytes() == sent[name].tobytes() for name in NAMES)
    for flags, want in ((0, _ref(none, ROWS_A[:0])), (4, sent)):
        state = _state_of(sent)
        assert _raw(engine, none, ROWS_A[:0], state, flags, ddg=None, S=None, base=None, row=None, letter=None, skip=None, wt=None) == 0
        assert all(state[name].cpu().numpy().tobytes() == want[name].tobytes() for name in NAMES), flags
    # L = 0: the state is empty
    zero = dict(ddg=np.zeros((4, 0, 21), np.float32), wt=np.zeros((0, 21), np.float32), base=np.zeros(4, np.float32), S_var=np.zeros((4, 0), np.int32),
                letter=np.zeros(4, np.int32), skip=np.zeros(4, np.int32))
    rows = np.arange(4, dtype=np.int32)
    got = _run(engine, zero, rows)
    assert all(got[name].shape == (R, 0) for name in NAMES)
    again = _run(engine, zero, rows, state=got)
    assert all(again[name] is got[name] for name in NAMES)
    for flags in (0, 4):
        assert _raw(engine, zero, rows, got, flags) == 0
    # R = 0: no state row, every variant's row is out of range
    assert all(t.shape == (0, 19) for t in _run(engine, c, ROWS_A, R=0).values())


def test_longest_protein_candidates_at_both_ends(engine):
    L = 2048
    c = _draw(3, L, 5)
    S = np.full((3, L), 20, np.int32)
    S[:, [0, L - 1]] = [[3, 7], [1, 19], [0, 0]]
    c["S_var"], c["skip"] = S, np.array([-1, 0, L - 1], np.int32)
    c["ddg"][:, [0, L - 1]] = np.random.default_rng(6).standard_normal((3, 2, 21)).astype(np.float32)
    c["wt"][[0, L - 1]] = np.random.default_rng(7).standard_normal((2, 21)).astype(np.float32)
    c["base"][:] = 0.5, -0.25, 1.0
    rows = np.array([2, 2, 0], np.int32)
    dev = (torch.from_numpy(c["ddg"]).cuda(), torch.from_numpy(c["wt"]).cuda())
    # (row, q) -> candidates. Variant 0 (row 2) has both ends, variant 1 (row 2, skip 0) the far end only, variant 2 (row 0, skip 2047)
    # the near end, and none under `upper`; 18 letters each without cysteine, 19 with it
    for kw, counts in ((dict(), {(2, 0): 18, (2, L - 1): 36, (0, 0): 18, (0, L - 1): 0}),
                       (dict(upper=True, include_cys=True), {(2, 0): 19, (2, L - 1): 38, (0, 0): 0, (0, L - 1): 0})):
        got, want = _run(engine, c, rows, R=3, dev=dev, **kw), _ref(c, rows, R=3, **kw)
        assert_pair_map_equal(got, want)
        assert (want["count"][:, 1:L - 1] == 0).all() and (want["count"][1] == 0).all()
        assert {at: int(want["count"][at]) for at in counts} == counts
        d = decode_reference(want)
        assert np.isfinite(d["best_ddG"][2, [0, L - 1]]).all() and d["best_a"][2, 0] == c["letter"][0] and d["eps_max_a"][2, 0] == c["letter"][0]


def test_error_codes_of_the_c_entry(engine, crafted):
    c = crafted[19, 21]
    sent = _sentinel(19)
    state = _state_of(sent)
    lib = engine.lib
    full = lib.tmpnn_pair_map_workspace_bytes(V, 19)
    assert full >= V * 19 * 32 + 256

    def untouched():
        return all(state[name].cpu().numpy().tobytes() == sent[name].tobytes() for name in NAMES)

    assert _raw(engine, c, ROWS_A, state, 0, nbytes=full - 257) == -4 and b"workspace" in lib.tmpnn_last_error() and untouched()   # one byte short
    assert _raw(engine, c, ROWS_A, state, 0, ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 0, ld_wt=3) == -1 and b"ld_wt=3" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 8) == -1 and b"flag" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 0, V=-1) == -1 and _raw(engine, c, ROWS_A, state, 0, R=-1) == -1 and b"sizes" in lib.tmpnn_last_error()
    for name in ("ddg", "S", "base", "row", "letter", "skip", "wt"):
        assert _raw(engine, c, ROWS_A, state, 0, **{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert _raw(engine, c, ROWS_A, dict(state, count=None), 4) == -1 and b"null" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 0, L=2049) == -2 and b"2048" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 0, V=(1 << 31) // 19 + 1) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert _raw(engine, c, ROWS_A, state, 0, R=(1 << 31) // 19 + 1) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert untouched()                                                    # every error came before a launch
    assert _raw(engine, c, ROWS_A, state, 0, nbytes=full - 256) == 0      # the aligned buffer needs none of the slack
    assert_pair_map_equal(state, _ref(c, ROWS_A))


# ---- end to end: a model, the front end, the command line --------------------------------------------------------------------
def test_double_mutant_map_equals_reductions_of_the_tables(tmp_path, monkeypatch):
    import masked_backbones as mb
    from thermompnn_amd import variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.pdb_io import alt_parse_PDB
    model = load_model(None, None, 0)
    path = mb.write_layout("msk_L40", tmp_path)
    pdb = alt_parse_PDB(path, "A")
    seq = pdb[0]["seq"]
    assert "-" in seq and len(seq) == 40
    wt_idx = variant_scan.sequence_indices(seq)
    positions = [p for p in range(40) if wt_idx[p] < 20]
    P, L = len(positions), 40
    dev = "cuda:0"
    with torch.no_grad():
        dm = variant_scan.double_mutant_table(model, pdb, positions=positions)                     # [P, 20, L, 20]
        _, S_bg = variant_scan.single_backgrounds(seq, positions)
        S_bg = S_bg.reshape(P * 20, L)
        t_bg = torch.cat([model.variant_tables(pdb, S_bg[v0:v0 + 256]) for v0 in range(0, P * 20, 256)]).view(P, 20, L, 21)[..., :20]
        wt = model.variant_tables(pdb, [seq])[0]
    e = t_bg - wt[None, None, :, :20]                                     # fp32: one subtract
    assert not torch.isnan(dm).any() and not torch.isnan(e).any()
    w = torch.as_tensor(wt_idx, device=dev)
    a, b = torch.arange(20, device=dev)[None, :, None, None], torch.arange(20, device=dev)[None, None, None, :]
    p, q = torch.as_tensor(positions, device=dev)[:, None, None, None], torch.arange(L, device=dev)[None, None, :, None]
    flat = lambda x: x.permute(0, 2, 1, 3).reshape(P, L, 400)             # [P, L, (a, b)]
    eng = model.engine()
    calls, encode = [], eng.encode
    monkeypatch.setattr(eng, "encode", lambda *args, **kw: (calls.append(1), encode(*args, **kw))[1])
    maps = {}
    for unordered, cys in ((False, False), (True, True)):
        del calls[:]
        with torch.no_grad():
            m = model.double_mutant_map(pdb, unordered=unordered, include_cys=cys, chunk=100)
        assert len(calls) == 1                                            # the encoder ran once for all the chunks
        maps[unordered] = m
        ok = (a != w[positions][:, None, None, None]) & (b != w[None, None, :, None]) & (w[None, None, :, None] < 20)
        ok = ok & ((q > p) if unordered else (q != p))
        if not cys:
            ok = ok & (a != 1) & (b != 1)
        ok_f = flat(ok.expand(P, 20, L, 20))
        count = ok_f.sum(2)
        none = (count == 0).cpu().numpy()
        np.testing.assert_array_equal(m.count, count.cpu().numpy())
        assert (~none).sum() == (P * (P - 1) // 2 if unordered else P * (P - 1))
        for name, x, sign in (("best_ddG", dm, 1.0), ("eps_min", e, 1.0), ("eps_max", e, -1.0)):
            masked = torch.where(ok_f, flat(x) * sign + 0.0, torch.full_like(flat(x), INF))
            val = masked.amin(2)
            first = (masked == val[:, :, None]).to(torch.int32).argmax(2)                        # the FIRST minimum in (a, b) order
            val = (val * sign + 0.0).cpu().numpy()
            stem = "best" if name == "best_ddG" else name
            got = getattr(m, name)
            np.testing.assert_array_equal(got.view(np.uint32)[~none], val.view(np.uint32)[~none], err_msg=name)     # the bits
            assert np.isnan(got[none]).all()
            np.testing.assert_array_equal(getattr(m, stem + "_a"), np.where(none, -1, (first // 20).cpu().numpy()), err_msg=name)
            np.testing.assert_array_equal(getattr(m, stem + "_b"), np.where(none, -1, (first % 20).cpu().numpy()), err_msg=name)
        mean64 = (torch.where(ok_f, flat(e).abs().double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(2) / count.clamp(min=1)).cpu().numpy()
        np.testing.assert_allclose(m.eps_abs_mean[~none], mean64[~none], rtol=1e-6)
        assert np.isnan(m.eps_abs_mean[none]).all() and m.positions.tolist() == positions and m.seq == seq
        np.testing.assert_array_equal(m.wt, wt.cpu().numpy())
    # the chunk size does not show, and the options reach the reduction
    with torch.no_grad():
        other = model.double_mutant_map(pdb, unordered=True, include_cys=True, chunk=37, positions=positions[3:9])
    for name in variant_scan.PairMap.ARRAYS[1:-1]:
        assert getattr(other, name).tobytes() == getattr(maps[True], name)[3:9].tobytes(), name
    # the command line writes the front end's arrays
    monkeypatch.undo()
    out = str(tmp_path / "map.npz")
    assert variant_scan.main([path, "--chain", "A", "--pair-map", "--unordered", "--include_cys", "--chunk", "100", "--out", out,
                              "--synthetic_weights", "0"]) == 0
    z = np.load(out)
    assert str(z["seq"]) == seq
    for name in variant_scan.PairMap.ARRAYS:
        x = getattr(maps[True], name)
        assert z[name].dtype == x.dtype and z[name].tobytes() == x.tobytes(), name
