"""Double-mutant hit lists, the parts that need no GPU: the numpy restatement of tmpnn_select_variant_hits against a brute-force loop
on tie-dominated inputs (with a state carried over several calls), the low word's pack and unpack at the ends of its fields, the
front end's chunk loop, CSV and command line through stub table and selection functions, and the argument errors and sizer zeros of
the two C entries (before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pair_hits_restatement import (MAX_LEN, MAX_TAG, NONE, assert_variant_hits_equal, ord32, pack_low, unord32, unpack_low,
                                   variant_hits_reference)

NAN, INF = float("nan"), float("inf")
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
POOL = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, NAN, INF, -INF], np.float32)    # ties dominate; a denormal; 1 and 1 + ulp


def _brute(ddg, S_var, base, tag, skip, k, cutoff, include_cys, upper, carried):
    """The contract read aloud: a Python loop over (v, q, b), np.float32 sums, a Python sort of (value, tag, q, b) tuples. ``carried``:
    the tuples earlier calls kept. -> (the restatement's dict without its state, the tuples kept)."""
    cut = None if cutoff is None else float(np.float32(cutoff))
    cands = list(carried)
    V, L = S_var.shape
    for v in range(V):
        if not 0 <= tag[v] <= MAX_TAG:
            continue
        for q in range(L):
            s = int(S_var[v, q])
            if not 0 <= s < 20 or (q <= skip[v] if upper else q == skip[v]):
                continue
            for b in range(20):
                with np.errstate(invalid="ignore"):
                    val = float(np.float32(base[v]) + np.float32(ddg[v, q, b]))
                if b == s or (b == 1 and not include_cys) or math.isnan(val) or (cut is not None and not val <= cut):
                    continue
                cands.append((val + 0.0, int(tag[v]), q, b))
    cands.sort()
    kept = cands[:k]
    out = dict(hit_ddg=np.full(k, np.nan, np.float32), hit_tag=np.full(k, -1, np.int32), hit_pos=np.full(k, -1, np.int32),
               hit_aa=np.full(k, -1, np.int32), hit_count=np.array([len(kept)], np.int32))
    for r, (val, t, q, b) in enumerate(kept):
        out["hit_ddg"][r], out["hit_tag"][r], out["hit_pos"][r], out["hit_aa"][r] = val, t, q, b
    return out, kept


def _crafted(V, L, seed, ld=21):
    rng = np.random.default_rng(seed)
    ddg = POOL[rng.integers(0, len(POOL), size=(V, L, ld))]
    base = POOL[rng.integers(0, len(POOL), size=V)]
    S_var = rng.integers(-1, 22, size=(V, L)).astype(np.int32)
    tag = rng.permutation(200)[:V].astype(np.int32)
    skip = rng.integers(-1, L, size=V).astype(np.int32)
    return ddg, S_var, base, tag, skip


def test_restatement_equals_a_brute_force_loop_over_three_calls():
    ddg, S_var, base, tag, skip = _crafted(9, 6, 0)
    tag[0], tag[1], tag[2], tag[3] = 0, MAX_TAG, MAX_TAG + 1, -1         # the ends of the field, and one beyond each
    base[4] = NAN                                                        # contributes nothing
    cuts = (None, 0.0, -0.0, 1.0, ONE_UP, -INF, 2e-40)
    for k in (1, 5, 64):
        for cutoff in cuts:
            for cys in (False, True):
                for upper in (False, True):
                    state, kept = None, []
                    for v0, v1 in ((0, 4), (4, 5), (5, 9)):
                        sl = slice(v0, v1)
                        got = variant_hits_reference(ddg[sl], S_var[sl], base[sl], tag[sl], skip[sl], k, cutoff, cys, upper, state)
                        want, kept = _brute(ddg[sl], S_var[sl], base[sl], tag[sl], skip[sl], k, cutoff, cys, upper, kept)
                        state = got.pop("state")
                        n = int(got["hit_count"][0])
                        assert (state[n:] == NONE).all() and (np.diff(state[:n].astype(object)) > 0).all()
                        assert_variant_hits_equal({**got, "state": state}, {**want, "state": state})
                    whole = variant_hits_reference(ddg, S_var, base, tag, skip, k, cutoff, cys, upper)
                    assert_variant_hits_equal({**got, "state": state}, whole)       # the cut into calls does not show
    full = variant_hits_reference(ddg, S_var, base, tag, skip, 64)
    n = int(full["hit_count"][0])
    assert 0 < n and not np.isin(full["hit_tag"][:n], [MAX_TAG + 1, -1, tag[4]]).any() and (full["hit_aa"][:n] != 1).all()
    assert np.isin(full["hit_tag"][:n], [0, MAX_TAG]).any()


def test_low_word_pack_and_unpack_at_the_ends_of_every_field():
    seen = set()
    for tag in (0, MAX_TAG):
        for q in (0, MAX_LEN - 1):
            for b in (0, 19):
                lo = pack_low(tag, q, b)
                assert int(lo) == tag * 65536 + q * 32 + b < 2 ** 32
                assert tuple(int(x) for x in unpack_low(lo)) == (tag, q, b)
                seen.add(int(lo))
    assert len(seen) == 8 and max(seen) == 0xfffffff3 and min(seen) == 0
    # the double mutants' tag: p * 32 + a fills the 16 bits exactly at L = 2048
    from thermompnn_amd.variant_scan import PAIR_MAX_LEN, pair_tag, split_tag
    assert PAIR_MAX_LEN == MAX_LEN and pair_tag(MAX_LEN - 1, 19) <= MAX_TAG < pair_tag(MAX_LEN, 0)
    assert split_tag(pair_tag(2047, 19)) == (2047, 19) and split_tag(pair_tag(0, 0)) == (0, 0)
    # ascending keys are ascending (value, tag, position, letter); the order word and its inverse
    bits = np.array([0xff800000, 0xbf800000, 0x80000001, 0x80000000, 0, 1, 0x3f800000, 0x3f800001, 0x7f800000], np.uint32)
    o = ord32(bits)
    assert (np.diff(o.astype(np.int64)) >= 0).all() and o[3] == o[4]
    back = unord32(o)
    assert back[3] == 0 and (np.delete(back, 3) == np.delete(bits, 3)).all()
    assert ord32(np.array([0x7fc00000], np.uint32))[0] > o[-1]               # a NaN's word lies above +inf's: all ones is free


# ---- the front end on stub tables -----------------------------------------------------------------------------------------------
STUB_POOL = np.array([-2.0, -1.25, -0.5, 0.0, 0.125, 0.75, 1e-40, ONE_UP], np.float32)


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


class StubSelect:
    """Engine.select_variant_hits on the host: the restatement, call by call."""
    def __init__(self):
        self.chunks = []

    def __call__(self, ddg, S_var, base, tag, k, skip=None, cutoff=None, include_cys=False, upper=False, state=None):
        self.chunks.append(int(ddg.shape[0]))
        old = None if state is None else state.numpy().view(np.uint64)
        r = variant_hits_reference(ddg.numpy(), S_var, base.numpy(), tag, skip, k, cutoff, include_cys, upper, old)
        return {key: torch.from_numpy(v.view(np.int64) if key == "state" else v) for key, v in r.items()}


def _brute_pairs(seq, k, cutoff=None, include_cys=False, unordered=False, positions=None):
    from thermompnn_amd.variant_scan import sequence_indices
    wt_idx = sequence_indices(seq)
    wt = stub_tables(wt_idx[None])[0].numpy()
    rows = []
    for p in (range(len(seq)) if positions is None else positions):
        for a in range(20):
            if wt_idx[p] >= 20 or a == wt_idx[p] or (a == 1 and not include_cys):
                continue
            S = wt_idx.copy()
            S[p] = a
            t = stub_tables(S[None])[0].numpy()
            for q in range(len(seq)):
                for b in range(20):
                    if q == p or (unordered and q < p) or S[q] >= 20 or b == S[q] or (b == 1 and not include_cys):
                        continue
                    val = float(np.float32(wt[p, a]) + np.float32(t[q, b]))
                    if cutoff is None or val <= float(np.float32(cutoff)):
                        rows.append((val + 0.0, p, a, q, b, float(wt[p, a]), float(wt[p, a]) + float(wt[q, b])))
    rows.sort()
    return rows[:k]


SEQ = "MKC-AXGWCYLE"


def _assert_hits_are(hits, rows, seq):
    from thermompnn_amd.datasets import ALPHABET
    assert len(hits) == len(rows)
    for h, (val, p, a, q, b, first, add) in zip(hits, rows):
        assert (h.first.position, h.first.wildtype, h.first.mutation) == (p, seq[p], ALPHABET[a])
        assert (h.second.position, h.second.wildtype, h.second.mutation) == (q, seq[q], ALPHABET[b])
        assert h.ddG == val and h.ddG_first == first == h.first.ddG and h.ddG_additive == add and h.epistasis == val - add


def test_front_end_chunk_loop_on_stub_tables():
    from thermompnn_amd.variant_scan import double_mutant_hits
    pdb = [{"seq": SEQ, "name": "stub"}]
    for kw in (dict(), dict(unordered=True), dict(include_cys=True, cutoff=-1.0), dict(positions=[0, 4, 11], cutoff=0.0)):
        for k in (1, 40):
            want = _brute_pairs(SEQ, k, **kw)
            assert want
            for chunk in (1, 7, 1000):
                sel = StubSelect()
                hits = double_mutant_hits(None, pdb, k, chunk=chunk, _tables=stub_tables, _select=sel, **kw)
                _assert_hits_are(hits, want, SEQ)
                n_bg = sum(sel.chunks)
                assert max(sel.chunks) <= chunk and len(sel.chunks) == -(-n_bg // chunk)
            per_site = 19 if kw.get("include_cys") else 18
            sites = kw.get("positions", [p for p, c in enumerate(SEQ) if c not in "-X"])
            assert n_bg == sum(per_site + (1 if SEQ[p] == "C" and not kw.get("include_cys") else 0) for p in sites)
    assert all(h.first.pdb == "stub" and h.second.ddG is None for h in hits)
    assert double_mutant_hits(None, pdb, 5, cutoff=-100.0, _tables=stub_tables, _select=StubSelect()) == []
    assert double_mutant_hits(None, pdb, 5, positions=[], _tables=stub_tables, _select=StubSelect()) == []
    for bad, word in ((dict(k=0), "k=0"), (dict(k=257), "k=257"), (dict(k=3, positions=[3]), "position 3"), (dict(k=3, positions=[5]), "position 5"),
                      (dict(k=3, positions=[12]), "position 12"), (dict(k=3, chunk=0), "chunk")):
        with pytest.raises(ValueError, match=word):
            double_mutant_hits(None, pdb, _tables=stub_tables, _select=StubSelect(), **bad)
    with pytest.raises(ValueError, match="2048"):
        double_mutant_hits(None, [{"seq": "A" * 2049}], 3, _tables=stub_tables, _select=StubSelect())


def test_command_line_parses_and_writes_the_csv_columns(tmp_path, capsys):
    from thermompnn_amd import variant_scan
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    X, seq = synthetic_backbone(14, 5)
    path = tmp_path / "tiny.pdb"
    path.write_text(backbone_pdb_text(X, seq))
    pdb = alt_parse_PDB(str(path), "A")
    assert pdb[0]["seq"] == seq
    out = tmp_path / "pairs.csv"
    argv = [str(path), "--chain", "A", "--top-pairs", "9", "--cutoff", "0.5", "--unordered", "--include_cys", "--chunk", "50", "--out", str(out)]
    assert variant_scan.main(argv, _tables=stub_tables, _select=StubSelect()) == 0
    assert "9 double mutants" in capsys.readouterr().out
    hits = variant_scan.double_mutant_hits(None, pdb, 9, cutoff=0.5, unordered=True, include_cys=True, _tables=stub_tables, _select=StubSelect())
    _assert_hits_are(hits, _brute_pairs(seq, 9, cutoff=0.5, unordered=True, include_cys=True), seq)
    lines = out.read_text().split("\n")
    assert lines[0] == "rank,first,second,ddG,ddG_first,ddG_additive,epistasis" and lines[-1] == "" and len(lines) == 11
    for r, (line, h) in enumerate(zip(lines[1:], hits)):
        f = line.split(",")
        assert f[0] == str(r)
        assert f[1] == f"{seq[h.first.position]}{h.first.position + 1}{h.first.mutation}"          # A12G: 1-based
        assert f[2] == f"{seq[h.second.position]}{h.second.position + 1}{h.second.mutation}"
        assert [float(x) for x in f[3:]] == [h.ddG, h.ddG_first, h.ddG_additive, h.epistasis]
        assert variant_scan.parse_variant_line(f[1] + "," + f[2]) == [variant_scan.Mutation(h.first.position, h.first.wildtype, h.first.mutation),
                                                                     variant_scan.Mutation(h.second.position, h.second.wildtype, h.second.mutation)]
    # --top-pairs is a third member of the exclusive group, and its options are its own
    base = [str(path), "--out", str(out), "--synthetic_weights", "0"]
    for bad, word in ((["--top-pairs", "5", "--all-singles"], "not allowed with"), (["--top-pairs", "5", "--variants", "v.txt"], "not allowed with"),
                      (["--top-pairs", "0"], "top-pairs"), (["--top-pairs", "257"], "top-pairs"), (["--all-singles", "--cutoff", "1"], "top-pairs"),
                      (["--all-singles", "--unordered"], "top-pairs"), (["--all-singles", "--include_cys"], "top-pairs"), ([], "required")):
        with pytest.raises(SystemExit):
            variant_scan.main(base + bad, _tables=stub_tables, _select=StubSelect())
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        variant_scan.main([str(path), "--out", "x.npz", "--top-pairs", "5"], _tables=stub_tables, _select=StubSelect())
    assert "CSV" in capsys.readouterr().err


def test_argument_errors_and_sizer_zeros_need_no_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    size = lib.tmpnn_variant_hits_workspace_bytes
    assert size(10, 100, 0) == 0 and size(10, 100, 257) == 0 and size(-1, 100, 8) == 0 and size(10, -1, 8) == 0
    assert size(10, 2049, 8) == 0 and size((1 << 31) // 2048 + 1, 2048, 8) == 0 and size(1 << 31, 1, 8) == 0
    assert size((1 << 31) // 2048 - 1, 2048, 8) > 0 and size(10, 2048, 256) >= 31 * 256 * 8
    assert size(10, 100, 8) >= 10 * 8 * 8 and size(300, 20, 32) >= 255 * 32 * 8 and size(40, 257, 256) >= 31 * 256 * 8
    assert size(0, 100, 8) > 0 and size(10, 0, 8) > 0                     # the merge alone
    d = C.c_void_p(256)                                                   # never dereferenced: every call below fails before a launch

    def call(ddg=d, ld=21, S=d, base=d, tag=d, skip=d, V=4, L=100, k=8, cutoff=INF, flags=0, state=d, o1=d, o2=d, o3=d, o4=d, o5=d, ws=d,
             nbytes=1 << 20):
        return lib.tmpnn_select_variant_hits(ddg, ld, S, base, tag, skip, V, L, k, cutoff, flags, state, o1, o2, o3, o4, o5, ws, nbytes, None)

    for name in ("ddg", "S", "base", "tag", "skip", "state", "o1", "o2", "o3", "o4", "o5", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(k=0) == -1 and b"k=0" in lib.tmpnn_last_error()
    assert call(k=257) == -1 and b"k=257" in lib.tmpnn_last_error()
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert call(V=-1) == -1 and b"sizes" in lib.tmpnn_last_error() and call(L=-1) == -1
    assert call(flags=8) == -1 and b"flag" in lib.tmpnn_last_error() and call(flags=-1) == -1
    assert call(cutoff=NAN) == -1 and b"NaN" in lib.tmpnn_last_error()
    assert call(L=2049) == -2 and b"2048" in lib.tmpnn_last_error()       # TMPNN_E_UNSUPPORTED
    assert call(V=(1 << 31) // 2048 + 1, L=2048) == -2 and b"2^31" in lib.tmpnn_last_error()
    assert call(nbytes=64) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert call(V=0, state=None) == -1 and call(L=0, o5=None) == -1       # the merge alone still needs its state and outputs
    assert (_lib.VHITS_INCLUDE_CYS, _lib.VHITS_UPPER, _lib.VHITS_CONTINUE, _lib.VHITS_MAX_LEN, _lib.VHITS_MAX_TAG) == (1, 2, 4, MAX_LEN, MAX_TAG)
