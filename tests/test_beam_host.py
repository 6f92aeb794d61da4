"""The beam step and the multi-mutant search, the parts that need no GPU: the numpy restatement of tmpnn_beam_step against a brute-force
loop on tie-dominated inputs, the duplicate fixture's own conditions (checked on the reference alone: they are what keeps the GPU test
from passing without ever meeting a duplicate), the front end's rounds, CSV and command line through stub table and step functions, and
the argument errors and sizer zeros of the two C entries (before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from beam_restatement import (CYS, MAX_DEPTH, MAX_KD, MAX_LEN, MAX_V, assert_beam_equal, beam_step_reference, child_set, duplicate_fixture,
                              ordered_candidates, pack_sub)
from test_pair_hits_host import POOL, SEQ, stub_tables

NAN, INF = float("nan"), float("inf")
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))


def _brute(ddg, S_var, score, muts, depth, k, allowed, cutoff, include_cys):
    """The contract read aloud: a Python loop over (v, q, b), np.float32 sums, a Python sort of (value, v, q, b) tuples, a walk that
    keeps a candidate when its sorted tuple of substitutions is new."""
    cut = None if cutoff is None else float(np.float32(cutoff))
    V, L = S_var.shape
    cands = []
    for v in range(V):
        own = [] if depth == 1 else [int(e) for e in muts[v]]
        if any(e < 0 for e in own) or math.isnan(float(score[v])):
            continue
        for q in range(L):
            s = int(S_var[v, q])
            if not 0 <= s < 20 or q in [e >> 5 for e in own] or (allowed is not None and not allowed[q]):
                continue
            for b in range(20):
                with np.errstate(invalid="ignore"):
                    val = float(np.float32(score[v]) + np.float32(ddg[v, q, b]))
                if b == s or (b == CYS and not include_cys) or math.isnan(val) or (cut is not None and not val <= cut):
                    continue
                cands.append((val + 0.0, v, q, b))
    cands.sort()
    out = dict(out_muts=np.full((k, depth), -1, np.int32), out_score=np.full(k, np.nan, np.float32), out_parent=np.full(k, -1, np.int32),
               out_S=np.full((k, L), 20, np.int32), out_count=np.zeros(1, np.int32))
    seen, n = [], 0
    for val, v, q, b in cands:
        if n == k:
            break
        cs = sorted(([] if depth == 1 else [int(e) for e in muts[v]]) + [q * 32 + b])
        if cs in seen:
            continue
        seen.append(cs)
        out["out_muts"][n], out["out_score"][n], out["out_parent"][n] = cs, val, v
        out["out_S"][n] = S_var[v]
        out["out_S"][n, q] = b
        n += 1
    out["out_count"][0] = n
    return out


def _crafted(V, L, depth, seed, ld=21):
    """Members that share substitutions, so that children coincide: every member's substitutions are drawn from three sites."""
    rng = np.random.default_rng(seed)
    ddg = POOL[rng.integers(0, len(POOL), size=(V, L, ld))]
    score = POOL[rng.integers(0, len(POOL), size=V)]
    S_var = rng.integers(-1, 22, size=(V, L)).astype(np.int32)
    muts = np.zeros((V, depth - 1), np.int32)
    seen = set()
    for v in range(V):
        while True:
            pos = np.sort(rng.choice(min(L, depth + 1), size=depth - 1, replace=False))
            let = rng.integers(2, 5, size=depth - 1)
            if depth == 1 or tuple(pack_sub(pos, let)) not in seen:
                break
        seen.add(tuple(pack_sub(pos, let)))
        muts[v] = pack_sub(pos, let)
        S_var[v, pos] = let
    return ddg, S_var, score, (muts if depth > 1 else None)


def test_restatement_equals_a_brute_force_loop():
    below = float(np.nextafter(np.float32(1.25), np.float32(0)))           # one ulp under the sum 1 + 0.25
    dups = 0
    for depth, V in ((1, 1), (2, 7), (3, 9)):
        ddg, S_var, score, muts = _crafted(V, 6, depth, depth)
        if depth > 1:
            muts[1, 0] = -1                                                # a dead member
            score[2] = NAN                                                 # contributes nothing
            score[0], score[3] = 1.0, 0.25
        else:
            score[0] = 1.0
        allowed = np.array([1, 1, 0, 1, 7, -1], np.int32)
        for k in (1, 5, 64):
            if k * depth > MAX_KD:
                continue
            for cutoff in (None, 0.0, -0.0, 1.25, below, -INF, 2e-40):
                for cys in (False, True):
                    for al in (None, allowed):
                        got = beam_step_reference(ddg, S_var, score, muts, depth, k, al, cutoff, cys)
                        assert_beam_equal(got, _brute(ddg, S_var, score, muts, depth, k, al, cutoff, cys))
                        dups += got["dropped"]
                        n = int(got["out_count"][0])
                        assert (got["out_S"][n:] == 20).all() and (got["out_muts"][n:] == -1).all() and np.isnan(got["out_score"][n:]).all()
                        assert len({tuple(r) for r in got["out_muts"][:n].tolist()}) == n
                        if al is not None and depth == 1:
                            assert not np.isin(got["out_muts"][:n, 0] >> 5, [2]).any()
        # few enough candidates (one row with a letter, finite entries) for the cutoff to show: it parts exactly at the sum 1 + 0.25
        tame = np.where(np.isfinite(ddg), ddg, np.float32(0.25))
        rows = np.full_like(S_var, 20)
        rows[:, 5] = 7
        at = beam_step_reference(tame, rows, score, muts, depth, 200, None, 1.25, True)
        under = beam_step_reference(tame, rows, score, muts, depth, 200, None, below, True)
        assert_beam_equal(at, _brute(tame, rows, score, muts, depth, 200, None, 1.25, True))
        assert_beam_equal(under, _brute(tame, rows, score, muts, depth, 200, None, below, True))
        n_at, n_under = int(at["out_count"][0]), int(under["out_count"][0])
        assert n_under < n_at < 200 and at["out_score"][n_at - 1] == np.float32(1.25) and under["out_score"][n_under - 1] < np.float32(1.25)
    assert dups > 0                                                      # the walk did pass over duplicates


def _fixture_conditions(fx, k):
    d = fx["depth"]
    ref = beam_step_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], d, k)
    o, v, q, b = ordered_candidates(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], d)
    first = [child_set(fx["muts"], d, v[i], q[i], b[i]) for i in range(min(k * d, len(o)))]
    most = max(first.count(cs) for cs in set(first))
    return ref, most


def test_duplicate_fixture_meets_its_conditions_on_the_reference_alone():
    """d = 3, V = 37: the fifteen pairs of a pool of six substitutions and 22 unrelated members. For every k of the GPU test some child
    set occurs d = 3 times within the first k d keys and count == k; for k >= 2 the walk drops at least k / 4 duplicates before the
    k-th kept entry. (For k = 1 nothing precedes the first kept entry, so no walk can drop anything there: the first condition stands
    in for it, the three smallest keys are three paths to ONE set.)"""
    for L in (300, 40):
        fx = duplicate_fixture(3, 37, L, 5)
        assert fx["muts"].shape == (37, 2) and (fx["muts"][36] < 0).any() and np.isnan(fx["score"][35])
        assert (fx["S_var"] < 0).any() and (fx["S_var"] >= 20).any() and not np.isneginf(fx["ddg"]).any()
        for k in (1, 5, 32, 85):
            ref, most = _fixture_conditions(fx, k)
            assert most == 3, (k, most)
            assert int(ref["out_count"][0]) == k
            if k >= 2:
                assert ref["dropped"] >= k / 4, (k, ref["dropped"])
            n_pool_children = sum(set(r) <= fx["pool"] for r in ref["out_muts"].tolist())
            assert n_pool_children == min(k, 20)                           # the pool's 20 triples come first
        ref, _ = _fixture_conditions(fx, 85)
        assert ref["dropped"] == 40                                        # each triple has three parents: two of its paths are dropped
    # the pool's entries are the bottom of the finite range of their members' tables
    fx = duplicate_fixture(3, 37, 300, 5)
    for v in range(15):
        t = fx["ddg"][v, :, :20]
        low = np.sort(t[np.isfinite(t)])[:4]
        assert (low <= -2.7).all() and (np.sort(t[np.isfinite(t)])[4] >= 0)
    # a short case: fewer distinct children than k
    short = duplicate_fixture(3, 16, 8, 6)
    allowed = np.zeros(8, np.int32)
    allowed[[0, 7]] = 1
    ref = beam_step_reference(short["ddg"], short["S_var"], short["score"], short["muts"], 3, 85, None, -8.5)
    assert int(ref["out_count"][0]) == 20 and ref["dropped"] == 40 and ref["walked"] == 60       # the pool's triples alone pass the cutoff
    ref = beam_step_reference(short["ddg"], short["S_var"], short["score"], short["muts"], 3, 85, allowed, -8.5)
    n = int(ref["out_count"][0])
    assert 0 < n < 20 and ref["dropped"] > 0 and ref["walked"] == len(ordered_candidates(short["ddg"], short["S_var"], short["score"],
                                                                                          short["muts"], 3, allowed, -8.5)[0])
    # the other depths of the GPU test carry duplicates too
    for d, V, L, k, n_pool in ((8, 37, 40, 32, 9), (2, 12, 40, 128, 6), (2, 3, 2048, 64, 3), (3, 20, 19, 32, 6), (2, 256, 40, 64, 6)):
        fx = duplicate_fixture(d, V, L, 7, n_pool=n_pool)
        ref, most = _fixture_conditions(fx, k)
        assert most == d and ref["dropped"] >= d - 1, (d, most, ref["dropped"])


# ---- the front end on stub tables ------------------------------------------------------------------------------------------------
class StubStep:
    """Engine.beam_step on the host: the restatement, round by round."""
    def __init__(self):
        self.members = []

    def __call__(self, ddg, S_var, score, muts, depth, k, allowed=None, cutoff=None, include_cys=False):
        self.members.append(int(ddg.shape[0]))
        r = beam_step_reference(ddg.numpy(), np.asarray(S_var), np.asarray(score), None if muts is None else np.asarray(muts), depth, k,
                                allowed, cutoff, include_cys)
        return {key: torch.from_numpy(np.asarray(r[key])) for key in ("out_muts", "out_score", "out_parent", "out_S", "out_count")}


def _brute_search(seq, order, beam, positions=None, cutoff=None, include_cys=False):
    """A beam search written out: members are (value, dict position -> letter, parent rank); every round lists every child of every
    member with np.float32 sums, sorts by (value, parent rank, q, b), and keeps the first ``beam`` new sets."""
    from thermompnn_amd.variant_scan import sequence_indices
    wt_idx = sequence_indices(seq)
    wt = stub_tables(wt_idx[None])[0].numpy()
    members, levels = [(np.float32(0.0), {})], []
    for _ in range(order):
        rows = []
        for rank, (val, subs) in enumerate(members):
            S = wt_idx.copy()
            for p, a in subs.items():
                S[p] = a
            t = stub_tables(S[None])[0].numpy()
            for q in range(len(seq)):
                for b in range(20):
                    if q in subs or S[q] >= 20 or b == S[q] or (b == 1 and not include_cys) or (positions is not None and q not in positions):
                        continue
                    new = np.float32(val) + np.float32(t[q, b])
                    if cutoff is None or float(new) <= float(np.float32(cutoff)):
                        rows.append((float(new) + 0.0, rank, q, b))
        rows.sort()
        kept, seen = [], []
        for val, rank, q, b in rows:
            subs = dict(members[rank][1])
            subs[q] = b
            if subs in seen or len(kept) == beam:
                continue
            seen.append(subs)
            kept.append((val, subs, rank))
        levels.append([(val, sorted(subs.items()), rank, sum(float(wt[p, a]) for p, a in sorted(subs.items()))) for val, subs, rank in kept])
        members = [(np.float32(val), subs) for val, subs, _ in kept]
    return levels


def _assert_levels_are(levels, want, seq):
    from thermompnn_amd.datasets import ALPHABET
    assert len(levels) == len(want)
    for hits, rows in zip(levels, want):
        assert len(hits) == len(rows)
        for h, (val, subs, rank, add) in zip(hits, rows):
            assert [(m.position, m.wildtype, m.mutation) for m in h.mutations] == [(p, seq[p], ALPHABET[a]) for p, a in subs]
            assert h.ddG == val and h.parent == rank and h.ddG_additive == add and h.epistasis == val - add
            assert isinstance(h.mutations, tuple)


def test_front_end_rounds_on_stub_tables():
    from thermompnn_amd.variant_scan import multi_mutant_search
    pdb = [{"seq": SEQ, "name": "stub"}]
    for kw in (dict(), dict(include_cys=True, cutoff=-1.0), dict(positions=[0, 4, 11]), dict(positions=[11, 2, 6, 9], cutoff=-0.5)):
        for order, beam in ((1, 7), (3, 5), (4, 40)):
            step = StubStep()
            levels = multi_mutant_search(None, pdb, order, beam, _tables=stub_tables, _step=step, **kw)
            want = _brute_search(SEQ, order, beam, **kw)
            assert want[0]
            _assert_levels_are(levels, want, SEQ)
            assert step.members[0] == 1 and all(m <= beam for m in step.members) and len(step.members) <= order
    assert all(m.pdb == "stub" for h in levels[1] for m in h.mutations) and all(len(h.mutations) == 4 for h in levels[3])
    # with a beam that holds every candidate, level 2 is the exhaustive minimum over both orders of every pair
    sites = [0, 4, 11]
    levels = multi_mutant_search(None, pdb, 2, 128, positions=sites, _tables=stub_tables, _step=StubStep())
    assert len(levels[0]) == 54 < 128                                      # 3 sites x 18 letters: the whole first level
    from thermompnn_amd.variant_scan import sequence_indices
    wt_idx = sequence_indices(SEQ)
    wt = stub_tables(wt_idx[None])[0].numpy()
    best = {}
    for p in sites:
        for a in range(20):
            if a == wt_idx[p] or a == 1:
                continue
            S = wt_idx.copy()
            S[p] = a
            t = stub_tables(S[None])[0].numpy()
            for q in sites:
                for b in range(20):
                    if q == p or b == wt_idx[q] or b == 1:
                        continue
                    key = tuple(sorted(((p, a), (q, b))))
                    val = float(np.float32(wt[p, a]) + np.float32(t[q, b])) + 0.0
                    best[key] = min(best.get(key, INF), val)
    want = sorted(best.values())[:128]
    assert len(best) == 3 * 18 * 18 and [h.ddG for h in levels[1]] == want
    for h in levels[1]:
        assert best[tuple((m.position, "ACDEFGHIKLMNPQRSTVWYX".index(m.mutation)) for m in h.mutations)] == h.ddG
        assert h.epistasis == h.ddG - h.ddG_additive and h.ddG_additive == sum(float(m.ddG) for m in h.mutations)
    # a cutoff that empties the beam leaves the later levels empty
    cut = float(sorted(h.ddG for h in levels[0])[0])
    gone = multi_mutant_search(None, pdb, 4, 8, cutoff=-100.0, _tables=stub_tables, _step=StubStep())
    assert gone == [[], [], [], []]
    step = StubStep()
    part = multi_mutant_search(None, pdb, 3, 8, positions=sites, cutoff=cut, _tables=stub_tables, _step=step)
    want = _brute_search(SEQ, 3, 8, positions=sites, cutoff=cut)
    _assert_levels_are(part, want, SEQ)
    assert part[0] and all(h.ddG <= cut for lv in part for h in lv)
    for bad, word in ((dict(order=0, beam=4), "order=0"), (dict(order=9, beam=4), "order=9"), (dict(order=2, beam=0), "beam=0"),
                      (dict(order=2, beam=129), "beam=129"), (dict(order=1, beam=257), "beam=257"), (dict(order=2, beam=4, positions=[3]), "position 3"),
                      (dict(order=2, beam=4, positions=[5]), "position 5"), (dict(order=2, beam=4, positions=[12]), "position 12")):
        with pytest.raises(ValueError, match=word):
            multi_mutant_search(None, pdb, _tables=stub_tables, _step=StubStep(), **bad)
    with pytest.raises(ValueError, match="2048"):
        multi_mutant_search(None, [{"seq": "A" * 2049}], 2, 4, _tables=stub_tables, _step=StubStep())
    deep = multi_mutant_search(None, pdb, 8, 32, positions=sites, _tables=stub_tables, _step=StubStep())
    assert [bool(lv) for lv in deep] == [True] * 3 + [False] * 5           # three sites: no mutant of four substitutions


def test_command_line_parses_and_writes_the_csv_columns(tmp_path, capsys):
    from thermompnn_amd import variant_scan
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    X, seq = synthetic_backbone(14, 5)
    path = tmp_path / "tiny.pdb"
    path.write_text(backbone_pdb_text(X, seq))
    pdb = alt_parse_PDB(str(path), "A")
    out = tmp_path / "multi.csv"
    argv = [str(path), "--chain", "A", "--combine", "3", "--beam", "6", "--cutoff", "0.5", "--include_cys", "--out", str(out)]
    assert variant_scan.main(argv, _tables=stub_tables, _step=StubStep()) == 0
    assert "18 mutants of 1 .. 3 substitutions" in capsys.readouterr().out
    levels = variant_scan.multi_mutant_search(None, pdb, 3, 6, cutoff=0.5, include_cys=True, _tables=stub_tables, _step=StubStep())
    _assert_levels_are(levels, _brute_search(seq, 3, 6, cutoff=0.5, include_cys=True), seq)
    lines = out.read_text().split("\n")
    assert lines[0] == "order,rank,mutations,ddG,ddG_additive,epistasis" and lines[-1] == "" and len(lines) == 20
    flat = [(d, r, h) for d, hits in enumerate(levels, 1) for r, h in enumerate(hits)]
    for line, (d, r, h) in zip(lines[1:], flat):
        f = line.split(",")
        assert f[0] == str(d) and f[1] == str(r) and f[2].count(":") == d - 1
        assert f[2].split(":") == [f"{seq[m.position]}{m.position + 1}{m.mutation}" for m in h.mutations]         # A12G: 1-based
        assert [float(x) for x in f[3:]] == [h.ddG, h.ddG_additive, h.epistasis]
        assert variant_scan.parse_variant_line(f[2].replace(":", ",")) == [variant_scan.Mutation(m.position, m.wildtype, m.mutation)
                                                                          for m in h.mutations]
    # --combine is a member of the exclusive group, goes with --beam, and takes --cutoff and --include_cys but not --unordered
    base = [str(path), "--out", str(out), "--synthetic_weights", "0"]
    for bad, word in ((["--combine", "3", "--beam", "4", "--all-singles"], "not allowed with"),
                      (["--combine", "3", "--beam", "4", "--top-pairs", "5"], "not allowed with"),
                      (["--combine", "3", "--beam", "4", "--pair-map"], "not allowed with"),
                      (["--combine", "3"], "go together"), (["--all-singles", "--beam", "4"], "go together"),
                      (["--combine", "0", "--beam", "4"], "combine"), (["--combine", "9", "--beam", "4"], "combine"),
                      (["--combine", "3", "--beam", "0"], "beam"), (["--combine", "3", "--beam", "86"], "beam"),
                      (["--combine", "3", "--beam", "4", "--unordered"], "unordered"),
                      (["--all-singles", "--cutoff", "1"], "combine"), (["--pair-map", "--cutoff", "1"], "combine")):
        with pytest.raises(SystemExit):
            variant_scan.main(base + bad, _tables=stub_tables, _step=StubStep())
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        variant_scan.main([str(path), "--out", "x.npz", "--combine", "3", "--beam", "4"], _tables=stub_tables, _step=StubStep())
    assert "CSV" in capsys.readouterr().err
    assert variant_scan.main(base + ["--combine", "3", "--beam", "85"], _tables=stub_tables, _step=StubStep()) == 0


def test_argument_errors_and_sizer_zeros_need_no_gpu():
    from thermompnn_amd import _lib, build
    assert "tmpnn_beam.hip" in build.SOURCES and build.FILE_FLAGS["tmpnn_beam.hip"] == []       # built with NaNs honoured
    assert (_lib.BEAM_INCLUDE_CYS, _lib.BEAM_MAX_LEN, _lib.BEAM_MAX_V, _lib.BEAM_MAX_DEPTH, _lib.BEAM_MAX_KD) == (1, MAX_LEN, MAX_V, MAX_DEPTH,
                                                                                                             MAX_KD)
    lib = _lib.load()
    assert lib.tmpnn_version() == 200
    size = lib.tmpnn_beam_step_workspace_bytes
    assert size(10, 100, 0, 2) == 0 and size(10, 100, 8, 0) == 0 and size(10, 100, 8, 9) == 0 and size(10, 100, -1, 2) == 0
    assert size(10, 100, 257, 1) == 0 and size(10, 100, 129, 2) == 0 and size(10, 100, 33, 8) == 0 and size(10, 100, 86, 3) == 0
    assert size(-1, 100, 8, 2) == 0 and size(10, -1, 8, 2) == 0 and size(10, 2049, 8, 2) == 0 and size(65537, 10, 8, 2) == 0
    assert size(1 << 31, 1, 8, 2) == 0 and size(1 << 20, 2048, 8, 2) == 0
    assert size(10, 100, 256, 1) > 0 and size(10, 100, 128, 2) > 0 and size(10, 100, 32, 8) > 0 and size(10, 100, 85, 3) > 0
    assert size(65536, 2048, 8, 2) > 0 and size(10, 2048, 32, 8) >= 20 * 256 * 8
    assert size(10, 100, 8, 2) >= 10 * 16 * 8 and size(300, 20, 16, 2) >= 255 * 32 * 8 and size(40, 257, 85, 3) >= 31 * 255 * 8
    assert size(0, 100, 8, 2) > 0 and size(10, 0, 8, 2) > 0                # the merge alone
    d = C.c_void_p(256)                                                   # never dereferenced: every call below fails before a launch

    def call(ddg=d, ld=21, S=d, score=d, muts=d, depth=3, allowed=None, V=4, L=100, k=8, cutoff=INF, flags=0, o1=d, o2=d, o3=d, o4=d, o5=d,
             ws=d, nbytes=1 << 20):
        return lib.tmpnn_beam_step(ddg, ld, S, score, muts, depth, allowed, V, L, k, cutoff, flags, o1, o2, o3, o4, o5, ws, nbytes, None)

    for name in ("ddg", "S", "score", "muts", "o1", "o2", "o3", "o4", "o5", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(k=0) == -1 and b"k=0" in lib.tmpnn_last_error() and call(k=-3) == -1
    assert call(depth=0) == -1 and b"depth=0" in lib.tmpnn_last_error()
    assert call(depth=9) == -1 and b"depth=9" in lib.tmpnn_last_error()
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert call(V=-1) == -1 and b"sizes" in lib.tmpnn_last_error() and call(L=-1) == -1
    assert call(flags=2) == -1 and b"flag" in lib.tmpnn_last_error() and call(flags=-1) == -1
    assert call(cutoff=NAN) == -1 and b"NaN" in lib.tmpnn_last_error()
    assert call(k=86) == -2 and b"256" in lib.tmpnn_last_error()          # TMPNN_E_UNSUPPORTED: k depth = 258
    assert call(k=257, depth=1) == -2 and call(k=33, depth=8) == -2 and call(k=1 << 30, depth=8) == -2
    assert call(L=2049) == -2 and b"2048" in lib.tmpnn_last_error()
    assert call(V=65537, L=10) == -2 and b"65536" in lib.tmpnn_last_error()
    assert call(V=65536, L=2048, k=256, depth=1, nbytes=64) == -4         # served at the top of every field
    assert call(nbytes=64) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert call(V=0, o1=None) == -1 and call(L=0, o5=None) == -1          # an empty call still needs its outputs
    assert call(V=0, ddg=None, S=None, score=None, muts=None, nbytes=64) == -4 and call(depth=1, muts=None, nbytes=64) == -4   # past the pointer checks
