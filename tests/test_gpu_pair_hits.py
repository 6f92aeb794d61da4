"""Streaming hit lists over variant tables on the device (tmpnn_select_variant_hits, Engine.select_variant_hits) and the double-mutant
front end on top of them (variant_scan.double_mutant_hits, TransferModel.double_mutant_hits, --top-pairs) against the numpy restatement
of the contract (tests/pair_hits_restatement.py). Every comparison is exact: counts, tags, positions, letters, the state's 64-bit keys,
and the value bits with -0.0 taken as +0.0. The tables of the selection tests are synthetic; only the end-to-end tests run a model."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from pair_hits_restatement import MAX_TAG, assert_variant_hits_equal, variant_hits_reference

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ONE_UP = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
# few values, so that sums tie: +-0, +-inf (inf - inf = NaN), NaN, a denormal, and 1 beside 1 + ulp
POOL = np.array([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, ONE_UP, 1e-40, NAN, INF, -INF], np.float32)
OUTPUTS = ("hit_ddg", "hit_tag", "hit_pos", "hit_aa", "hit_count")


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


def _draw(V, L, seed, ld=21, tags=None):
    rng = np.random.default_rng(seed)
    ddg = POOL[rng.integers(0, len(POOL), size=(V, L, ld))]
    base = POOL[rng.integers(0, len(POOL), size=V)]
    S_var = rng.integers(-2, 22, size=(V, L)).astype(np.int32)           # 20, 21: no residue; negative letters
    tag = (rng.permutation(MAX_TAG + 1)[:V] if tags is None else np.asarray(tags)).astype(np.int32)
    skip = rng.integers(-1, L, size=V).astype(np.int32)
    return dict(ddg=ddg, S_var=S_var, base=base, tag=tag, skip=skip)


@pytest.fixture(scope="module")
def crafted():
    """V = 37 variants of L = 300 rows: the second block of 256 residues has 44. Left unchanged by the tests that share it."""
    c = _draw(37, 300, 1)
    c["tag"][[0, 1, 2]] = 0, MAX_TAG, MAX_TAG + 1                         # the ends of the field, and one tag out of range
    c["skip"][[0, 1, 2, 3]] = -1, 0, 299, 299
    c["base"][5] = NAN
    assert len(set(c["tag"].tolist())) == 37 and (c["S_var"] < 0).any() and (c["S_var"] == 20).any()
    bits = set(c["ddg"].view(np.uint32).ravel().tolist())
    assert {0x80000000, 0, 0x7f800000, 0xff800000, 0x3f800000, 0x3f800001} <= bits and any(0 < b < 0x00800000 for b in bits)
    return c


def _ref(c, k, sl=slice(None), state=None, **kw):
    return variant_hits_reference(c["ddg"][sl], c["S_var"][sl], c["base"][sl], c["tag"][sl], c["skip"][sl], k, kw.get("cutoff"),
                                  kw.get("include_cys", False), kw.get("upper", False), state)


def _run(engine, c, k, sl=slice(None), state=None, dev_ddg=None, **kw):
    ddg = torch.from_numpy(c["ddg"][sl]).cuda() if dev_ddg is None else dev_ddg[sl]
    return engine.select_variant_hits(ddg, c["S_var"][sl], c["base"][sl], c["tag"][sl], k, skip=c["skip"][sl], state=state, **kw)


def test_crafted_chunk_every_k_flag_and_cutoff(engine, crafted):
    dev = torch.from_numpy(crafted["ddg"]).cuda()
    below = float(np.nextafter(np.float32(1.25), np.float32(0)))         # one ulp under the sum 1 + 0.25, which many candidates have
    counts = set()
    for k in (1, 5, 32, 100, 256):
        for cys in (False, True):
            for upper in (False, True):
                for cutoff in (None, 0.0, below):
                    kw = dict(cutoff=cutoff, include_cys=cys, upper=upper)
                    got = _run(engine, crafted, k, dev_ddg=dev, **kw)
                    assert_variant_hits_equal(got, _ref(crafted, k, **kw))
                    counts.add(int(got["hit_count"][0]))
    assert counts == {1, 5, 32, 100, 256}
    full = {name: v.cpu().numpy() for name, v in _run(engine, crafted, 256, dev_ddg=dev, include_cys=True).items()}
    assert not (full["hit_tag"] == crafted["tag"][5]).any() and (full["hit_ddg"] == -INF).all()      # (a NaN base; -inf sums abound)
    # a row stride above 21 is the table's leading dimension; a view that is no such table is copied
    wide = torch.full((37, 300, 24), -5.0, device="cuda")
    wide[:, :, :21] = dev
    assert_variant_hits_equal(_run(engine, crafted, 32, dev_ddg=wide[:, :, :21]), _ref(crafted, 32))
    odd = torch.full((37, 300, 42), -5.0, device="cuda")
    odd[:, :, ::2] = dev
    assert_variant_hits_equal(_run(engine, crafted, 32, dev_ddg=odd[:, :, ::2]), _ref(crafted, 32))
    # few enough candidates (four rows with a letter, in both blocks) for the cutoff to show at k = 256: it parts exactly at the sum
    finite = _draw(3, 300, 4)
    finite["ddg"] = np.where(np.isfinite(finite["ddg"]), finite["ddg"], np.float32(0.25))
    finite["base"][:], finite["skip"][:] = (1.0, ONE_UP, 0.25), -1
    letters = np.full((3, 300), 20, np.int32)
    letters[:, [0, 255, 256, 299]] = 7
    finite["S_var"] = letters
    at, under = _run(engine, finite, 256, cutoff=1.25), _run(engine, finite, 256, cutoff=below)
    assert_variant_hits_equal(at, _ref(finite, 256, cutoff=1.25))
    assert_variant_hits_equal(under, _ref(finite, 256, cutoff=below))
    n_at, n_under = int(at["hit_count"][0]), int(under["hit_count"][0])
    assert n_under < n_at < 256 and float(at["hit_ddg"][n_at - 1]) == 1.25 and float(under["hit_ddg"][n_under - 1]) < 1.25


def test_any_cut_into_calls_and_any_order_give_the_same_bits(engine, crafted):
    dev = torch.from_numpy(crafted["ddg"]).cuda()
    for k, kw in ((5, dict()), (100, dict(upper=True, cutoff=0.25)), (256, dict(include_cys=True))):
        whole = _run(engine, crafted, k, dev_ddg=dev, **kw)
        assert_variant_hits_equal(whole, _ref(crafted, k, **kw))
        again = _run(engine, crafted, k, dev_ddg=dev, **kw)
        cuts = ([slice(0, 1), slice(1, 37)], [slice(0, 7), slice(7, 37)], [slice(7, 37), slice(0, 7)], [slice(1, 37), slice(0, 1)],
                [slice(30, 37), slice(0, 12), slice(12, 30)])
        results = [again]
        for cut in cuts:
            res = state = None
            for sl in cut:
                res = _run(engine, crafted, k, sl=sl, state=state, dev_ddg=dev, **kw)
                state = res["state"]
            results.append(res)
        for res in results:
            assert res["state"].dtype == torch.int64 and torch.equal(res["state"], whole["state"])
            for name in OUTPUTS:
                a, b = res[name], whole[name]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name          # (the bits: NaN padding compares equal)
    # the state of the first call of a cut is what the restatement carries
    first = _run(engine, crafted, 100, sl=slice(0, 7), dev_ddg=dev)
    want = _ref(crafted, 100, sl=slice(0, 7))
    assert_variant_hits_equal(first, want)
    assert_variant_hits_equal(_run(engine, crafted, 100, sl=slice(7, 37), state=first["state"], dev_ddg=dev),
                              _ref(crafted, 100, sl=slice(7, 37), state=want["state"]))


@pytest.mark.parametrize("V,L,k", [(40, 257, 256), (300, 20, 32)])
def test_more_items_than_workgroups(engine, V, L, k):
    """80 items on 31 workgroups (k = 256: 8192 / 256 - 1), 300 items on 255 (k = 32): workgroups loop and carry their leaders."""
    c = _draw(V, L, 10 + V)
    finite = np.random.default_rng(V).standard_normal((V, L, 21)).astype(np.float32)
    for case in (c, dict(c, ddg=finite, base=np.linspace(-1, 1, V).astype(np.float32))):
        for kw in (dict(), dict(upper=True, include_cys=True)):
            assert_variant_hits_equal(_run(engine, case, k, **kw), _ref(case, k, **kw))
    # the winners sit in the LAST items: a workgroup's last trips must reach the result
    late = dict(c, ddg=np.full((V, L, 21), 1.0, np.float32), base=-np.arange(V, dtype=np.float32), S_var=np.zeros((V, L), np.int32),
                skip=np.full(V, -1, np.int32))
    got = _run(engine, late, k)
    assert_variant_hits_equal(got, _ref(late, k))
    assert int(got["hit_tag"][0]) == int(c["tag"][V - 1]) and float(got["hit_ddg"][0]) == 2.0 - V


def test_field_tops_and_the_length_limit(engine):
    from thermompnn_amd._lib import TmpnnError
    c = _draw(2, 2048, 21, tags=[MAX_TAG, 7])
    c["ddg"] = np.where(np.isneginf(c["ddg"]), np.float32(0.25), c["ddg"])
    c["S_var"][:, 2047], c["skip"][:] = 3, (-1, 0)
    c["base"][:] = 0.25
    c["ddg"][0, 2047, 19], c["ddg"][1, 2047, 19], c["ddg"][0, 2047, 0] = -100.0, -99.0, -98.0
    for k in (3, 256):
        got = _run(engine, c, k)
        assert_variant_hits_equal(got, _ref(c, k))
        assert got["hit_tag"][:3].tolist() == [MAX_TAG, 7, MAX_TAG] and got["hit_pos"][:3].tolist() == [2047] * 3
        assert got["hit_aa"][:3].tolist() == [19, 19, 0] and (int(got["state"][0]) & 0xffffffff) == 0xfffffff3
    with pytest.raises(TmpnnError, match="2048"):
        engine.select_variant_hits(torch.zeros((1, 2049, 21), device="cuda"), np.zeros((1, 2049), np.int32), [0.0], [1], 4)
    for bad in (dict(k=0), dict(k=257), dict(k=4, cutoff=NAN), dict(k=4, state=torch.zeros(5, dtype=torch.int64, device="cuda"))):
        with pytest.raises(TmpnnError):
            engine.select_variant_hits(torch.zeros((1, 8, 21), device="cuda"), np.zeros((1, 8), np.int32), [0.0], [1], **bad)
    with pytest.raises(TmpnnError, match="device"):
        engine.select_variant_hits(torch.zeros((1, 8, 21)), np.zeros((1, 8), np.int32), [0.0], [1], 4)


def test_short_lists_no_candidates_and_empty_calls(engine):
    few = _draw(2, 3, 30, tags=[4, 9])
    few["S_var"][:] = [[0, 20, 5], [20, 20, 20]]
    few["ddg"] = np.where(np.isnan(few["ddg"]), np.float32(0.25), few["ddg"])
    few["base"][:], few["skip"][:] = 1.0, -1
    got = _run(engine, few, 100, include_cys=True)
    assert_variant_hits_equal(got, _ref(few, 100, include_cys=True))
    n = int(got["hit_count"][0])
    assert n == 38 and bool(torch.isnan(got["hit_ddg"][n:]).all()) and (got["hit_pos"][n:] == -1).all() and (got["hit_tag"][n:] == -1).all()
    assert (got["hit_aa"][n:] == -1).all() and (got["state"][n:] == -1).all() and (got["state"][:n] != -1).all()
    none = dict(few, S_var=np.full((2, 3), 20, np.int32))
    for case, kw in ((none, dict()), (few, dict(cutoff=-INF, upper=True)), (dict(few, base=np.full(2, NAN, np.float32)), dict()),
                     (dict(few, tag=np.array([-1, MAX_TAG + 1], np.int32)), dict())):
        if kw.get("cutoff") == -INF:
            case = dict(case, ddg=np.abs(np.nan_to_num(case["ddg"], posinf=1.0, neginf=1.0)))
        got = _run(engine, case, 7, **kw)
        assert_variant_hits_equal(got, _ref(case, 7, **kw))
        assert int(got["hit_count"][0]) == 0 and (got["state"] == -1).all() and bool(torch.isnan(got["hit_ddg"]).all())
    # V = 0: without a state the selection is empty; with one, the state is kept and decoded again
    empty = dict(ddg=np.zeros((0, 3, 21), np.float32), S_var=np.zeros((0, 3), np.int32), base=np.zeros(0, np.float32),
                 tag=np.zeros(0, np.int32), skip=np.zeros(0, np.int32))
    got = _run(engine, empty, 7)
    assert_variant_hits_equal(got, _ref(empty, 7))
    assert int(got["hit_count"][0]) == 0 and (got["state"] == -1).all() and (got["hit_aa"] == -1).all()
    kept = _run(engine, few, 7)
    before = {name: v.clone() for name, v in kept.items()}
    after = _run(engine, empty, 7, state=kept["state"])
    assert after["state"] is kept["state"]
    for name in OUTPUTS + ("state",):
        assert torch.equal(after[name].view(torch.int32), before[name].view(torch.int32)), name
    assert int(after["hit_count"][0]) == 7
    zero_rows = dict(ddg=np.zeros((4, 0, 21), np.float32), S_var=np.zeros((4, 0), np.int32), base=np.zeros(4, np.float32),
                     tag=np.arange(4, dtype=np.int32), skip=np.zeros(4, np.int32))
    assert int(_run(engine, zero_rows, 7)["hit_count"][0]) == 0


# ---- end to end: a model, the front end, the command line --------------------------------------------------------------------
def _fixture_entry(g, name):
    """A parsed-structure dict (the shape alt_parse_PDB produces) holding a fixture's own coordinates and sequence."""
    from thermompnn_amd.datasets import ALPHABET
    seq = "".join(ALPHABET[int(s)] for s in g["S"])
    coords = {f"{a}_chain_A": g["X"][:, i].astype(np.float64).tolist() for i, a in enumerate(("N", "CA", "C", "O"))}
    return {"resn_list": [str(i + 1) for i in range(len(seq))], "seq_chain_A": seq, "coords_chain_A": coords, "name": name,
            "num_of_chains": 1, "seq": seq}


@pytest.fixture(scope="module")
def model():
    from thermompnn_amd.custom_inference import load_model
    return load_model(None, None, 0)


def _table_hits(dm, seq, positions, k, include_cys, unordered, cutoff=None):
    """The top of double_mutant_table [P, 20, L, 20] under double_mutant_hits' predicates, sorted by the restatement: the table's
    entries ARE the sums (the same single fp32 add), so they enter with base 0; dropped backgrounds get a tag out of range."""
    from thermompnn_amd.variant_scan import pair_tag, sequence_indices
    wt_idx = sequence_indices(seq)
    P, L = len(positions), len(seq)
    p_of, a_of = np.repeat(positions, 20), np.tile(np.arange(20), P)
    S = np.tile(wt_idx, (P * 20, 1))
    S[np.arange(P * 20), p_of] = a_of
    drop = (a_of == wt_idx[p_of]) | ((a_of == 1) & (not include_cys))
    return variant_hits_reference(dm.reshape(P * 20, L, 20), S, np.zeros(P * 20, np.float32), np.where(drop, -1, pair_tag(p_of, a_of)),
                                  p_of, k, cutoff, include_cys, unordered)


@pytest.mark.parametrize("case", ["syn_L32", "msk_L40"])
def test_double_mutant_hits_equal_the_top_of_the_double_mutant_table(case, model, tmp_path, monkeypatch):
    import masked_backbones as mb
    from thermompnn_amd import variant_scan
    from thermompnn_amd.datasets import ALPHABET
    from thermompnn_amd.pdb_io import alt_parse_PDB
    if case == "syn_L32":
        path, pdb = None, [_fixture_entry(load_golden(case), case)]
    else:
        path = mb.write_layout(case, tmp_path)
        pdb = alt_parse_PDB(path, "A")
        assert "-" in pdb[0]["seq"]
    seq = pdb[0]["seq"]
    positions = [p for p, c in enumerate(seq) if c != "-"]
    with torch.no_grad():
        dm = variant_scan.double_mutant_table(model, pdb).cpu().numpy()
        wt = model.variant_tables(pdb, [seq])[0].cpu().numpy()
    eng = model.engine()
    calls, encode = [], eng.encode
    monkeypatch.setattr(eng, "encode", lambda *a, **kw: (calls.append(1), encode(*a, **kw))[1])
    for unordered in (False, True):
        del calls[:]
        with torch.no_grad():
            hits = model.double_mutant_hits(pdb, 64, unordered=unordered, chunk=100)
        assert len(calls) == 1                                            # the encoder ran once for all 7 chunks or so
        want = _table_hits(dm, seq, positions, 64, False, unordered)
        assert int(want["hit_count"][0]) == 64 == len(hits)
        p, a = variant_scan.split_tag(want["hit_tag"].astype(np.int64))
        assert [(h.first.position, h.first.mutation, h.second.position, h.second.mutation) for h in hits] == \
            [(int(pp), ALPHABET[int(aa)], int(q), ALPHABET[int(b)]) for pp, aa, q, b in zip(p, a, want["hit_pos"], want["hit_aa"])]
        got_bits, want_bits = np.array([h.ddG for h in hits], np.float32).view(np.uint32), want["hit_ddg"].view(np.uint32)
        np.testing.assert_array_equal(got_bits, want_bits)
        for h in hits:
            pp, aa, q, b = h.first.position, ALPHABET.index(h.first.mutation), h.second.position, ALPHABET.index(h.second.mutation)
            assert h.first.wildtype == seq[pp] and h.second.wildtype == seq[q] and seq[q] != "-" and (not unordered or q > pp) and q != pp
            assert h.ddG == float(dm[positions.index(pp), aa, q, b]) and h.ddG_first == float(wt[pp, aa])
            assert h.ddG_additive == float(wt[pp, aa]) + float(wt[q, b]) and h.epistasis == h.ddG - h.ddG_additive
        assert [h.ddG for h in hits] == sorted(h.ddG for h in hits)
    # the other options reach the selection
    cut = float(_table_hits(dm[3:9], seq, positions[3:9], 64, True, True)["hit_ddg"][30])
    with torch.no_grad():
        opt = model.double_mutant_hits(pdb, 64, unordered=True, cutoff=cut, positions=positions[3:9], include_cys=True)
    sub = _table_hits(dm[3:9], seq, positions[3:9], 64, True, True, cutoff=cut)
    n = int(sub["hit_count"][0])
    assert 31 <= n < 64 and [(h.first.position, h.first.mutation, h.second.position, h.second.mutation, h.ddG) for h in opt] == \
        [(int(t) >> 5, ALPHABET[int(t) & 31], int(q), ALPHABET[int(b)], float(v))
         for t, q, b, v in zip(sub["hit_tag"][:n], sub["hit_pos"][:n], sub["hit_aa"][:n], sub["hit_ddg"][:n])]
    if path is None:
        return
    # the command line writes the front end's list
    monkeypatch.undo()
    out, ref = str(tmp_path / "cli.csv"), str(tmp_path / "ref.csv")
    assert variant_scan.main([path, "--chain", "A", "--top-pairs", "64", "--unordered", "--chunk", "100", "--out", out,
                              "--synthetic_weights", "0"]) == 0
    variant_scan.write_pair_hits_csv(ref, hits)
    assert open(out, "rb").read() == open(ref, "rb").read() and open(out).read().count("\n") == 65
