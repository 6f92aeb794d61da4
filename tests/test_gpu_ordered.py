"""Order-masked decoding on the GPU (Engine.decode_ordered, ProteinMPNN.conditional_probs / unconditional_probs,
ProteinMPNNBaseline(scoring=...)): parity with the imported reference's stored tensors, arbitrary orders against the torch
restatement on the device's graph, batch invariance bit for bit, the range contract and the ISA record of the new instantiations."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, HOT_F64_FACTOR, REPO, is_hot, load_golden, weights_for_case
from ordered_restatement import ordered_decode

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for decoder states and log-probabilities
TOL_DDG = 1e-4            # kcal/mol
ORDER_MOVES = 1e-3        # 100 x the line: two opposite orders must differ by more than this somewhere
PRECISIONS = ["f16x2", "bf16x3", "fp32"]
_ENGINES, _MODELS, _RESTATED = {}, {}, {}


def engine_for(g, precision):
    from thermompnn_amd.engine import Engine
    key = (int(g["weight_seed"]), str(g["weight_style"]) if "weight_style" in g else "xavier", precision)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(weights_for_case(g), "cuda:0", 48, precision=precision, retry_precision=None)
    return _ENGINES[key]


def model_for(precision):
    """ProteinMPNN with the seed-0 Xavier weights at ``precision``, the range retry disabled."""
    from thermompnn_amd import weights
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    if precision not in _MODELS:
        m = ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
        m.load_state_dict(weights.split_transfer_state_dict(weights.synthetic_state_dict(0))[0])
        m.precision, m.retry_precision = precision, None
        _MODELS[precision] = m.eval().cuda()
    return _MODELS[precision]


def packed(g, dev="cuda:0"):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    L = len(g["S"])
    return dict(X=t(g["X"], torch.float32), S=t(g["S"], torch.int32), mask=t(g["mask"], torch.float32),
                ridx=t(g["residue_idx"], torch.int32), cenc=t(g["chain_enc"], torch.int32),
                offsets=torch.tensor([0, L], dtype=torch.int32, device=dev), L=L)


def encode(eng, p):
    return eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])


def batch_of(g, dev="cuda:0"):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)[None]
    return dict(X=t(g["X"], torch.float32), S=t(g["S"], torch.int64), mask=t(g["mask"], torch.float32),
                ridx=t(g["residue_idx"], torch.int64), cenc=t(g["chain_enc"], torch.int64))


def orders_of(g):
    """(sequences [V,L], ranks [V,L]): two sequences under each of left-to-right, reversed, a seeded permutation, all equal and a
    two-level rank with ties (first half 0, second half 1)."""
    S = g["S"].astype(np.int64)
    L, rng = len(S), np.random.default_rng(13)
    other = np.where(S == 20, 20, (S + 1 + rng.integers(0, 19, L)) % 20)        # gaps stay gaps
    ranks = [np.arange(L), np.arange(L)[::-1].copy(), rng.permutation(L), np.zeros(L, np.int64), (np.arange(L) >= L // 2).astype(np.int64)]
    seqs = np.stack([s for _ in ranks for s in (S, other)])
    return seqs, np.stack([r for r in ranks for _ in range(2)]).astype(np.int64)


def restated(g, case, seqs, ranks, ei, f64=False):
    key = (case, seqs.tobytes(), ranks.tobytes(), ei.tobytes(), f64)
    if key not in _RESTATED:
        _RESTATED[key] = ordered_decode(weights_for_case(g), g, seqs, ranks, ei, f64=f64)
    return _RESTATED[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_A", "2OCJ_A_gap"])
def test_probs_match_the_reference(case, precision):
    g, o = load_golden(case), load_golden("ordered_" + case)
    b, m = batch_of(g), model_for(precision)
    chain_M = torch.ones_like(b["mask"])
    randn = torch.from_numpy(o["randn"]).cuda()
    with torch.no_grad():
        got = {"cond": m.conditional_probs(b["X"], b["S"], b["mask"], chain_M, b["ridx"], b["cenc"], randn),
               "cond_backbone_only": m.conditional_probs(b["X"], b["S"], b["mask"], chain_M, b["ridx"], b["cenc"], randn, backbone_only=True),
               "uncond": m.unconditional_probs(b["X"], b["mask"], b["ridx"], b["cenc"])}
    dead = np.nonzero(g["mask"] == 0)[0]
    for k, v in got.items():
        assert v.shape == (1, len(g["S"]), 21) and v.is_cuda
        err = float(np.abs(v[0].cpu().numpy().astype(np.float64) - o[k]).max())
        print(f"{case}/{precision}/{k}: {err:.3e} (line {TOL_INTERMEDIATE:g})")
        assert err <= TOL_INTERMEDIATE, (case, precision, k, err)
        if k != "uncond":
            assert (v[0].cpu().numpy()[dead] == 0).all()        # rows that are not looped over: exactly 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_chain_M_loops_over_the_subset_only(precision):
    """chain_M selects a designable subset (here also covering residues whose mask is 0): fewer variants than L, so variant v is
    not position v. Rows outside chain_M * mask are exactly 0; rows inside have the bits of the all-ones call (a variant's numbers
    do not depend on V or on its slot) and sit within the line of the reference's tensor."""
    g, o = load_golden("2OCJ_A_gap"), load_golden("ordered_2OCJ_A_gap")
    b, m = batch_of(g), model_for(precision)
    L = len(g["S"])
    pick = np.zeros(L, bool)
    pick[3::7] = True
    pick[100:131] = True
    pick[np.nonzero(g["mask"] == 0)[0]] = True                  # masked residues inside the selection are still not looped over
    chain_M = torch.from_numpy(pick.astype(np.float32)).cuda()[None]
    randn = torch.from_numpy(o["randn"]).cuda()
    looped = pick & (g["mask"] == 1)
    assert 0 < looped.sum() < (g["mask"] == 1).sum() and not looped[0] and looped[3]
    with torch.no_grad():
        full = m.conditional_probs(b["X"], b["S"], b["mask"], torch.ones_like(b["mask"]), b["ridx"], b["cenc"], randn)[0].cpu()
        for bb in (False, True):
            part = m.conditional_probs(b["X"], b["S"], b["mask"], chain_M, b["ridx"], b["cenc"], randn, backbone_only=bb)[0].cpu()
            assert (part[torch.from_numpy(~looped)] == 0).all()
            ref = o["cond_backbone_only" if bb else "cond"]
            assert float(np.abs(part.numpy()[looped].astype(np.float64) - ref[looped]).max()) <= TOL_INTERMEDIATE
            if not bb:
                assert torch.equal(part[torch.from_numpy(looped)], full[torch.from_numpy(looped)])


def test_conditional_probs_takes_one_structure_and_unconditional_any_batch():
    g = load_golden("syn_L32")
    b, m = batch_of(g), model_for("f16x2")
    two = {k: torch.cat([v, v]) for k, v in b.items()}
    with pytest.raises(NotImplementedError):
        m.conditional_probs(two["X"], two["S"], two["mask"], torch.ones_like(two["mask"]), two["ridx"], two["cenc"], torch.randn(1, 32))
    with torch.no_grad():
        one = m.unconditional_probs(b["X"], b["mask"], b["ridx"], b["cenc"])
        both = m.unconditional_probs(two["X"], two["mask"], two["ridx"], two["cenc"])
    assert both.shape == (2, 32, 21) and torch.equal(both[0], one[0]) and torch.equal(both[1], one[0])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_A_gap", "2OCJ_AB", "2OCJ_A_hot"])
def test_arbitrary_orders_match_the_restatement(case, precision):
    g = load_golden(case)
    eng = engine_for(g, precision)
    p = packed(g)
    enc = encode(eng, p)
    ei = enc.E_idx.cpu().numpy()[:, :min(48, p["L"])]
    seqs, ranks = orders_of(g)
    res = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert (got["ddg"][np.arange(len(seqs))[:, None], np.arange(p["L"]), seqs] == 0).all()      # relative to the variant's own residue
    ref = restated(g, case, seqs, ranks, ei)
    t64 = restated(g, case, seqs, ranks, ei, f64=True) if is_hot(g) else None
    for what, line in (("hidden", TOL_INTERMEDIATE), ("log_probs", TOL_INTERMEDIATE), ("ddg", TOL_DDG)):
        if t64 is not None:
            truth = t64[what].astype(np.float64)
            ref_err = float(np.abs(ref[what].astype(np.float64) - truth).max())
            hip_err = float(np.abs(got[what].astype(np.float64) - truth).max())
            print(f"{case}/{precision}/{what}: |hip - f64| {hip_err:.3e}, |restatement fp32 - f64| {ref_err:.3e}")
            assert hip_err <= HOT_F64_FACTOR * ref_err, (case, precision, what, hip_err, ref_err)
        else:
            err = np.abs(got[what].astype(np.float64) - ref[what]).reshape(len(seqs), -1).max(1)
            print(f"{case}/{precision}/{what}: per variant {np.array2string(err, precision=2)} (line {line:g})")
            assert err.max() <= line, (case, precision, what, err)
    # the order is honoured: left-to-right (variant 0) and reversed (variant 2) of the same sequence are far apart
    assert float(np.abs(ref["log_probs"][0] - ref["log_probs"][2]).max()) > ORDER_MOVES
    assert float(np.abs(got["log_probs"][0] - got["log_probs"][2]).max()) > ORDER_MOVES


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_pair_has_the_same_bits_in_any_batch(precision):
    g = load_golden("2OCJ_A_gap")
    eng = engine_for(g, precision)
    enc = encode(eng, packed(g))
    rng = np.random.default_rng(3)
    S = g["S"].astype(np.int64)
    L = len(S)
    mine, my_rank = S.copy(), rng.permutation(L)
    mine[[5, 40, 41]] = [(S[5] + 1) % 20, (S[40] + 2) % 20, (S[41] + 9) % 20]
    others = rng.integers(0, 21, (36, L))
    other_ranks = np.stack([rng.permutation(L) for _ in range(36)])
    want = dict(want_hidden=True, want_log_probs=True)
    plain_before = eng.decode_variants(enc, mine[None], want_ddg=False, **want)
    alone = eng.decode_ordered(enc, mine[None], my_rank[None], **want)
    first = eng.decode_ordered(enc, np.concatenate([mine[None], others]), np.concatenate([my_rank[None], other_ranks]), **want)
    last = eng.decode_ordered(enc, np.concatenate([others, mine[None]]), np.concatenate([other_ranks, my_rank[None]]), **want)
    chunked = eng.decode_ordered(enc, np.concatenate([others, mine[None]]), np.concatenate([other_ranks, my_rank[None]]), max_rows=L, **want)
    plain_after = eng.decode_variants(enc, mine[None], want_ddg=False, **want)
    for k in ("hidden", "log_probs"):
        assert torch.equal(first[k][0], alone[k][0]), k
        assert torch.equal(last[k][36], alone[k][0]), k
        assert torch.equal(chunked[k], last[k]), k
        assert torch.equal(plain_before[k], plain_after[k]), k           # the unmasked path is untouched by an ordered call
        assert not torch.equal(plain_before[k][0], alone[k][0]), k       # ... and is another computation
    # all ranks equal: nobody sees a sequence, so two different sequences give the same bits
    zero = np.zeros((2, L), np.int64)
    blind = eng.decode_ordered(enc, np.stack([mine, others[0]]), zero, **want)
    assert torch.equal(blind["hidden"][0], blind["hidden"][1]) and torch.equal(blind["log_probs"][0], blind["log_probs"][1])


def test_range_overflow_raises_or_retries(synthetic_weights):
    """Weights scaled as test_gpu_variants.test_range_overflow_raises_or_retries scales them: the f16x2 ordered decode raises
    without a retry precision; with one it warns and returns the bf16x3 result, bit for bit what a direct bf16x3 call gives."""
    from thermompnn_amd._lib import TmpnnRangeError
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    g = load_golden("syn_L32")
    p = packed(g)
    S = np.stack([g["S"], (g["S"] + 4) % 20]).astype(np.int64)
    ranks = np.stack([np.arange(32), np.arange(32)[::-1]]).astype(np.int64)
    direct = Engine(W, "cuda:0", 48, precision="bf16x3", retry_precision=None)
    want = direct.decode_ordered(encode(direct, p), S, ranks)["log_probs"]
    assert bool(torch.isfinite(want).all())
    strict = Engine(W, "cuda:0", 48, precision="f16x2", retry_precision=None)
    with pytest.raises(TmpnnRangeError):
        strict.decode_ordered(encode(strict, p), S, ranks)
    eng = Engine(W, "cuda:0", 48, precision="f16x2")
    enc = encode(eng, p)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = eng.decode_ordered(enc, S, ranks)["log_probs"]
    assert any("bf16x3" in str(w.message) for w in rec)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_baseline_scoring_modes(tmp_path, synthetic_weights):
    from thermompnn_amd import pdb_io, weights
    from thermompnn_amd.pdb_io import tied_featurize
    from thermompnn_amd.thermompnn_benchmarking import ProteinMPNNBaseline

    class AD(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__
    mp, _ = weights.split_transfer_state_dict(synthetic_weights)
    os.makedirs(tmp_path / "vanilla_model_weights")
    weights.save_vanilla_checkpoint(tmp_path / "vanilla_model_weights" / "v_48_020.pt", mp, 48)
    cfg = AD(model=AD(load_pretrained=True, freeze_weights=True), platform=AD(thermompnn_dir=str(tmp_path)))
    pdb = pdb_io.alt_parse_PDB(os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"), "A")
    with torch.no_grad():
        plain = ProteinMPNNBaseline(cfg).eval().cuda().ssm_table(pdb)
        visible = ProteinMPNNBaseline(cfg, scoring="visible").eval().cuda().ssm_table(pdb)
        assert torch.equal(plain, visible)
        base = ProteinMPNNBaseline(cfg, scoring="conditional", seed=5).eval().cuda()
        table = base.ssm_table(pdb)
        f = tied_featurize([pdb[0]], "cuda:0", None, None, None, None, None, None, ca_only=False)
        X, S, mask, chain_M, chain_enc, residue_idx = f[0], f[1], f[2], f[4], f[5], f[12]
        randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(5)).cuda()
        assert torch.equal(table, -base.prot_mpnn.conditional_probs(X, S, mask, chain_M, residue_idx, chain_enc, randn)[0])
        assert float((table - visible).abs().max()) > 1e-2
        unc = ProteinMPNNBaseline(cfg, scoring="unconditional").eval().cuda()
        assert torch.equal(unc.ssm_table(pdb), -unc.prot_mpnn.unconditional_probs(X, mask, residue_idx, chain_enc)[0])
        muts = __import__("thermompnn_amd.ssm", fromlist=["mutation_objects"]).mutation_objects(pdb[0])[:40]
        pred, lp = base(pdb, muts)
        assert torch.equal(lp[0], -table) and abs(pred[3]["ddG"].item() - table[muts[3].position, "ACDEFGHIKLMNPQRSTVWYX".index(muts[3].mutation)].item()) == 0


def test_isa_record_lists_the_order_masked_instantiations_without_scratch():
    import glob
    import bench
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_isa_counts.json")), reverse=True)
    d = next(x for x in (json.load(open(f)) for f in files) if x.get("source_stamp") == bench.kernel_source_stamp())
    mine = {n: e for n, e in d["kernels"].items() if "var_msg8_kernel" in n and ("Lb1E" in n or "true" in n)}      # (mangled or demangled)
    assert any("SplitH2" in n for n in mine) and any("SplitBF3" in n for n in mine), sorted(mine)
    for n, e in mine.items():
        assert int(e.get("scratch_bytes") or 0) == 0, f"{n} spills {e['scratch_bytes']} bytes of scratch"
