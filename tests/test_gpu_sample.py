"""Autoregressive sampling on the GPU (Engine.sample / ProteinMPNN.sample, tmpnn_sample): the imported reference's fixtures with
their recorded uniforms; the teacher-forced identity (the sampler's own sequence and order fed to Engine.decode_ordered must give
back the sampler's probabilities) on every form; the torch restatement on the device's own graph of the masked layouts, K = 30 and
several orders; chain independence bit for bit; the draw rule; fixed and masked positions; argument errors; the range retry."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, weights_for_case
from masked_backbones import checked_graph, pack, protein
from sample_restatement import inverse_orders, sample_chains

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # the project's line on log-probabilities; a softmax at temperature T moves at most 1 / (2 T) per unit of logit
MARGIN = 1e-3             # 100 x the line: every compared draw sits this far from a cumulative boundary
PRECISIONS = ["f16x2", "bf16x3"]
_ENGINES, _MODELS = {}, {}


def engine(precision, K=48):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if (precision, K) not in _ENGINES:
        _ENGINES[precision, K] = Engine(synthetic_state_dict(0), "cuda:0", K, precision=precision, retry_precision=None)
    return _ENGINES[precision, K]


def model_for(precision):
    from thermompnn_amd import weights
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    if precision not in _MODELS:
        m = ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
        m.load_state_dict(weights.split_transfer_state_dict(weights.synthetic_state_dict(0))[0])
        m.precision, m.retry_precision = precision, None
        _MODELS[precision] = m.eval().cuda()
    return _MODELS[precision]


def golden_protein(case):
    g = load_golden(case)
    return dict(X=g["X"], S=g["S"].astype(np.int64), mask=g["mask"], ridx=g["residue_idx"].astype(np.int64), cenc=g["chain_enc"].astype(np.int64))


def fixture_of(p):
    return dict(X=p["X"], S=p["S"], mask=p["mask"], residue_idx=p["ridx"], chain_enc=p["cenc"], weight_seed=np.int64(0))


def encode(eng, prots):
    p = pack(prots)
    return eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"]), p


def chains(L, N, seed, mask=None, fixed_every=0):
    """N chains over L residues: a seeded permutation each (chain 0 left to right, chain 1 reversed when N > 2), random fixed
    letters, uniforms, and every ``fixed_every``-th position fixed."""
    rng = np.random.default_rng(seed)
    order = np.stack([rng.permutation(L) for _ in range(N)])
    if N > 2:
        order[0], order[1] = np.arange(L), np.arange(L)[::-1]
    free = np.ones((N, L), np.float32)
    if fixed_every:
        free[:, ::fixed_every] = 0
    return dict(order=order.astype(np.int64), S_fixed=rng.integers(0, 21, (N, L)), free=free, u=rng.random((N, L)).astype(np.float32))


def run(eng, enc, c, **kw):
    return eng.sample(enc, c["order"], c["S_fixed"], c["free"], c["u"], **kw)


def teacher_forced(eng, enc, res, c, mask, temperature=1.0, bias=None, allowed=None, tag=""):
    """The sampler's own S and order through Engine.decode_ordered: probs rebuilt from those log_probs with the same temperature,
    bias and allowed tables match on every free position, and the other rows are exactly 0."""
    ranks = inverse_orders(c["order"])
    lp = eng.decode_ordered(enc, res["S"], ranks)["log_probs"]
    z = lp / temperature
    if bias is not None:
        z = z + torch.as_tensor(bias, dtype=torch.float32, device=z.device)
    p = torch.softmax(z, dim=-1)
    if allowed is not None:
        pm = p * torch.as_tensor(allowed, dtype=torch.float32, device=z.device)
        p = pm / pm.sum(-1, keepdim=True)
    is_free = torch.as_tensor(c["free"] * np.asarray(mask)[None] == 1, device=z.device)
    err = float((res["probs"] - p)[is_free].abs().max()) if bool(is_free.any()) else 0.0
    print(f"{tag} teacher-forced: {err:.3e} (line {TOL_INTERMEDIATE / temperature:g}), {int(is_free.sum())} free positions")
    assert err <= TOL_INTERMEDIATE / temperature, (tag, err)
    assert bool((res["probs"][~is_free] == 0).all())
    fixed = torch.as_tensor(c["S_fixed"], device=z.device).to(torch.int32)
    assert torch.equal(res["S"][~is_free], fixed[~is_free])
    assert int(res["S"].min()) >= 0 and int(res["S"].max()) < 21
    s = res["probs"][is_free].sum(-1)
    assert float((s - 1).abs().max()) < 1e-5


def against_restatement(res, ref, temperature, tag):
    err = float(np.abs(res["probs"].cpu().numpy().astype(np.float64) - ref["probs"]).max())
    print(f"{tag} restatement: probs {err:.3e} (line {TOL_INTERMEDIATE / temperature:g}), smallest margin {ref['min_margin']:.2e} (bar {MARGIN:g})")
    assert ref["min_margin"] >= MARGIN
    assert np.array_equal(res["S"].cpu().numpy(), ref["S"]), tag
    assert err <= TOL_INTERMEDIATE / temperature, (tag, err)


# ---- the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_A_gap"])
def test_reference_goldens(case, precision):
    g, o = load_golden(case), load_golden("sample_" + case)
    N, temperature = o["randn"].shape[0], float(o["temperature"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dt)
    rep = lambda a, dt: t(a, dt)[None].repeat(N, *([1] * np.ndim(a)))
    m = model_for(precision)
    with torch.no_grad():
        out = m.sample(rep(g["X"], torch.float32), t(o["randn"], torch.float32), t(o["S_true"], torch.int64), t(o["chain_mask"], torch.float32),
                       rep(g["chain_enc"], torch.int64), rep(g["residue_idx"], torch.int64), mask=rep(g["mask"], torch.float32),
                       temperature=temperature, omit_AAs_np=o["omit_AAs"], bias_AAs_np=o["bias_AAs"], chain_M_pos=t(o["chain_M_pos"], torch.float32),
                       omit_AA_mask=t(o["omit_AA_mask"], torch.float32) if "omit_AA_mask" in o else None,
                       bias_by_res=t(o["bias_by_res"], torch.float32), uniforms=t(o["u"], torch.float32))
    assert out["S"].dtype == torch.int64 and out["S"].shape == (N, len(g["S"])) and out["probs"].shape == (N, len(g["S"]), 21)
    err = float(np.abs(out["probs"].cpu().numpy().astype(np.float64) - o["probs"]).max())
    print(f"{case}/{precision}: probs {err:.3e} (line {TOL_INTERMEDIATE / temperature:g}), golden margin {float(o['min_margin']):.2e}")
    assert np.array_equal(out["decoding_order"].cpu().numpy(), o["decoding_order"])
    assert np.array_equal(out["S"].cpu().numpy(), o["S"])
    assert err <= TOL_INTERMEDIATE / temperature
    fixed = (o["free"] * g["mask"][None]) != 1
    assert (out["probs"].cpu().numpy()[fixed] == 0).all()


# ---- masked layouts on the device's own graph ------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["msk_L17", "msk_L40", "msk_L56_2ch"])
def test_masked_layouts(name, precision):
    eng, p = engine(precision), protein(name)
    enc, _ = encode(eng, [p])
    ei, _ = checked_graph(name, enc.E_idx.cpu().numpy())
    L = len(p["S"])
    c = chains(L, 3, 5, fixed_every=4)
    temperature = 0.5
    ref = sample_chains(weights_for_case(fixture_of(p)), fixture_of(p), c["order"], c["S_fixed"], c["free"], c["u"], temperature, E_idx=ei,
                        margin=MARGIN, rng=np.random.default_rng(6))
    c["u"] = ref["u"]
    res = run(eng, enc, c, temperature=temperature)
    against_restatement(res, ref, temperature, f"{name}/{precision}")
    teacher_forced(eng, enc, res, c, p["mask"], temperature, tag=f"{name}/{precision}")
    dead = p["mask"] == 0
    assert (res["probs"].cpu().numpy()[:, dead] == 0).all() and np.array_equal(res["S"].cpu().numpy()[:, dead], c["S_fixed"][:, dead])


# ---- other forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_k30_and_orders(precision):
    """K = 30, and within one group: left to right, reversed, and two different permutations."""
    p = golden_protein("syn_L32")
    for K in (30, 48):
        eng = engine(precision, K)
        enc, _ = encode(eng, [p])
        ei = enc.E_idx.cpu().numpy()
        Keff = min(K, 32)
        assert (ei[:, Keff:] == -1).all() and (ei[:, :Keff] >= 0).all()
        c = chains(32, 4, 21)
        ref = sample_chains(weights_for_case(fixture_of(p)), fixture_of(p), c["order"], c["S_fixed"], c["free"], c["u"], 1.0, E_idx=ei[:, :Keff],
                            margin=MARGIN, rng=np.random.default_rng(8))
        c["u"] = ref["u"]
        res = run(eng, enc, c)
        against_restatement(res, ref, 1.0, f"K{K}/{precision}")
        teacher_forced(eng, enc, res, c, p["mask"], tag=f"K{K}/{precision}")
        assert not np.array_equal(ref["S"][0], ref["S"][1])                 # the orders matter


@pytest.mark.parametrize("precision", PRECISIONS)
def test_packed_context_with_bias_and_allowed(precision):
    """Two proteins in one context, a chain runs over the whole packed axis; per-residue bias and allowed tables."""
    eng = engine(precision)
    prots = [golden_protein("syn_L32"), protein("msk_L17")]
    enc, pk = encode(eng, prots)
    T = 49
    c = chains(T, 5, 33, fixed_every=7)
    rng = np.random.default_rng(2)
    temperature = 0.7
    bias = (rng.normal(size=(T, 21)) * 0.5).astype(np.float32)
    bias[:, 20] -= 1e8
    allowed = (rng.random((T, 21)) > 0.2).astype(np.float32)
    allowed[:, 0] = 1
    res = run(eng, enc, c, temperature=temperature, bias=bias, allowed=allowed)
    mask = pk["mask"].cpu().numpy()
    teacher_forced(eng, enc, res, c, mask, temperature, bias, allowed, tag=f"packed/{precision}")
    is_free = c["free"] * mask[None] == 1
    S = res["S"].cpu().numpy()
    assert (S[is_free] != 20).all() and (allowed[np.nonzero(is_free)[1], S[is_free]] == 1).all()      # never an omitted letter


# ---- independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_independence(precision):
    """N = 33: two full groups and a tail of one. A chain has the same bits alone, in another slot, and under three chunks."""
    eng, p = engine(precision), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    c = chains(32, 33, 44, fixed_every=9)
    full = run(eng, enc, c)
    again = run(eng, enc, c)
    assert torch.equal(full["S"], again["S"]) and torch.equal(full["probs"], again["probs"])
    for k in (0, 15, 16, 32):
        alone = run(eng, enc, {key: v[k:k + 1] for key, v in c.items()})
        assert torch.equal(alone["S"][0], full["S"][k]) and torch.equal(alone["probs"][0], full["probs"][k]), k
    perm = np.roll(np.arange(33), 5)
    moved = run(eng, enc, {key: v[perm] for key, v in c.items()})
    assert torch.equal(moved["S"], full["S"][perm]) and torch.equal(moved["probs"], full["probs"][perm])
    chunked = run(eng, enc, c, max_rows=11 * 32)
    assert torch.equal(chunked["S"], full["S"]) and torch.equal(chunked["probs"], full["probs"])
    teacher_forced(eng, enc, full, c, p["mask"], tag=f"N33/{precision}")
    assert len({tuple(r) for r in full["S"].cpu().numpy().tolist()}) > 16


# ---- the draw rule --------------------------------------------------------------------------------------------------
def test_the_draw_rule():
    """64 chains that differ only in the uniform of the first decoded residue, u = (n + 0.5) / 64: the picks are non-decreasing in
    n and every letter is drawn 64 p_a times up to 1."""
    eng, p = engine("f16x2"), protein("msk_L17")
    enc, _ = encode(eng, [p])
    L, N = 17, 64
    first = int(np.nonzero(p["mask"] > 0)[0][3])
    order = np.concatenate([[first], np.setdiff1d(np.arange(L), [first])])
    c = dict(order=np.tile(order, (N, 1)), S_fixed=np.zeros((N, L), np.int64), free=np.ones((N, L), np.float32),
             u=np.tile(np.random.default_rng(1).random(L).astype(np.float32), (N, 1)))
    c["u"][:, first] = (np.arange(N) + 0.5) / N
    res = run(eng, enc, c, temperature=2.0)
    picks, probs = res["S"][:, first].cpu().numpy(), res["probs"][:, first].cpu().numpy()
    assert (probs == probs[0]).all()
    assert (np.diff(picks) >= 0).all() and len(set(picks.tolist())) > 3
    counts = np.bincount(picks, minlength=21)
    print("draw rule: counts", counts.tolist(), "64 p", np.round(64 * probs[0], 2).tolist())
    assert (np.abs(counts - 64 * probs[0].astype(np.float64)) <= 1).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch():
    from thermompnn_amd._lib import TmpnnError
    eng, p = engine("f16x2"), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    c = chains(32, 2, 3)
    sentinel = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    eng._status.copy_(sentinel)
    bad = dict(c, order=c["order"].copy())
    bad["order"][1, 5] = bad["order"][1, 6]
    with pytest.raises(TmpnnError, match="permutation"):
        run(eng, enc, bad)
    with pytest.raises(TmpnnError, match="permutation"):
        run(eng, enc, dict(c, order=c["order"] + 1))
    letters = dict(c, S_fixed=c["S_fixed"].copy())
    letters["S_fixed"][0, 0] = 21
    with pytest.raises(TmpnnError, match="residue indices"):
        run(eng, enc, letters)
    with pytest.raises(TmpnnError, match="temperature"):
        run(eng, enc, c, temperature=0.0)
    with pytest.raises(TmpnnError, match="order"):
        run(eng, enc, dict(c, u=c["u"][:, :31]))
    assert int(eng._status.item()) == 77                    # tmpnn_sample zeroes the word on the stream first: it never ran
    m = model_for("f16x2")
    X = torch.zeros(1, 32, 4, 3, device="cuda:0")
    z = torch.zeros(1, 32, device="cuda:0")
    for flag in ("pssm_bias_flag", "pssm_log_odds_flag"):
        with pytest.raises(NotImplementedError):
            m.sample(X, z, z.long(), z + 1, z.long(), z.long(), mask=z + 1, **{flag: True})
    with pytest.raises(ValueError, match="temperature"):
        m.sample(X, z, z.long(), z + 1, z.long(), z.long(), mask=z + 1, temperature=0)
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    fp32 = Engine(synthetic_state_dict(0), "cuda:0", 48, precision="fp32", retry_precision=None)
    with pytest.raises(TmpnnError, match="bf16x3"):
        run(fp32, encode(fp32, [p])[0], c)


# ---- the range contract --------------------------------------------------------------------------------------------
def test_range_overflow_raises_or_retries(synthetic_weights):
    """Weights scaled as test_gpu_ordered.test_range_overflow_raises_or_retries scales them: the f16x2 sampler raises without a
    retry precision; with one it warns and returns the bf16x3 result, bit for bit what a direct bf16x3 call gives."""
    from thermompnn_amd._lib import TmpnnRangeError
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    p = golden_protein("syn_L32")
    c = chains(32, 2, 9)
    direct = Engine(W, "cuda:0", 48, precision="bf16x3", retry_precision=None)
    want = run(direct, encode(direct, [p])[0], c)
    assert bool(torch.isfinite(want["probs"]).all())
    strict = Engine(W, "cuda:0", 48, precision="f16x2", retry_precision=None)
    with pytest.raises(TmpnnRangeError):
        run(strict, encode(strict, [p])[0], c)
    eng = Engine(W, "cuda:0", 48, precision="f16x2")
    enc = encode(eng, [p])[0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run(eng, enc, c)
    assert any("bf16x3" in str(w.message) for w in rec)
    assert all(w.category is RuntimeWarning and w.filename == __file__ for w in rec if "bf16x3" in str(w.message))     # attributed to the caller
    assert torch.equal(got["S"], want["S"]) and torch.equal(got["probs"], want["probs"])
