"""Tied sampling and the PSSM terms on the GPU (Engine.sample_tied / ProteinMPNNDesign, tmpnn_sample_tied): the imported reference's
tied_sample / sample fixtures with their recorded uniforms; the torch restatement (tests/tied_restatement.py) on the device's own
graph of the masked layouts, at K = 30 and with different groupings inside one workgroup; the untied equivalence with Engine.sample
bit for bit; chain independence; weights; argument errors; the range retry.

Comparison line for probs: 1e-5 / temperature / min_den (see test_tied_sample_host.py; min_den = 1 where no table renormalises).
S and decoding_order must be identical."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, weights_for_case
from masked_backbones import checked_graph, pack, protein
from tied_restatement import sample_tied_chains

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5
MARGIN = 1e-3
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
    from thermompnn_amd.design import ProteinMPNNDesign
    if precision not in _MODELS:
        m = ProteinMPNNDesign(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
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


def groups_of_four(L):
    return [list(range(i, i + 4)) for i in range(0, L - L % 4, 4)]


def tied_chains(L, N, seed, groupings, fixed_every=0, betas=None):
    """N chains over L residues; chain n regroups a seeded permutation by groupings[n % len(groupings)] (a list of groups) and
    weighs with betas (default 1) / len(group). Random fixed letters and uniforms; every ``fixed_every``-th position fixed."""
    from thermompnn_amd.design import tied_decoding_order
    rng = np.random.default_rng(seed)
    order, close, weight = [], [], []
    for n in range(N):
        tied = groupings[n % len(groupings)]
        o, c = tied_decoding_order(rng.permutation(L), tied)
        size = np.ones(L, np.float32)
        for grp in tied:
            size[grp] = len(grp)
        order.append(o.numpy())
        close.append(c.numpy())
        weight.append((np.ones(L, np.float32) if betas is None else np.asarray(betas, np.float32)) / size)
    free = np.ones((N, L), np.float32)
    if fixed_every:
        free[:, ::fixed_every] = 0
    return dict(order=np.stack(order).astype(np.int64), close=np.stack(close).astype(np.int32), S_fixed=rng.integers(0, 21, (N, L)), free=free,
                u=rng.random((N, L)).astype(np.float32), weight=np.stack(weight))


def run(eng, enc, c, **kw):
    return eng.sample_tied(enc, c["order"], c["close"], c["S_fixed"], c["free"], c["u"], weight=c.get("weight"), **kw)


def restate(p, c, temperature, E_idx, seed, **tables):
    """The restatement on the caller's graph with the margin-redraw rule; c["u"] becomes the uniforms as used."""
    ref = sample_tied_chains(weights_for_case(fixture_of(p)), fixture_of(p), c["order"], c["close"], c["S_fixed"], c["free"], c["u"], temperature,
                             weight=c.get("weight"), E_idx=E_idx, margin=MARGIN, rng=np.random.default_rng(seed), **tables)
    c["u"] = ref["u"]
    return ref


def against_restatement(res, ref, temperature, tag, renormalised=False):
    line = TOL_INTERMEDIATE / temperature / (ref["min_den"] if renormalised else 1.0)
    err = float(np.abs(res["probs"].cpu().numpy().astype(np.float64) - ref["probs"]).max())
    print(f"{tag} restatement: probs {err:.3e} (line {line:g}), smallest margin {ref['min_margin']:.2e} (bar {MARGIN:g}), min den {ref['min_den']:.3f}")
    assert ref["min_margin"] >= MARGIN
    assert np.array_equal(res["S"].cpu().numpy(), ref["S"]), tag
    assert err <= line, (tag, err)


def group_runs(order, close):
    ends = np.nonzero(close)[0]
    return [order[a:b + 1].tolist() for a, b in zip(np.concatenate([[0], ends[:-1] + 1]), ends)]


def check_groups(res, c, mask):
    """Dead groups: S_fixed of the first masked member on every member, probs rows 0. Live groups: one letter, probs rows that sum to 1."""
    S, P = res["S"].cpu().numpy(), res["probs"].cpu().numpy()
    n_dead = 0
    for n in range(S.shape[0]):
        for grp in group_runs(c["order"][n], c["close"][n]):
            masked = [k for k in grp if mask[k] == 0]
            assert len(set(S[n, grp].tolist())) == 1
            if masked:
                n_dead += 1
                assert S[n, grp[0]] == c["S_fixed"][n, masked[0]] and (P[n, grp] == 0).all()
            else:
                assert (np.abs(P[n, grp].sum(-1) - 1) < 1e-5).all() and (P[n, grp] == P[n, grp[:1]]).all()
    return n_dead


# ---- the reference's fixtures ------------------------------------------------------------------------------
def _model_inputs(g, o):
    N = o["randn"].shape[0]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dt)
    rep = lambda a, dt: t(a, dt)[None].repeat(N, *([1] * np.ndim(a)))
    pssm = "pssm_coef" in o
    args = (rep(g["X"], torch.float32), t(o["randn"], torch.float32), t(o["S_true"], torch.int64), t(o["chain_mask"], torch.float32),
            rep(g["chain_enc"], torch.int64), rep(g["residue_idx"], torch.int64))
    kw = dict(mask=rep(g["mask"], torch.float32), temperature=float(o["temperature"]), omit_AAs_np=o["omit_AAs"], bias_AAs_np=o["bias_AAs"],
              chain_M_pos=t(o["chain_M_pos"], torch.float32), omit_AA_mask=t(o["omit_AA_mask"], torch.float32) if "omit_AA_mask" in o else None,
              bias_by_res=t(o["bias_by_res"], torch.float32), uniforms=t(o["u"], torch.float32))
    if pssm:
        kw.update(pssm_coef=t(o["pssm_coef"], torch.float32), pssm_bias=t(o["pssm_bias"], torch.float32), pssm_multi=float(o["pssm_multi"]),
                  pssm_log_odds_flag=True, pssm_log_odds_mask=t(o["pssm_log_odds_mask"], torch.float32), pssm_bias_flag=True)
    return args, kw


def _compare_with_fixture(out, o, tag):
    temperature, min_den = float(o["temperature"]), float(o["min_den"])
    line = TOL_INTERMEDIATE / temperature / min_den
    err = float(np.abs(out["probs"].cpu().numpy().astype(np.float64) - o["probs"]).max())
    print(f"{tag}: probs {err:.3e} (line {line:g}), golden margin {float(o['min_margin']):.2e}, min den {min_den:.3f}")
    assert float(o["min_margin"]) >= MARGIN and min_den >= 0.25
    assert out["S"].dtype == torch.int64 and out["S"].shape == o["S"].shape and out["probs"].shape == o["probs"].shape
    assert np.array_equal(out["decoding_order"].cpu().numpy(), o["decoding_order"])
    assert np.array_equal(out["S"].cpu().numpy(), o["S"])
    assert err <= line


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_AB"])
def test_reference_goldens(case, precision):
    g, o = load_golden(case), load_golden("tied_" + case)
    args, kw = _model_inputs(g, o)
    tied = [[int(k) for k in row if k >= 0] for row in o["tied_pos"]]
    with torch.no_grad():
        out = model_for(precision).tied_sample(*args, tied_pos=tied, tied_beta=torch.from_numpy(o["tied_beta"]), **kw)
    _compare_with_fixture(out, o, f"tied_{case}/{precision}")
    P = out["probs"].cpu().numpy()
    dead = np.zeros(len(g["S"]), bool)
    for grp in tied:
        dead[grp] = any(g["mask"][k] == 0 for k in grp)
    dead |= (g["mask"] == 0)
    assert ((P == 0).all(-1) == dead[None]).all()                  # exactly 0 only on dead groups
    assert all((out["S"][:, grp] == out["S"][:, grp[:1]]).all() for grp in tied)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sample_with_pssm_flags(precision):
    g, o = load_golden("syn_L32"), load_golden("sample_pssm_syn_L32")
    args, kw = _model_inputs(g, o)
    with torch.no_grad():
        out = model_for(precision).sample(*args, **kw)
    _compare_with_fixture(out, o, f"sample_pssm_syn_L32/{precision}")
    fixed = (o["free"] * g["mask"][None]) != 1
    assert (out["probs"].cpu().numpy()[fixed] == 0).all()
    # a position that is not free: its row is zeroed on the host as sample's :1376 has it, the letter is S_true
    kw["chain_M_pos"] = kw["chain_M_pos"].clone()
    kw["chain_M_pos"][:, ::4] = 0
    with torch.no_grad():
        part = model_for(precision).sample(*args, **kw)
    assert (part["probs"][:, ::4] == 0).all() and torch.equal(part["S"][:, ::4], args[2][:, ::4])
    assert float((part["probs"][:, 1::4].sum(-1) - 1).abs().max()) < 1e-5


# ---- masked layouts on the device's own graph ------------------------------------------------------------
MASKED = {"msk_L56_2ch": [[i, 28 + i] for i in range(28)],
          # a masked residue first ([0, 1]), in the middle ([6, 7, 8]) and last ([11, 12]); live groups and singletons
          "msk_L40": [[0, 1], [6, 7, 8], [11, 12], [2, 3], [14, 15, 16], [33, 34], [24, 37]]}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(MASKED))
def test_masked_layouts(name, precision):
    eng, p = engine(precision), protein(name)
    enc, _ = encode(eng, [p])
    ei, _ = checked_graph(name, enc.E_idx.cpu().numpy())
    L = len(p["S"])
    c = tied_chains(L, 3, 5, [MASKED[name]], fixed_every=4)
    temperature = 0.5
    ref = restate(p, c, temperature, ei, 6)
    res = run(eng, enc, c, temperature=temperature)
    against_restatement(res, ref, temperature, f"{name}/{precision}")
    n_dead = check_groups(res, c, p["mask"])
    assert n_dead >= 3 * 3
    if name == "msk_L40":
        S = res["S"].cpu().numpy()
        assert np.array_equal(S[:, [0, 1]], c["S_fixed"][:, [0, 0]]) and np.array_equal(S[:, [6, 7, 8]], c["S_fixed"][:, [7, 7, 7]])
        assert np.array_equal(S[:, [11, 12]], c["S_fixed"][:, [12, 12]])


# ---- other forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_k30_and_groupings(precision):
    """K = 30 and K = 48; within one workgroup the four chains are untied, in pairs, with the triple, and all in groups of four."""
    p = golden_protein("syn_L32")
    groupings = [[], [[i, 16 + i] for i in range(16)], [[i, 16 + i] for i in range(10)] + [[10, 11, 27]], groups_of_four(32)]
    for K in (30, 48):
        eng = engine(precision, K)
        enc, _ = encode(eng, [p])
        ei = enc.E_idx.cpu().numpy()
        Keff = min(K, 32)
        assert (ei[:, Keff:] == -1).all() and (ei[:, :Keff] >= 0).all()
        c = tied_chains(32, 4, 21, groupings)
        assert [int(c["close"][n].sum()) for n in range(4)] == [32, 16, 20, 8]
        ref = restate(p, c, 1.0, ei[:, :Keff], 8)
        res = run(eng, enc, c)
        against_restatement(res, ref, 1.0, f"K{K}/{precision}")
        assert check_groups(res, c, p["mask"]) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pssm_tables_against_restatement(precision):
    """Tied pairs with every table at once (bias, allowed, pssm_mix / pssm_bias, pssm_keep) against the restatement; the tables are
    read at the closing member."""
    eng, p = engine(precision), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    c = tied_chains(32, 3, 17, [[[i, 16 + i] for i in range(16)]], fixed_every=5)
    rng = np.random.default_rng(3)
    temperature = 0.7
    tables = dict(bias=(rng.normal(size=(32, 21)) * 0.5).astype(np.float32), allowed=np.ones((32, 21), np.float32),
                  pssm_mix=(0.3 * rng.random(32)).astype(np.float32), pssm_bias=rng.dirichlet(np.ones(21), 32).astype(np.float32),
                  pssm_keep=np.ones((32, 21), np.float32))
    for t in range(32):
        tables["allowed"][t, rng.permutation(21)[:2]] = 0
        tables["pssm_keep"][t, rng.permutation(21)[:3]] = 0
    ref = restate(p, c, temperature, enc.E_idx.cpu().numpy()[:, :32], 4, **tables)
    assert ref["min_den"] >= 0.25
    res = run(eng, enc, c, temperature=temperature, **tables)
    against_restatement(res, ref, temperature, f"tables/{precision}", renormalised=True)
    S = res["S"].cpu().numpy()
    closing_free = c["free"][:, 16:] == 1
    assert (tables["allowed"][np.nonzero(closing_free)[1] + 16, S[:, 16:][closing_free]] == 1).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_untied_equivalence(precision):
    """close all ones, no optional tables: Engine.sample's letters and free rows bit for bit; fixed unmasked rows get their probs."""
    eng, p = engine(precision), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    c = tied_chains(32, 33, 44, [[]], fixed_every=9)
    assert (c["close"] == 1).all()
    c["weight"] = None
    tied = run(eng, enc, c)
    plain = eng.sample(enc, c["order"], c["S_fixed"], c["free"], c["u"])
    assert torch.equal(tied["S"], plain["S"])
    is_free = torch.as_tensor(c["free"] == 1, device="cuda:0")
    assert torch.equal(tied["probs"][is_free], plain["probs"][is_free])
    assert bool((plain["probs"][~is_free] == 0).all())
    assert float((tied["probs"][~is_free].sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_independence(precision):
    """N = 33 tied chains, groupings varying by chain: two full workgroups and a tail of one. A chain has the same bits alone, in
    another slot, under three chunks and in a rerun."""
    eng, p = engine(precision), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    groupings = [[], [[i, 16 + i] for i in range(16)], [[i, 16 + i] for i in range(10)] + [[10, 11, 27]], groups_of_four(32), [[3, 30], [7, 8, 9, 10, 11]]]
    c = tied_chains(32, 33, 45, groupings, fixed_every=9)
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
    assert check_groups(full, c, p["mask"]) == 0
    assert len({tuple(r) for r in full["S"].cpu().numpy().tolist()}) > 16


@pytest.mark.parametrize("precision", PRECISIONS)
def test_weights(precision):
    eng, p = engine(precision), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    # weight = 1 on singletons is weight = None, bit for bit
    c = tied_chains(32, 3, 51, [[]])
    assert (c["weight"] == 1).all()
    ones = run(eng, enc, c)
    none = run(eng, enc, dict(c, weight=None))
    assert torch.equal(ones["S"], none["S"]) and torch.equal(ones["probs"], none["probs"])
    # a negative beta on the second member of every pair: the restatement's distribution, and not the all-ones one
    pairs = [[i, 16 + i] for i in range(16)]
    betas = np.ones(32, np.float32)
    betas[16:] = -0.5
    neg = tied_chains(32, 3, 52, [pairs], betas=betas)
    assert (neg["weight"][:, :16] == 0.5).all() and (neg["weight"][:, 16:] == -0.25).all()
    ref = restate(p, neg, 1.0, enc.E_idx.cpu().numpy()[:, :32], 9)
    res = run(eng, enc, neg)
    against_restatement(res, ref, 1.0, f"negative beta/{precision}")
    pos = run(eng, enc, dict(neg, weight=np.full((3, 32), 0.5, np.float32)))
    assert float((pos["probs"] - res["probs"]).abs().max()) > 1e-2


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch():
    from thermompnn_amd._lib import TmpnnError
    eng, p = engine("f16x2"), golden_protein("syn_L32")
    enc, _ = encode(eng, [p])
    c = tied_chains(32, 2, 3, [[[i, 16 + i] for i in range(16)]])
    eng._status.copy_(torch.full((1,), 77, dtype=torch.int32, device="cuda:0"))
    open_end = dict(c, close=c["close"].copy())
    open_end["close"][1, -1] = 0
    with pytest.raises(TmpnnError, match="close"):
        run(eng, enc, open_end)
    twos = dict(c, close=c["close"].copy())
    twos["close"][0, 3] = 2
    with pytest.raises(TmpnnError, match="close must hold 0 or 1"):
        run(eng, enc, twos)
    with pytest.raises(TmpnnError, match="close"):
        run(eng, enc, dict(c, close=c["close"][:, :31]))
    with pytest.raises(TmpnnError, match="weight"):
        run(eng, enc, dict(c, weight=c["weight"][:1]))
    with pytest.raises(TmpnnError, match="pssm_keep"):
        run(eng, enc, c, pssm_keep=np.ones((32, 20), np.float32))
    with pytest.raises(TmpnnError, match="pssm_mix"):
        run(eng, enc, c, pssm_mix=np.ones((31,), np.float32), pssm_bias=np.ones((32, 21), np.float32))
    with pytest.raises(TmpnnError, match="pssm_bias goes with pssm_mix"):
        run(eng, enc, c, pssm_bias=np.ones((32, 21), np.float32))
    with pytest.raises(TmpnnError, match="pssm_bias goes with pssm_mix"):
        run(eng, enc, c, pssm_mix=np.ones((32,), np.float32))
    bad = dict(c, order=c["order"].copy())
    bad["order"][1, 5] = bad["order"][1, 6]
    with pytest.raises(TmpnnError, match="permutation"):
        run(eng, enc, bad)
    letters = dict(c, S_fixed=c["S_fixed"].copy())
    letters["S_fixed"][0, 0] = 21
    with pytest.raises(TmpnnError, match="residue indices"):
        run(eng, enc, letters)
    with pytest.raises(TmpnnError, match="temperature"):
        run(eng, enc, c, temperature=0.0)
    assert int(eng._status.item()) == 77                    # tmpnn_sample_tied zeroes the word on the stream first: it never ran
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    fp32 = Engine(synthetic_state_dict(0), "cuda:0", 48, precision="fp32", retry_precision=None)
    with pytest.raises(TmpnnError, match="bf16x3"):
        run(fp32, encode(fp32, [p])[0], c)


# ---- the range contract --------------------------------------------------------------------------------------------
def test_range_overflow_raises_or_retries(synthetic_weights):
    """Weights scaled as test_gpu_sample.test_range_overflow_raises_or_retries scales them: the f16x2 tied sampler raises without a
    retry precision; with one it warns and returns the bf16x3 result, bit for bit what a direct bf16x3 call gives."""
    from thermompnn_amd._lib import TmpnnRangeError
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    p = golden_protein("syn_L32")
    c = tied_chains(32, 2, 9, [[[i, 16 + i] for i in range(16)]])
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
