"""Sampling for many backbones in one launch (Engine.sample_each / sample_tied_each, tmpnn_sample_each): four different proteins
packed into one context (T = 145); every (protein, chain) result is bit for bit what Engine.sample gives for that protein encoded
alone — which carries the reference parity test_gpu_sample.py pins for the solo call — and does not depend on the packing order,
the launch order, the chunking or a rerun; the tied form against solo sample_tied; argument errors before any launch; the range
contract; the module's padded batch of different members."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from masked_backbones import pack, protein
from test_gpu_sample import TOL_INTERMEDIATE, chains, encode, engine, golden_protein, model_for
from test_gpu_tied_sample import groups_of_four, tied_chains

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x2", "bf16x3"]
NAMES = ["syn_L32", "msk_L17", "msk_L40", "msk_L56_2ch"]
TEMPERATURE = 0.7
KEYS = ("order", "close", "S_fixed", "free", "u", "weight")
_CACHE = {}


def proteins(names=NAMES):
    return [golden_protein(n) if n.startswith("syn") else protein(n) for n in names]


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def packed_enc(precision, names=NAMES):
    return cached(("enc", precision, tuple(names)), lambda: encode(engine(precision), proteins(names)))


def solo_enc(precision, name):
    return cached(("solo", precision, name), lambda: encode(engine(precision), proteins([name]))[0])


def tables(names, seed=2):
    """Per-protein bias / allowed tables [L,21] (the letter 20 biased away, a fifth of the letters disallowed, letter 0 always allowed)."""
    rng, out = np.random.default_rng(seed), []
    for p in proteins(names):
        L = len(p["S"])
        bias = (rng.normal(size=(L, 21)) * 0.5).astype(np.float32)
        bias[:, 20] -= 1e8
        allowed = (rng.random((L, 21)) > 0.2).astype(np.float32)
        allowed[:, 0] = 1
        out.append(dict(bias=bias, allowed=allowed))
    return out


def join(local, starts):
    """Per-protein chain dicts (local indices) -> one dict over the packed axis: orders shifted by the protein's first row."""
    out = {}
    for k in KEYS:
        if k in local[0]:
            out[k] = np.concatenate([c[k] + (starts[b] if k == "order" else 0) for b, c in enumerate(local)], axis=1)
    return out


def each_case(names, N, seed=50, fixed_every=5):
    ps = proteins(names)
    local = [chains(len(p["S"]), N, seed + b, fixed_every=fixed_every) for b, p in enumerate(ps)]
    starts = np.concatenate([[0], np.cumsum([len(p["S"]) for p in ps])])
    return local, join(local, starts), starts


def run_each(eng, enc, c, **kw):
    return eng.sample_each(enc, c["order"], c["S_fixed"], c["free"], c["u"], **kw)


def run_solo(eng, enc, c, **kw):
    return eng.sample(enc, c["order"], c["S_fixed"], c["free"], c["u"], **kw)


def cat_tables(tabs, key):
    return np.concatenate([t[key] for t in tabs])


def solo_results(precision, N):
    """Engine.sample on every protein of NAMES encoded alone, with the chains of each_case(NAMES, N) and the tables of tables(NAMES)."""
    def make():
        eng, (local, _, _), tabs = engine(precision), each_case(NAMES, N), tables(NAMES)
        return [run_solo(eng, solo_enc(precision, n), local[b], temperature=TEMPERATURE, bias=tabs[b]["bias"], allowed=tabs[b]["allowed"])
                for b, n in enumerate(NAMES)]
    return cached(("solo_res", precision, N), make)


def full_result(precision, N):
    def make():
        eng, (enc, _), (_, c, _), tabs = engine(precision), packed_enc(precision), each_case(NAMES, N), tables(NAMES)
        return run_each(eng, enc, c, temperature=TEMPERATURE, bias=cat_tables(tabs, "bias"), allowed=cat_tables(tabs, "allowed"))
    return cached(("full", precision, N), make)


def assert_segments_equal(res, solos, starts, order=None, tag=""):
    """Protein b's segment of the packed result equals the b-th solo result bit for bit (``order``: packed slot -> solo index)."""
    for slot in range(len(starts) - 1):
        b = slot if order is None else order[slot]
        t0, t1 = int(starts[slot]), int(starts[slot + 1])
        assert torch.equal(res["S"][:, t0:t1], solos[b]["S"]), (tag, slot)
        assert torch.equal(res["probs"][:, t0:t1], solos[b]["probs"]), (tag, slot)


# ---- bits equal the solo call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", [1, 3, 17])
def test_bits_equal_the_solo_call(N, precision):
    (_, pk), (_, c, starts) = packed_enc(precision), each_case(NAMES, N)
    assert pk["X"].shape[0] == 145
    res, solos = full_result(precision, N), solo_results(precision, N)
    assert_segments_equal(res, solos, starts, tag=f"N{N}/{precision}")
    mask = pk["mask"].cpu().numpy()
    is_free = torch.as_tensor(c["free"] * mask[None] == 1, device="cuda:0")
    assert int(is_free.sum()) > 50 * N and bool((res["probs"][~is_free] == 0).all())
    assert float((res["probs"][is_free].sum(-1) - 1).abs().max()) < 1e-5
    if N > 1:
        assert not torch.equal(res["S"][0], res["S"][1])                     # the orders matter


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reference_golden_as_one_member(precision):
    """The 2OCJ_A_gap fixture of the imported reference as the middle member of three, with its recorded uniforms: the reference's
    letters, its probabilities within the solo test's line."""
    from thermompnn_amd.protein_mpnn_utils import pack_sample_args
    g, o = load_golden("2OCJ_A_gap"), load_golden("sample_2OCJ_A_gap")
    temperature = float(o["temperature"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n_all = o["randn"].shape[0]
    mask_rep = t(np.tile(g["mask"], (n_all, 1)))
    pk = pack_sample_args(t(o["randn"]), t(o["chain_mask"]), mask_rep, temperature, o["omit_AAs"], o["bias_AAs"], t(o["chain_M_pos"]),
                          t(o["omit_AA_mask"]) if "omit_AA_mask" in o else None, t(o["bias_by_res"]))
    assert np.array_equal(pk["decoding_order"].numpy(), o["decoding_order"])
    same = all(v is None or bool((v[1:] == v[:1]).all()) for v in (pk["bias"], pk["allowed"]))
    N = n_all if same else 1                                              # one table set per protein: chains that share member 0's
    gold = dict(order=pk["decoding_order"].numpy()[:N], S_fixed=o["S_true"][:N].astype(np.int64), free=pk["free"].numpy()[:N],
                u=o["u"][:N].astype(np.float32))
    L = len(g["S"])
    members = [golden_protein("syn_L32"), golden_protein("2OCJ_A_gap"), protein("msk_L17")]
    local = [chains(32, N, 70), gold, chains(17, N, 71)]
    starts = np.concatenate([[0], np.cumsum([32, L, 17])])
    c = join(local, starts)
    T = int(starts[-1])
    bias, allowed = np.zeros((T, 21), np.float32), np.ones((T, 21), np.float32)
    bias[32:32 + L] = pk["bias"][0].numpy()
    if pk["allowed"] is not None:
        allowed[32:32 + L] = pk["allowed"][0].numpy()
    eng = engine(precision)
    enc, _ = encode(eng, members)
    res = run_each(eng, enc, c, temperature=temperature, bias=bias, allowed=allowed)
    S, probs = res["S"][:, 32:32 + L].cpu().numpy(), res["probs"][:, 32:32 + L].cpu().numpy().astype(np.float64)
    err = float(np.abs(probs - o["probs"][:N]).max())
    print(f"2OCJ_A_gap as a member/{precision}: {N} chain(s), probs {err:.3e} (line {TOL_INTERMEDIATE / temperature:g})")
    assert np.array_equal(S, o["S"][:N])
    assert err <= TOL_INTERMEDIATE / temperature


# ---- independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_independent_of_packing_chunking_and_rerun(precision):
    N = 17
    eng, (enc, _), (local, c, starts), tabs = engine(precision), packed_enc(precision), each_case(NAMES, N), tables(NAMES)
    full, solos = full_result(precision, N), solo_results(precision, N)
    kw = dict(temperature=TEMPERATURE, bias=cat_tables(tabs, "bias"), allowed=cat_tables(tabs, "allowed"))
    again = run_each(eng, enc, c, **kw)
    assert torch.equal(again["S"], full["S"]) and torch.equal(again["probs"], full["probs"])
    # the proteins packed in another order
    perm = [2, 0, 3, 1]
    names = [NAMES[i] for i in perm]
    enc2, _ = packed_enc(precision, names)
    lens = [len(p["S"]) for p in proteins(names)]
    starts2 = np.concatenate([[0], np.cumsum(lens)])
    moved = run_each(eng, enc2, join([local[i] for i in perm], starts2), temperature=TEMPERATURE,
                     bias=cat_tables([tabs[i] for i in perm], "bias"), allowed=cat_tables([tabs[i] for i in perm], "allowed"))
    assert_segments_equal(moved, solos, starts2, order=perm, tag="moved")
    # max_rows that split the proteins into several ranges (17 chains of 49 = 32 + 17 rows; of 40; of 56), then one protein's chains
    from thermompnn_amd.engine import plan_each_chunks
    for max_rows in (17 * 49, 17 * 56, 5 * 56, 40):
        plan = plan_each_chunks(starts.tolist(), N, max_rows)
        got = run_each(eng, enc, c, max_rows=max_rows, **kw)
        assert torch.equal(got["S"], full["S"]) and torch.equal(got["probs"], full["probs"]), max_rows
        assert len(plan) > 1
    assert len({(p0, p1) for p0, p1, _, _ in plan_each_chunks(starts.tolist(), N, 17 * 49)}) == 3
    assert len({(n0, n1) for _, _, n0, n1 in plan_each_chunks(starts.tolist(), N, 5 * 56)}) > 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_launch_order_through_the_c_entry(precision):
    """tmpnn_sample_each with sched given (longest first), NULL and reversed; and a protein sub-range whose scratch is its own rows."""
    from thermompnn_amd.engine import _ptr, _stream, each_schedule
    N = 3
    eng, (enc, _), (_, c, starts), tabs = engine(precision), packed_enc(precision), each_case(NAMES, N), tables(NAMES)
    full = full_result(precision, N)
    T, P, offs = 145, 4, starts.tolist()
    O, S0, Fr, U = eng._i32(c["order"]), eng._i32(c["S_fixed"]), eng._f32(c["free"]), eng._f32(c["u"])
    B, A = eng._f32(cat_tables(tabs, "bias")), eng._f32(cat_tables(tabs, "allowed"))
    longest_first = each_schedule(offs, 0, P)
    assert longest_first.tolist() == [3, 2, 0, 1]

    def call(p0, p1, sched):
        S = torch.full((N, T), -1, dtype=torch.int32, device="cuda:0")
        probs = torch.full((N, T, 21), -1.0, device="cuda:0")
        rows = offs[p1] - offs[p0]
        ws = torch.empty(eng.lib.tmpnn_sample_each_workspace_bytes(rows, N), dtype=torch.uint8, device="cuda:0")
        sd = None if sched is None else torch.tensor(sched, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = eng.lib.tmpnn_sample_each(eng.w.handle, _ptr(enc.ctx), enc.ctx.numel(), _ptr(enc.mask), T, _ptr(enc.offsets), P, p0, p1,
                                       offs[p0], rows, _ptr(sd), N, _ptr(O), _ptr(S0), _ptr(Fr), _ptr(U), 1.0 / TEMPERATURE, _ptr(B),
                                       _ptr(A), _ptr(S), _ptr(probs), _ptr(status), _ptr(ws), ws.numel(), _stream())
        assert rc == 0 and int(status.item()) == 0
        return S, probs

    for sched in (longest_first.tolist(), None, longest_first.tolist()[::-1]):
        S, probs = call(0, P, sched)
        assert torch.equal(S, full["S"]) and torch.equal(probs, full["probs"]), sched
    S, probs = call(1, 3, [2, 1])                                         # rows [32, 89) only: the others keep the fill
    assert torch.equal(S[:, 32:89], full["S"][:, 32:89]) and torch.equal(probs[:, 32:89], full["probs"][:, 32:89])
    assert bool((S[:, :32] == -1).all()) and bool((S[:, 89:] == -1).all()) and bool((probs[:, 89:] == -1).all())


# ---- tied --------------------------------------------------------------------------------------------------------------
def tied_case(names, N, seed=80):
    ps = proteins(names)
    local = []
    for b, p in enumerate(ps):
        L = len(p["S"])
        pairs = [[i, L - 1 - i] for i in range(0, L // 2, 3)]
        betas = np.random.default_rng(seed + 10 + b).uniform(0.5, 1.5, L).astype(np.float32)
        local.append(tied_chains(L, N, seed + b, [groups_of_four(L), pairs, []], fixed_every=6, betas=betas))
    starts = np.concatenate([[0], np.cumsum([len(p["S"]) for p in ps])])
    return local, join(local, starts), starts


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tied_equals_solo_sample_tied(precision):
    N = 4
    eng, (enc, _), (local, c, starts), tabs = engine(precision), packed_enc(precision), tied_case(NAMES, N), tables(NAMES)
    rng = np.random.default_rng(12)
    pssm = []
    for p in proteins(NAMES):
        L = len(p["S"])
        pb = rng.random((L, 21)).astype(np.float32)
        pssm.append(dict(pssm_mix=(rng.random(L) * 0.4).astype(np.float32), pssm_bias=pb / pb.sum(-1, keepdims=True),
                         pssm_keep=(rng.random((L, 21)) > 0.3).astype(np.float32)))
    for with_pssm in (False, True):
        extra = (lambda b: pssm[b]) if with_pssm else (lambda b: {})
        kw = dict(temperature=TEMPERATURE, bias=cat_tables(tabs, "bias"), allowed=cat_tables(tabs, "allowed"))
        if with_pssm:
            kw.update({k: np.concatenate([t[k] for t in pssm]) for k in pssm[0]})
        res = eng.sample_tied_each(enc, c["order"], c["close"], c["S_fixed"], c["free"], c["u"], weight=c["weight"], **kw)
        solos = [eng.sample_tied(solo_enc(precision, n), local[b]["order"], local[b]["close"], local[b]["S_fixed"], local[b]["free"],
                                 local[b]["u"], weight=local[b]["weight"], temperature=TEMPERATURE, bias=tabs[b]["bias"],
                                 allowed=tabs[b]["allowed"], **extra(b)) for b, n in enumerate(NAMES)]
        assert_segments_equal(res, solos, starts, tag=f"tied/{precision}/pssm={with_pssm}")
        split = eng.sample_tied_each(enc, c["order"], c["close"], c["S_fixed"], c["free"], c["u"], weight=c["weight"], max_rows=2 * 56, **kw)
        assert torch.equal(split["S"], res["S"]) and torch.equal(split["probs"], res["probs"])
    S = res["S"].cpu().numpy()
    assert (S[0, [0, 1, 2, 3]] == S[0, 0]).all() and (S[0, 32:36] == S[0, 32]).all()       # chain 0: groups of four, in every protein


@pytest.mark.parametrize("precision", PRECISIONS)
def test_tied_with_close_all_ones_is_sample_each(precision):
    N = 3
    eng, (enc, pk), (_, c, _) = engine(precision), packed_enc(precision), each_case(NAMES, N)
    untied = run_each(eng, enc, c, temperature=TEMPERATURE)
    tied = eng.sample_tied_each(enc, c["order"], np.ones_like(c["order"]), c["S_fixed"], c["free"], c["u"], temperature=TEMPERATURE)
    assert torch.equal(tied["S"], untied["S"])
    is_free = torch.as_tensor(c["free"] * pk["mask"].cpu().numpy()[None] == 1, device="cuda:0")
    assert torch.equal(tied["probs"][is_free], untied["probs"][is_free])


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch():
    from thermompnn_amd._lib import TmpnnError
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    eng, (enc, _), (_, c, starts) = engine("f16x2"), packed_enc("f16x2"), each_case(NAMES, 2)
    _, ct, _ = tied_case(NAMES, 2)
    tied = lambda d, **kw: eng.sample_tied_each(enc, d["order"], d["close"], d["S_fixed"], d["free"], d["u"], **kw)
    eng._status.copy_(torch.full((1,), 77, dtype=torch.int32, device="cuda:0"))
    spans = dict(ct, close=ct["close"].copy())
    spans["close"][1, 31] = 0                                            # protein 0's last step stays open: its group would run into protein 1
    with pytest.raises(TmpnnError, match="last step must close"):
        tied(spans)
    wrong = dict(c, order=c["order"].copy())
    wrong["order"][1, [5, 40]] = wrong["order"][1, [40, 5]]              # still a permutation of 0..144, two entries in the wrong protein
    with pytest.raises(TmpnnError, match="inside the protein"):
        run_each(eng, enc, wrong)
    with pytest.raises(TmpnnError, match="inside the protein"):
        tied(dict(ct, order=wrong["order"]))
    twice = dict(c, order=c["order"].copy())
    twice["order"][0, 5] = twice["order"][0, 6]
    with pytest.raises(TmpnnError, match="permutation"):
        run_each(eng, enc, twice)
    letters = dict(c, S_fixed=c["S_fixed"].copy())
    letters["S_fixed"][0, 0] = 21
    with pytest.raises(TmpnnError, match="residue indices"):
        run_each(eng, enc, letters)
    with pytest.raises(TmpnnError, match="temperature"):
        run_each(eng, enc, c, temperature=0.0)
    with pytest.raises(TmpnnError, match="order"):
        run_each(eng, enc, dict(c, u=c["u"][:, :144]))
    with pytest.raises(TmpnnError, match="bias"):
        run_each(eng, enc, c, bias=np.zeros((32, 21), np.float32))
    assert int(eng._status.item()) == 77                    # the entry zeroes the word on the stream first: it never ran
    fp32 = Engine(synthetic_state_dict(0), "cuda:0", 48, precision="fp32", retry_precision=None)
    fp32._status.copy_(torch.full((1,), 77, dtype=torch.int32, device="cuda:0"))
    enc32 = encode(fp32, proteins(NAMES[:2]))[0]
    fp32._status.copy_(torch.full((1,), 77, dtype=torch.int32, device="cuda:0"))
    _, c2, _ = each_case(NAMES[:2], 2)
    with pytest.raises(TmpnnError, match="bf16x3"):
        run_each(fp32, enc32, c2)
    assert int(fp32._status.item()) == 77


# ---- the range contract --------------------------------------------------------------------------------------------
def test_range_overflow_raises_or_retries(synthetic_weights):
    from thermompnn_amd._lib import TmpnnRangeError
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    names = NAMES[:2]
    _, c, _ = each_case(names, 2)
    direct = Engine(W, "cuda:0", 48, precision="bf16x3", retry_precision=None)
    want = run_each(direct, encode(direct, proteins(names))[0], c)
    assert bool(torch.isfinite(want["probs"]).all())
    strict = Engine(W, "cuda:0", 48, precision="f16x2", retry_precision=None)
    with pytest.raises(TmpnnRangeError):
        run_each(strict, encode(strict, proteins(names))[0], c)
    eng = Engine(W, "cuda:0", 48, precision="f16x2")
    enc = encode(eng, proteins(names))[0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run_each(eng, enc, c, max_rows=2 * 32)
    assert any("bf16x3" in str(w.message) for w in rec)
    assert all(w.category is RuntimeWarning and w.filename == __file__ for w in rec if "bf16x3" in str(w.message))     # attributed to the caller
    assert torch.equal(got["S"], want["S"]) and torch.equal(got["probs"], want["probs"])


# ---- the module: a padded batch of different members ---------------------------------------------------------------------
def padded_members(names, L):
    ps = proteins(names)
    B = len(ps)
    X, mask = np.zeros((B, L, 4, 3), np.float32), np.zeros((B, L), np.float32)
    S, ridx, cenc = np.zeros((B, L), np.int64), np.zeros((B, L), np.int64), np.zeros((B, L), np.int64)
    for b, p in enumerate(ps):
        n = len(p["S"])
        X[b, :n], mask[b, :n], S[b, :n], cenc[b, :n] = p["X"], p["mask"], p["S"], p["cenc"]
        ridx[b, :n] = p["ridx"]
        ridx[b, n:] = -100                                              # tied_featurize's padding value
    t = lambda a: torch.from_numpy(a).to("cuda:0")
    return t(X), t(S), t(mask), t(ridx), t(cenc)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_module_sample_on_different_members(precision):
    names, L = ["syn_L32", "msk_L17", "msk_L40"], 40
    B = len(names)
    X, S, mask, ridx, cenc = padded_members(names, L)
    rng = np.random.default_rng(4)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dt)
    randn, u = t(rng.normal(size=(B, L))), t(rng.random((B, L)))
    chain_mask = mask.clone()
    chain_mask[:, ::6] = 0
    by_res = t(rng.normal(size=(B, L, 21)) * 0.3)
    omit = t((rng.random((B, L, 21)) > 0.85).astype(np.float32))
    omit[..., 0] = 0
    m = model_for(precision)
    kw = dict(temperature=TEMPERATURE, omit_AAs_np=np.eye(21)[20], bias_AAs_np=np.zeros(21))
    with torch.no_grad():
        out = m.sample(X, randn, S, chain_mask, cenc, ridx, mask=mask, omit_AA_mask=omit, bias_by_res=by_res, uniforms=u, **kw)
        assert out["S"].shape == (B, L) and out["S"].dtype == torch.int64 and out["probs"].shape == (B, L, 21)
        for b in range(B):
            one = m.sample(X[b:b + 1], randn[b:b + 1], S[b:b + 1], chain_mask[b:b + 1], cenc[b:b + 1], ridx[b:b + 1], mask=mask[b:b + 1],
                           omit_AA_mask=omit[b:b + 1], bias_by_res=by_res[b:b + 1], uniforms=u[b:b + 1], **kw)
            assert torch.equal(out["S"][b], one["S"][0]) and torch.equal(out["probs"][b], one["probs"][0]), b
            assert torch.equal(out["decoding_order"][b], one["decoding_order"][0])
    assert len({tuple(r) for r in out["S"].cpu().numpy().tolist()}) == B


@pytest.mark.parametrize("precision", PRECISIONS)
def test_module_tied_sample_on_different_members(precision):
    from thermompnn_amd import weights
    from thermompnn_amd.design import ProteinMPNNDesign
    # (tied_sample regroups member 0's decoding order for EVERY member, and that order puts member 0's masked residues first: the
    # one-member calls reproduce it when the members share the mask layout — here one backbone as one chain and cut into two)
    names, L = ["msk_L56", "msk_L56_2ch"], 56
    B = len(names)
    X, S, mask, ridx, cenc = padded_members(names, L)
    assert torch.equal(mask[0], mask[1]) and not torch.equal(cenc[0], cenc[1]) and not torch.equal(ridx[0], ridx[1])
    m = ProteinMPNNDesign(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
    m.load_state_dict(weights.split_transfer_state_dict(weights.synthetic_state_dict(0))[0])
    m.precision, m.retry_precision = precision, None
    m = m.eval().cuda()
    rng = np.random.default_rng(5)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dt)
    randn, u = t(np.tile(rng.normal(size=(1, L)), (B, 1))), t(rng.random((B, L)))      # (the order is member 0's for every member)
    by_res = t(rng.normal(size=(B, L, 21)) * 0.3)
    kw = dict(temperature=TEMPERATURE, omit_AAs_np=np.eye(21)[20], bias_AAs_np=np.zeros(21), tied_pos=[[i, i + 16] for i in range(1, 15, 2)],
              tied_beta=t(np.ones(L)))
    with torch.no_grad():
        out = m.tied_sample(X, randn, S, mask.clone(), cenc, ridx, mask=mask, bias_by_res=by_res, uniforms=u, **kw)
        for b in range(B):
            one = m.tied_sample(X[b:b + 1], randn[b:b + 1], S[b:b + 1], mask[b:b + 1].clone(), cenc[b:b + 1], ridx[b:b + 1], mask=mask[b:b + 1],
                                bias_by_res=by_res[b:b + 1], uniforms=u[b:b + 1], **kw)
            assert torch.equal(out["decoding_order"][b], one["decoding_order"][0])
            assert torch.equal(out["S"][b], one["S"][0]) and torch.equal(out["probs"][b], one["probs"][0]), b
    assert not torch.equal(out["S"][0], out["S"][1])


# ---- the driver ------------------------------------------------------------------------------------------------------------
def test_design_scan_driver(tmp_path):
    """design_scan on two files: 2 x (1 + 3) records, the sequences of an Engine.sample_each call built from the same seed, masked
    residues written as X, every score the mean -log p of decode_ordered under the sampler's orders."""
    from conftest import GOLDEN
    import os
    from thermompnn_amd import design_scan as ds
    from thermompnn_amd.native_pdb import parse_pdbs
    paths = [os.path.join(GOLDEN, "2OCJ.pdb"), os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb")]
    out = tmp_path / "designs.fa"
    assert ds.main([*paths, "--chain", "A", "--num_seq", "3", "--synthetic_weights", "0", "--seed", "1", "--out", str(out)]) == 0
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 2 * 2 * (1 + 3) + 1
    heads, seqs = lines[0:-1:2], lines[1:-1:2]
    assert all(h.startswith(">") for h in heads) and [h.split(",")[0] for h in heads] == [">2OCJ"] * 4 + [">2OCJ_gap_chainA"] * 4
    # the same call built by hand
    entries = parse_pdbs(paths, ["A", "A"])
    gen = torch.Generator().manual_seed(1)
    local = [ds.draw_chains(e, 3, [], gen) for e in entries]
    c = ds.join_chains(local)
    eng = engine("f16x2")
    cat = lambda k: np.concatenate([e[k] for e in entries])
    starts = np.concatenate([[0], np.cumsum([len(e["S"]) for e in entries])])
    enc = eng.encode(cat("X"), cat("mask"), cat("residue_idx"), cat("chain_enc"), torch.tensor(starts, dtype=torch.int32))
    bias = np.zeros((int(starts[-1]), 21), np.float32)
    bias[:, 20] = -1e8
    res = eng.sample_each(enc, c["order"], c["S_fixed"], c["free"], c["u"], temperature=0.1, bias=bias)
    lp = eng.decode_ordered(enc, res["S"], ds.ranks_of(torch.as_tensor(c["order"], device="cuda:0")))["log_probs"].double().cpu().numpy()
    S = res["S"].cpu().numpy()
    assert sum(int((e["mask"] == 0).sum()) for e in entries) > 0
    for b, e in enumerate(entries):
        t0, t1 = int(starts[b]), int(starts[b + 1])
        live = e["mask"] > 0
        assert seqs[4 * b] == ds.letters(e["S"], e["mask"]) and f"L={t1 - t0}" in heads[4 * b] and "native" in heads[4 * b]
        for k in range(3):
            head, seq = heads[4 * b + 1 + k], seqs[4 * b + 1 + k]
            assert seq == ds.letters(S[k, t0:t1], e["mask"]), (b, k)
            assert all(ch == "X" for ch, m in zip(seq, live) if not m) and "X" not in "".join(ch for ch, m in zip(seq, live) if m)
            fields = dict(f.strip().split("=") for f in head.split(",")[1:])
            assert fields["sample"] == str(k + 1) and fields["T"] == "0.1" and fields["seed"] == "1"
            want = -lp[k, np.arange(t0, t1), S[k, t0:t1]][live].mean()
            print(f"{heads[4 * b]} sample {k + 1}: score {fields['score']} against {want:.7f}, recovery {fields['seq_recovery']}")
            assert abs(float(fields["score"]) - want) <= 1e-6
            rec = float((S[k, t0:t1] == e["S"])[live].mean())
            assert abs(float(fields["seq_recovery"]) - rec) <= 1e-4
    assert len(set(seqs)) == 8                                           # eight different sequences
