"""The C-alpha-only flavour on the GPU (tmpnn_graph_ca.hip behind tmpnn_weights_create_ca): frames, the featurizer stage at every
precision, ProteinMPNN(ca_only=True).forward, every decoder over one encoder state, batch independence, and the full-backbone path
left alone. Fixtures: tests/golden/make_ca_golden.py (the imported reference in float32 and float64).

The featurizer is judged edge by edge against FLOAT64. The fixtures hold the reference's float64 E on a few rows only (a whole E does
not fit a committed file); tests/ca_restatement.py reproduces those rows to 1e-12 (test_ca_host.py, and here once more) and stands for
the float64 featurizer on every edge. The quaternion's sign() and sqrt(|.|) make some edges ill-conditioned in fp32 for ANY
implementation — the self edge (R ~ I: radicands ~ 0) and pairs of parallel frames. An edge is well-conditioned when, in float64,
each of the three radicands, the three sign differences and 1 + tr R is exactly 0 or at least 1e-3 in magnitude:
  * well-conditioned edges meet TOL_INTERMEDIATE = 1e-5 outright;
  * the others: at most 2.5 x the reference-fp32's own largest distance from float64 on the same case (recorded in the fixture from the
    imported reference, never from the code under test) — the rule and factor of the README's parity row for the "hot" draws;
  * the ill-conditioned share of a case may not exceed 10 % of its valid edges.
Decoder states and log_probs: max(1e-5, 2.5 x the reference-fp32's distance from float64)."""
import numpy as np
import pytest
import torch

import ca_restatement as car
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5
F64_FACTOR = 2.5
ILL_CAP = 0.10
PRECISIONS = ["fp32", "f16x2", "bf16x3"]
SMALL = ["syn_L32", "syn_L40", "msk_L40", "msk_L56_2ch", "pad_L32_L40", "msk_L17", "msk_L47", "msk_L49"]
CASES = SMALL + ["2OCJ_A", "2OCJ_AB"]
_ENGINES, _MODELS, _TRUTH = {}, {}, {}


def ca_weights():
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, "mpnn_ca")


def engine(precision, K=48):
    from thermompnn_amd.engine import Engine
    if (precision, K) not in _ENGINES:
        _ENGINES[precision, K] = Engine(ca_weights(), "cuda:0", K, precision=precision, retry_precision=None)
        assert _ENGINES[precision, K].ca_only
    return _ENGINES[precision, K]


def model_for(precision, K=48):
    from thermompnn_amd.design import ProteinMPNNDesign
    if (precision, K) not in _MODELS:
        m = ProteinMPNNDesign(21, 128, 128, 128, k_neighbors=K, augment_eps=0.0, ca_only=True)
        r = m.load_state_dict(ca_weights(), strict=True)
        assert not r.missing_keys and not r.unexpected_keys
        m.precision, m.retry_precision = precision, None
        _MODELS[precision, K] = m.eval().cuda()
    return _MODELS[precision, K]


def truth(case):
    """The case's float64 featurizer output on every edge (the restatement, pinned to the reference's float64 rows), its
    well-conditioned edges and its frames. Computed once per case and left unchanged."""
    if case not in _TRUTH:
        g = load_golden("ca_" + case)
        W = ca_weights()
        t = torch.from_numpy
        E, well, O = [], [], []
        for b in range(g["S"].shape[0]):
            Ca, ei = t(g["Ca"][b]).double(), t(g["E_idx"][b].astype(np.int64))
            E.append(car.edge_features(W, Ca, t(g["mask"][b]).double(), t(g["residue_idx"][b].astype(np.int64)),
                                       t(g["chain_enc"][b].astype(np.int64)), ei).numpy())
            O.append(car.frames(Ca))
            well.append(car.well_conditioned(O[-1], ei).numpy())
        E = np.stack(E)
        assert float(np.abs(E[:, g["rows"]] - g["E64_rows"]).max()) <= 1e-12
        _TRUTH[case] = dict(g=g, E=E, well=np.stack(well), O=torch.stack(O).numpy())
    return _TRUTH[case]


def packed(g, dev="cuda:0"):
    """The padded fixture [B,L,...] as the engine takes it: B segments of L rows, X [B L,4,3] with C-alpha in slot 1."""
    B, L = g["S"].shape
    X = np.zeros((B * L, 4, 3), np.float32)
    X[:, 1] = g["Ca"].reshape(B * L, 3)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    return dict(X=t(X, torch.float32), S=t(g["S"].reshape(-1), torch.int32), mask=t(g["mask"].reshape(-1), torch.float32),
                ridx=t(g["residue_idx"].reshape(-1), torch.int32), cenc=t(g["chain_enc"].reshape(-1), torch.int32),
                offsets=torch.arange(B + 1, dtype=torch.int32) * L, B=B, L=L)


def global_graph(g):
    """The fixture's E_idx [B,L,Keff] as the engine's [B L,48]: global rows, -1 in the slots beyond Keff; and the k-NN's distances."""
    B, L, Keff = g["E_idx"].shape
    ei = np.full((B, L, 48), -1, np.int32)
    ei[:, :, :Keff] = g["E_idx"] + (np.arange(B) * L)[:, None, None]
    D = np.zeros((B, L, 48), np.float32)
    for b in range(B):
        t = torch.from_numpy
        D[b, :, :Keff] = car.masked_neighbor_distance(t(g["Ca"][b]), t(g["mask"][b]), t(g["E_idx"][b].astype(np.int64))).numpy()
    return ei.reshape(B * L, 48), D.reshape(B * L, 48)


# ---- 1. frames ---------------------------------------------------------------------------------------------------------------
def test_frames_packed_padded_and_short_segments():
    eng = engine("f16x2")
    t = torch.from_numpy
    # the packed pair: each protein a segment of its own length; the padded pair: two segments of 40 rows
    a, b = load_golden("ca_syn_L32"), load_golden("ca_msk_L40")
    Ca = np.concatenate([a["Ca"][0], b["Ca"][0]])
    X = np.zeros((72, 4, 3), np.float32)
    X[:, 1] = Ca
    O = eng.ca_frames(X, [0, 32, 72]).cpu()
    want = car.frames_packed(t(Ca).double(), [0, 32, 72])
    assert float((O.double() - want).abs().max()) <= 1e-6
    for s, e in ((0, 32), (32, 72)):
        assert bool((O[[s, e - 2, e - 1]] == 0).all())
    assert bool((O[1:30] != 0).any(-1).all())
    dead = [i for i in range(40) if (b["Ca"][0][i] == 0).all()]          # a missing C-alpha: the steps that touch it are zeroed
    assert dead and all(bool((O[32 + i] == 0).all()) and bool((want[32 + i] == 0).all()) for i in dead)
    assert bool(((want == 0).all(-1) == (O == 0).all(-1)).all())
    p = truth("pad_L32_L40")
    O2 = eng.ca_frames(packed(p["g"])["X"], [0, 40, 80]).cpu().view(2, 40, 9)
    assert float((O2.double().numpy() - p["O"]).__abs__().max()) <= 1e-6
    # the shorter member: the steps behind its end are zero, so its last row keeps o = U[30] alone and the rows behind it nothing
    assert bool((O2[:, [0, 38, 39]] == 0).all()) and bool((O2[0, 32:] == 0).all()) and bool((O2[0, 31, 3:] == 0).all())
    # segments of 1, 2 and 3 rows between longer ones: zero frames, finite output, the neighbours' frames untouched
    offs = [0, 32, 33, 35, 38, 78]
    Ca3 = np.concatenate([a["Ca"][0], b["Ca"][0][5:6], b["Ca"][0][5:7], b["Ca"][0][5:8], b["Ca"][0]])
    X3 = np.zeros((78, 4, 3), np.float32)
    X3[:, 1] = Ca3
    O3 = eng.ca_frames(X3, offs).cpu()
    assert bool(torch.isfinite(O3).all()) and bool((O3[32:38] == 0).all())
    assert torch.equal(O3[:32], O[:32]) and torch.equal(O3[38:], O[32:])
    assert float((O3.double() - car.frames_packed(t(Ca3).double(), offs)).abs().max()) <= 1e-6


# ---- 2. featurizer stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_featurizer_stage(case, precision):
    p = truth(case)
    g, E64, well = p["g"], p["E"], p["well"]
    Keff = g["E_idx"].shape[2]
    assert float(g["min_window_margin"]) >= 1e-3
    ill_share = float((~well).mean())
    assert ill_share <= ILL_CAP, f"{case}: {100 * ill_share:.1f} % of the edges are ill-conditioned"
    q = packed(g)
    ei, D = global_graph(g)
    eng = engine(precision, int(g["K"]))
    h_E, E = eng.edge_featurize(q["X"], q["ridx"], q["cenc"], torch.from_numpy(ei).cuda(), torch.from_numpy(D).cuda(), want_E=True,
                                offsets=q["offsets"])
    E, h_E = E.cpu().view(q["B"], q["L"], 48, 128), h_E.cpu().view(q["B"], q["L"], 48, 128)
    assert bool((E[:, :, Keff:] == 0).all()) and bool((h_E[:, :, Keff:] == 0).all())           # invalid slots: exactly 0
    d = np.abs(E[:, :, :Keff].double().numpy() - E64).max(-1)
    ref_ill = float(g["ref32_ill"])
    err_well, err_ill = float(d[well].max()), float(d[~well].max()) if (~well).any() else 0.0
    print(f"{case}/{precision}: E vs float64: {err_well:.2e} on well-conditioned edges (line {TOL_INTERMEDIATE:g}; reference fp32 "
          f"{float(g['ref32_well']):.2e}), {err_ill:.2e} on the other {100 * ill_share:.1f} % (line {F64_FACTOR} x {ref_ill:.2e})")
    assert err_well <= TOL_INTERMEDIATE
    assert err_ill <= F64_FACTOR * ref_ill
    assert bool(torch.isfinite(h_E).all())


# ---- 3. forward --------------------------------------------------------------------------------------------------------------
def forward_line(g, key):
    return max(TOL_INTERMEDIATE, F64_FACTOR * float(np.abs(g[key + "32"].astype(np.float64) - g[key + "64"]).max()))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_forward(case, precision):
    g = load_golden("ca_" + case)
    B, L, Keff = g["E_idx"].shape
    m = model_for(precision, int(g["K"]))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)
    args = (t(g["Ca"], torch.float32), t(g["S"], torch.int64), t(g["mask"], torch.float32), torch.ones(B, L, device="cuda:0"),
            t(g["residue_idx"], torch.int64), t(g["chain_enc"], torch.int64), None)
    with torch.no_grad():
        hidden, h_S, lp = m(*args)
        enc = m._encode_padded(m.engine(), *[args[k] for k in (0, 2, 4, 5)])
    ei = enc.E_idx.cpu().numpy().reshape(B, L, 48)
    assert (ei[:, :, Keff:] == -1).all()
    local = ei[:, :, :Keff] - (np.arange(B) * L)[:, None, None]
    # the reference's neighbours, row by row. Their ORDER may differ where two distances are one rounding apart (the residues 3.8 A
    # before and after a residue of a synthetic walk; torch on the CPU and the device round the square root independently): the
    # listed distances then agree slot by slot as test_gpu_parity asks of the k-NN (1 ulp of the square root), and the network sums
    # over a row's neighbours
    assert np.array_equal(np.sort(local, -1), np.sort(g["E_idx"].astype(np.int64), -1)), f"{case}: the device's neighbour sets differ from the reference's"
    for b in range(B):
        D = lambda idx: car.masked_neighbor_distance(torch.from_numpy(g["Ca"][b]), torch.from_numpy(g["mask"][b]), torch.from_numpy(idx.astype(np.int64))).numpy()
        np.testing.assert_allclose(D(local[b]), D(g["E_idx"][b]), atol=1e-6, rtol=3e-7)
    err = float(np.abs(lp.cpu().double().numpy() - g["log_probs64"]).max())
    line = forward_line(g, "log_probs")
    print(f"{case}/{precision}: log_probs vs float64 {err:.2e} (line {line:.2e})")
    assert err <= line
    masked = g["mask"] == 0
    if "hidden64" in g:
        got = torch.stack([hidden[2], hidden[1], hidden[0]]).cpu()                   # decoder layers 1..3
        herr = float(np.abs(got.double().numpy() - g["hidden64"]).max())
        hline = forward_line(g, "hidden")
        print(f"{case}/{precision}: decoder states vs float64 {herr:.2e} (line {hline:.2e})")
        assert herr <= hline
        assert bool((got[:, torch.from_numpy(masked)] == 0).all())                   # rows with mask 0: exactly 0
    assert h_S.shape == (B, L, 128)


# ---- 4. one encoder state, every decoder -------------------------------------------------------------------------------------
def _inputs(g, N):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)
    rep = lambda a, dt: t(a, dt).repeat(N, *([1] * (np.ndim(a) - 1)))
    return dict(X=rep(g["Ca"], torch.float32), S=rep(g["S"], torch.int64), mask=rep(g["mask"], torch.float32),
                ridx=rep(g["residue_idx"], torch.int64), cenc=rep(g["chain_enc"], torch.int64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["msk_L56_2ch", "syn_L32"])
def test_conditional_and_unconditional_probs(case, precision):
    g, o = load_golden("ca_" + case), load_golden("ca_probs_" + case)
    i = _inputs(g, 1)
    m = model_for(precision)
    t = lambda a: torch.from_numpy(a).cuda()
    with torch.no_grad():
        cond = m.conditional_probs(i["X"], i["S"], i["mask"], t(o["chain_M"]), i["ridx"], i["cenc"], t(o["randn"]))
        uncond = m.unconditional_probs(i["X"], i["mask"], i["ridx"], i["cenc"])
    ec = float(np.abs(cond.cpu().numpy() - o["conditional"]).max())
    eu = float(np.abs(uncond.cpu().numpy() - o["unconditional"]).max())
    print(f"{case}/{precision}: conditional_probs {ec:.2e}, unconditional_probs {eu:.2e} (line {TOL_INTERMEDIATE:g})")
    assert ec <= TOL_INTERMEDIATE and eu <= TOL_INTERMEDIATE
    assert np.array_equal((cond.cpu().numpy() != 0).any(-1), (o["conditional"] != 0).any(-1))


def _sample_args(g, o):
    N = o["randn"].shape[0]
    i = _inputs(g, N)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)
    args = (i["X"], t(o["randn"], torch.float32), t(o["S_true"], torch.int64), t(o["chain_mask"], torch.float32), i["cenc"], i["ridx"])
    kw = dict(mask=i["mask"], temperature=float(o["temperature"]), omit_AAs_np=o["omit_AAs"], bias_AAs_np=o["bias_AAs"],
              chain_M_pos=t(o["chain_M_pos"], torch.float32), bias_by_res=t(o["bias_by_res"], torch.float32), uniforms=t(o["u"], torch.float32))
    return args, kw


def _same_as_reference(out, o, tag):
    line = TOL_INTERMEDIATE / float(o["temperature"])
    err = float(np.abs(out["probs"].cpu().numpy().astype(np.float64) - o["probs"]).max())
    print(f"{tag}: probs {err:.2e} (line {line:g}), golden margin {float(o['min_margin']):.2e}")
    assert float(o["min_margin"]) >= 1e-3
    assert np.array_equal(out["decoding_order"].cpu().numpy(), o["decoding_order"])
    assert np.array_equal(out["S"].cpu().numpy(), o["S"]), tag                     # letter for letter
    assert err <= line


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])                        # (the samplers serve these two: tmpnn_sample)
@pytest.mark.parametrize("case", ["msk_L56_2ch", "syn_L32"])
def test_sample_and_tied_sample_reproduce_the_reference(case, precision):
    g = load_golden("ca_" + case)
    m = model_for(precision)
    o = load_golden("ca_sample_" + case)
    if "E_idx" in o:
        assert np.array_equal(o["E_idx"], g["E_idx"][0])
    args, kw = _sample_args(g, o)
    with torch.no_grad():
        _same_as_reference(m.sample(*args, **kw), o, f"sample {case}/{precision}")
    o = load_golden("ca_tied_" + case)
    args, kw = _sample_args(g, o)
    tied = [[int(k) for k in row if k >= 0] for row in o["tied_pos"]]
    with torch.no_grad():
        out = m.tied_sample(*args, tied_pos=tied, tied_beta=torch.from_numpy(o["tied_beta"]), **kw)
    _same_as_reference(out, o, f"tied_sample {case}/{precision}")


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample_each_is_sample_on_each_protein_alone(precision):
    eng = engine(precision)
    prots = [packed(load_golden("ca_" + c)) for c in ("msk_L56_2ch", "syn_L32")]
    rng = np.random.default_rng(3)
    N, alone, chains = 3, [], []
    for q in prots:
        L = q["L"]
        c = dict(order=np.stack([rng.permutation(L) for _ in range(N)]).astype(np.int64), S_fixed=rng.integers(0, 21, (N, L)),
                 free=np.ones((N, L), np.float32), u=rng.random((N, L)).astype(np.float32))
        c["free"][:, ::6] = 0
        enc = eng.encode(q["X"], q["mask"], q["ridx"], q["cenc"], q["offsets"])
        alone.append(eng.sample(enc, c["order"], c["S_fixed"], c["free"], c["u"], temperature=0.7))
        chains.append(c)
    cat = lambda k: torch.cat([q[k] for q in prots])
    enc = eng.encode(cat("X"), cat("mask"), cat("ridx"), cat("cenc"), torch.tensor([0, 56, 88], dtype=torch.int32))
    both = {k: np.concatenate([c[k] for c in chains], 1) for k in ("S_fixed", "free", "u")}
    both["order"] = np.concatenate([chains[0]["order"], chains[1]["order"] + 56], 1)
    res = eng.sample_each(enc, both["order"], both["S_fixed"], both["free"], both["u"], temperature=0.7)
    for (a, b), one in zip(((0, 56), (56, 88)), alone):
        assert torch.equal(res["S"][:, a:b], one["S"]) and torch.equal(res["probs"][:, a:b], one["probs"])


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_independence(precision):
    """A protein's E, hidden states and log_probs have the same bits alone, first or last of a packed batch of four, and in a batch
    of more tiles than compute units (8 x 40 rows: the persistent-tile path of the edge kernel)."""
    eng = engine(precision)
    me = packed(load_golden("ca_syn_L40"))
    others = [packed(load_golden("ca_" + c)) for c in ("syn_L32", "msk_L56_2ch", "msk_L40")]

    def run(members, at):
        cat = lambda k: torch.cat([q[k] for q in members])
        starts = np.concatenate([[0], np.cumsum([q["L"] for q in members])])
        offsets = torch.tensor(starts, dtype=torch.int32)
        X = cat("X")
        r = eng.ssm_forward(X, cat("S"), cat("mask"), cat("ridx"), cat("cenc"), offsets, want_ddg=False, want_hidden=True,
                            want_log_probs=True, want_E_idx=True)
        E_idx, D_nb = eng.knn_topk(X, cat("mask"), offsets)
        assert torch.equal(E_idx, r["E_idx"])
        E = eng.edge_featurize(X, cat("ridx"), cat("cenc"), E_idx, D_nb, want_E=True, offsets=offsets)[1]
        a, b = int(starts[at]), int(starts[at + 1])
        return E[a:b].clone(), r["hidden"][:, a:b].clone(), r["log_probs"][a:b].clone()

    alone = run([me], 0)
    assert tm_cus() < 8 * 40
    for members, at in (([me] + others, 0), (others + [me], 3), ([me] * 8, 5)):
        got = run(members, at)
        assert all(torch.equal(x, y) for x, y in zip(got, alone)), (len(members), at)


def tm_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 6. nothing else moved ---------------------------------------------------------------------------------------------------
def test_full_backbone_handle_is_untouched_by_a_ca_handle():
    """ssm_forward of a full-backbone engine before any CA handle exists in the process equals, bit for bit, the same call after CA
    handles were created and used: the CA path shares no mutable state. Runs in a fresh process so that 'before' is before."""
    import os
    import subprocess
    import sys
    code = r'''
import numpy as np, torch, sys
sys.path.insert(0, sys.argv[1])
from thermompnn_amd.engine import Engine
from thermompnn_amd.weights import synthetic_state_dict
g = np.load(sys.argv[2])
full = Engine(synthetic_state_dict(0), "cuda:0", 48, retry_precision=None)
args = (g["X"], g["S"], g["mask"], g["residue_idx"], g["chain_enc"], [0, 32])
kw = dict(want_ddg=True, want_hidden=True, want_log_probs=True)
before = {k: v.clone() for k, v in full.ssm_forward(*args, **kw).items()}
ca = Engine(synthetic_state_dict(0, "mpnn_ca"), "cuda:0", 48, retry_precision=None)
lp = ca.ssm_forward(*args, want_ddg=False, want_log_probs=True)["log_probs"]
assert bool(torch.isfinite(lp).all())
after = full.ssm_forward(*args, **kw)
assert all(torch.equal(before[k], after[k]) for k in before), "the full-backbone result moved"
assert not torch.equal(lp, after["log_probs"])
print("SAME")
'''
    from conftest import GOLDEN, REPO
    r = subprocess.run([sys.executable, "-c", code, REPO, os.path.join(GOLDEN, "syn_L32.npz")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SAME" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_ddg_and_the_plain_featurizer_entry_are_refused():
    """A CA handle with a ddg output is TMPNN_E_INVALID from the C entry itself, before any launch (the status word keeps its
    value); the Python layer refuses earlier; tmpnn_edge_featurize points a CA handle to tmpnn_edge_featurize_ca."""
    import ctypes as C
    eng, q = engine("f16x2"), packed(load_golden("ca_syn_L32"))
    with pytest.raises(ValueError, match="ca_only"):
        eng.ssm_forward(q["X"], q["S"], q["mask"], q["ridx"], q["cenc"], q["offsets"])
    p = lambda t: C.c_void_p(t.data_ptr())
    offsets = q["offsets"].cuda()
    ws = torch.empty(eng.lib.tmpnn_workspace_bytes(32), dtype=torch.uint8, device="cuda:0")
    ddg, lp = torch.full((32, 21), 7.0, device="cuda:0"), torch.full((32, 21), 7.0, device="cuda:0")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    call = lambda d: eng.lib.tmpnn_ssm_forward(eng.w.handle, p(q["X"]), p(q["S"]), p(q["mask"]), p(q["ridx"]), p(q["cenc"]), p(offsets), 1, 32, 32, 48,
                                               d, None, p(lp), None, p(status), p(ws), ws.numel(), None)
    assert eng.lib.tmpnn_weights_is_ca(eng.w.handle) == 1
    rc = call(p(ddg))
    assert rc == -1 and b"CA handle" in eng.lib.tmpnn_last_error()
    torch.cuda.synchronize()
    assert int(status.item()) == 77 and bool((ddg == 7).all()) and bool((lp == 7).all())        # nothing was launched
    assert call(None) == 0                                                                    # the same call without ddg runs
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool(torch.isfinite(lp).all()) and not bool((lp == 7).any())
    E_idx, D_nb = eng.knn_topk(q["X"], q["mask"], q["offsets"])
    h_E = torch.empty((32, 48, 128), device="cuda:0")
    rc = eng.lib.tmpnn_edge_featurize(eng.w.handle, q["X"].data_ptr(), q["ridx"].data_ptr(), q["cenc"].data_ptr(), E_idx.data_ptr(),
                                      D_nb.data_ptr(), 32, h_E.data_ptr(), None, None)
    assert rc == -1 and b"tmpnn_edge_featurize_ca" in eng.lib.tmpnn_last_error()
    with pytest.raises(ValueError, match="no ddG head"):
        from thermompnn_amd.engine import Engine
        Engine(ca_weights(), "cuda:0", 48, with_head=True)


# ---- the model on batches of different members, and the command line ----------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample_on_a_batch_of_different_members_is_each_member_alone(precision):
    """ProteinMPNN(ca_only=True).sample and ProteinMPNNDesign.tied_sample on the padded pair (two different structures: one padded
    encode, one launch) give each member the letters and probs of a call with that member alone, bit for bit. tied_sample takes
    member 0's decoding order — argsort of (chain_M_pos * mask + 1e-4) |randn| — for every member, so the rows behind the shorter
    member's end are fixed positions in both members: the order is then the same whichever member comes first."""
    g = load_golden("ca_pad_L32_L40")
    m = model_for(precision)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)
    gen = torch.Generator().manual_seed(5)
    randn, u = torch.randn(2, 40, generator=gen).cuda(), torch.rand(2, 40, generator=gen).cuda()
    X, S, mask = t(g["Ca"], torch.float32), t(g["S"], torch.int64), t(g["mask"], torch.float32)
    cenc, ridx, ones = t(g["chain_enc"], torch.int64), t(g["residue_idx"], torch.int64), torch.ones(2, 40, device="cuda:0")
    tied = [[i, 16 + i] for i in range(8)]
    pos = torch.ones(2, 40, device="cuda:0")
    pos[:, 32:] = 0

    def run(sl):
        kw = dict(mask=mask[sl], temperature=0.7, uniforms=u[sl], chain_M_pos=pos[sl])
        with torch.no_grad():
            a = m.sample(X[sl], randn[sl], S[sl], ones[sl], cenc[sl], ridx[sl], **kw)
            b = m.tied_sample(X[sl], randn[:1].expand(2, 40)[sl], S[sl], ones[sl], cenc[sl], ridx[sl], tied_pos=tied, **kw)
        return a, b

    both = run(slice(0, 2))
    for k in range(2):
        alone = run(slice(k, k + 1))
        for got, want in zip(both, alone):
            assert torch.equal(got["S"][k], want["S"][0]) and torch.equal(got["probs"][k], want["probs"][0]), k
    assert bool((both[0]["probs"][0, 32:] == 0).all()) and not torch.equal(both[0]["S"][0, :32], both[0]["S"][1, :32])
    assert torch.equal(both[0]["S"][1, 32:], S[1, 32:])                                    # fixed positions keep their letter


def test_design_scan_ca_only(tmp_path):
    """python -m thermompnn_amd.design_scan --ca_only: reads the C-alpha atoms alone (a residue without its N line is designed, a
    numbering gap is not), and its first sample is Engine.sample_each's on the same orders and uniforms."""
    import os
    from conftest import GOLDEN
    from thermompnn_amd import design_scan
    from thermompnn_amd.native_pdb import parse_pdbs
    pdb = os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb")
    out = tmp_path / "ca.fa"
    assert design_scan.main([pdb, "--ca_only", "--synthetic_weights", "0", "--num_seq", "2", "--seed", "3", "--out", str(out)]) == 0
    lines = out.read_text().splitlines()
    e = parse_pdbs([pdb])[0]
    assert len(lines) == 6 and f"unmasked={int(e['ca_mask'].sum())}" in lines[0] and int(e["ca_mask"].sum()) == int(e["mask"].sum()) + 1
    assert [i for i, c in enumerate(lines[3]) if c == "X"] == [i for i in range(len(e["S"])) if e["ca_mask"][i] == 0]
    e["mask"] = e["ca_mask"]
    chains = design_scan.draw_chains(e, 2, [], torch.Generator().manual_seed(3))
    want = design_scan.design_batch(engine("f16x2"), [e], [chains], 0.1)[0]
    assert lines[3] == design_scan.letters(want["S"][0], e["mask"]) and lines[5] == design_scan.letters(want["S"][1], e["mask"])
    assert f"score={float(want['score'][0]):.6f}" in lines[2]
