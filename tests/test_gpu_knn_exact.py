"""The k-NN graph against an exact statement of its rule, at distance ties, in every form and through every entry that builds it.

On the integer lattices of tests/lattice_backbones.py (checked on the host by test_knn_exact_host.py) the promised list — ascending
adjusted distance, the lower index first among equals, masked candidates at the row's D_max, a masked row listing 0 .. Keff-1 — is a
stable sort on integers (exact_knn). Everywhere here E_idx[:, :Keff] EQUALS that list on every row, masked rows included: no set
comparison, no row left out. Shipped library only; every row form is reached through ``max_len`` (Engine._max_len honours a value
larger than the longest protein when ``offsets`` is host data):
    max_len <= 256: knn_row_sel<4> / knn_row_reg<4>      max_len <= 512: knn_row_sel<8> / knn_row_reg<8>
    above: LDS rows, knn_row<false> for L <= 512, knn_row<true> for L > 512 (a second rescan pass for L > 4096)
and the k-NN inside the featurizer launch (a small f16x2 forward), encode() and the training step build the same lists."""
import numpy as np
import pytest
import torch

from lattice_backbones import NAMES, STEP, backbone, exact_graph, expected_D, lattice, oracle_table, row_keys

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for log-probabilities
TOL_DDG = 1e-4            # kcal/mol
F64_FACTOR = 2.5          # conftest.HOT_F64_FACTOR: the rule test_gpu_parity.close applies where an absolute line does not fit
D_NB_ULP = 0              # D_nb against lattice_backbones.expected_D: sqrtf is correctly rounded here, like numpy's root (measured: 0 ulp in every slot)
MAX_LENS = (300, 600, 4200)
KS = (48, 30)
SMALL = ["lat_L64", "lat_L100", "lat_shell", "lat_L90hm"]                     # alone: T <= CUs and max_len <= 256
RAGGED = (["lat_L49m", "lat_L300m", "lat_L65", "lat_shell"], ["lat_L100", "lat_L600m", "lat_L64"],
          ["lat_L90hm", "lat_L520hm", "lat_L64"])
CONSUMED = ["lat_L100", "lat_shell", "lat_L49m"]
_ENGINES = {}
_ALONE = {}


def engine(precision="f16x2", K=48):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if (precision, K) not in _ENGINES:
        _ENGINES[precision, K] = Engine(synthetic_state_dict(0), "cuda:0", K, precision=precision, retry_precision=None)
    return _ENGINES[precision, K]


def pack(names):
    prots = [backbone(n) for n in names]
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in prots])).to("cuda:0", dt)
    starts = np.concatenate([[0], np.cumsum([len(p["S"]) for p in prots])])
    return dict(X=cat("X", torch.float32), S=cat("S", torch.int32), mask=cat("mask", torch.float32), ridx=cat("ridx", torch.int32),
                cenc=cat("cenc", torch.int32), offsets=torch.tensor(starts, dtype=torch.int32), starts=starts)


def assert_exact_graph(name, ei, K, what, start=0):
    """ei [L,48]: the device's rows of layout ``name`` (global indices of a batch in which it starts at ``start``)."""
    E, _ = exact_graph(name, K)
    Keff = E.shape[1]
    assert ei.shape == (len(E), 48)
    assert (ei[:, Keff:] == -1).all(), f"{what}: slots beyond {Keff}"
    got = ei[:, :Keff].astype(np.int64) - start
    bad = np.nonzero((got != E).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        slot = int(np.nonzero(got[i] != E[i])[0][0])
        live = bool(lattice(name)[1][i] > 0)
        raise AssertionError(f"{what}: {name} K={K}: {len(bad)} rows differ from exact_knn; first row {i} ({'live' if live else 'masked'}) "
                             f"slot {slot}: device {got[i, slot:slot + 6].tolist()} exact {E[i, slot:slot + 6].tolist()}")


def knn_alone(name, K):
    """knn_topk of the layout alone at max_len = L -> (E_idx, D_nb) numpy, cached (checked by test_every_row_form)."""
    if (name, K) not in _ALONE:
        p = pack([name])
        E_idx, D_nb = engine("f16x2", K).knn_topk(p["X"], p["mask"], p["offsets"], max_len=len(backbone(name)["S"]))
        _ALONE[name, K] = (E_idx.cpu().numpy(), D_nb.cpu().numpy())
    return _ALONE[name, K]


# ---- a. every row form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", NAMES)
def test_every_row_form(name, K):
    eng = engine("f16x2", K)
    P, mask = lattice(name)
    L = len(P)
    E, key = exact_graph(name, K)
    Keff = E.shape[1]
    p = pack([name])
    lens = [L] + [m for m in MAX_LENS if m > L]
    first = None
    for max_len in lens:
        if max_len == L:
            ei, dn = knn_alone(name, K)
        else:
            E_idx, D_nb = eng.knn_topk(p["X"], p["mask"], p["offsets"], max_len=max_len)
            ei, dn = E_idx.cpu().numpy(), D_nb.cpu().numpy()
        assert_exact_graph(name, ei, K, f"knn_topk(max_len={max_len})")
        if first is None:
            first = dn
        assert np.array_equal(dn.view(np.uint32), first.view(np.uint32)), f"D_nb at max_len={max_len} differs from max_len={L}"
    dn = first
    assert (dn[:, Keff:] == 0).all()
    bits = dn[:, :Keff].view(np.uint32).astype(np.int64)
    assert (np.diff(bits, axis=1) >= 0).all()                                 # ascending (non-negative floats order like their bits)
    assert np.array_equal(np.diff(bits, axis=1) == 0, np.diff(key, axis=1) == 0)       # bit-equal exactly where the integer keys tie
    want = expected_D(P, STEP, mask, E).view(np.uint32).astype(np.int64)
    ulp = np.abs(bits - want)
    print(f"{name} K={K} max_len in {lens}: D_nb vs expected_D: max {int(ulp.max())} ulp, {int((ulp > 0).sum())} of {ulp.size} slots differ")
    assert int(ulp.max()) <= D_NB_ULP


# ---- b. ragged batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("names", RAGGED, ids=["max300", "max600", "max520_masked"])
def test_ragged_batches_have_the_single_protein_rows(names, K):
    p = pack(names)
    E_idx, D_nb = engine("f16x2", K).knn_topk(p["X"], p["mask"], p["offsets"])
    ei, dn = E_idx.cpu().numpy(), D_nb.cpu().numpy()
    for k, name in enumerate(names):
        s, e = int(p["starts"][k]), int(p["starts"][k + 1])
        assert_exact_graph(name, ei[s:e], K, f"batch {names}", start=s)
        a_ei, a_dn = knn_alone(name, K)
        assert np.array_equal(np.where(ei[s:e] < 0, -1, ei[s:e] - s), a_ei), name
        assert np.array_equal(dn[s:e].view(np.uint32), a_dn.view(np.uint32)), name


# ---- c. every entry that builds the graph ----------------------------------------------------------------------------------------
def forward(eng, names, **kw):
    b = pack(names)
    r = eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], want_E_idx=True, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}, b["starts"]


@pytest.mark.parametrize("precision,K", [("f16x2", 48), ("f16x2", 30), ("fp32", 48)])
@pytest.mark.parametrize("name", SMALL)
def test_fused_forward_graph(name, precision, K):
    """f16x2, T <= CUs, max_len <= 256: the rows are computed inside the featurizer launch (featurize_fusable, knn_residue<4>);
    fp32: the separate launch."""
    L = len(backbone(name)["S"])
    assert L <= torch.cuda.get_device_properties(0).multi_processor_count and L <= 256
    r, _ = forward(engine(precision, K), [name])
    assert_exact_graph(name, r["E_idx"], K, f"ssm_forward[{precision}]")
    assert np.isfinite(r["ddg"]).all()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SMALL)
def test_encode_graph(name, K):
    p = pack([name])
    enc = engine("f16x2", K).encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])
    assert_exact_graph(name, enc.E_idx.cpu().numpy(), K, "encode")


@pytest.mark.parametrize("name", ["lat_L49m", "lat_L100", "lat_L600m", "lat_L90hm"])
def test_training_step_graph(name, tmp_path):
    """launch_knn with max_len = L inside tmpnn_finetune_step; only the graph is checked, and that the loss is finite."""
    from test_gpu_finetune import _model
    from thermompnn_amd.finetune import MPNNTrainer, Protein
    tr = MPNNTrainer(_model(tmp_path), seed=1)
    g = backbone(name)
    L = len(g["S"])
    live = np.nonzero(g["mask"] > 0)[0]
    pos = live[[0, len(live) // 3, len(live) // 2, len(live) // 2, len(live) - 1]]
    wt = g["S"][pos]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    prot = Protein(dev(g["X"], torch.float32), dev(g["S"], torch.int32), dev(g["mask"], torch.float32), dev(g["ridx"], torch.int32),
                   dev(g["cenc"], torch.int32), dev(pos, torch.int32), dev((wt + 3) % 20, torch.int32), dev(wt, torch.int32),
                   dev(np.linspace(-1.0, 1.0, len(pos)), torch.float32), name)
    Keff = min(48, L)
    E_idx = torch.full((L, Keff), -7, dtype=torch.int32, device="cuda")
    loss = tr.forward_backward(prot, p_mpnn=0.0, p_head=0.0, step=1, E_idx_out=E_idx)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.item()))
    ei = np.full((L, 48), -1, np.int32)
    ei[:, :Keff] = E_idx.cpu().numpy()
    assert_exact_graph(name, ei, 48, "tmpnn_finetune_step")


# ---- d. the order is consumed as produced ----------------------------------------------------------------------------------------
def close(got, want, tol, what, f64):
    """|got - want| <= tol; where that line is exceeded, the rule of test_gpu_parity.close for its hot and wide draws: against the
    oracle evaluated in float64 (``f64()``), |got - f64| <= max(2.5 x max|want - f64|, tol)."""
    got64, want64 = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.abs(got64 - want64).max())
    print(f"{what}: max |hip - oracle| = {err:.3e} (line {tol:g})")
    if err <= tol:
        return
    truth = np.asarray(f64(), np.float64)
    ref_err, hip_err = float(np.abs(want64 - truth).max()), float(np.abs(got64 - truth).max())
    print(f"{what}: |hip - f64| = {hip_err:.3e}, |oracle fp32 - f64| = {ref_err:.3e}, ratio {hip_err / ref_err:.2f}")
    assert hip_err <= max(F64_FACTOR * ref_err, tol), f"{what}: |hip - f64| = {hip_err:.3e}, the reference is {ref_err:.3e} from the truth"


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_the_order_is_consumed_as_produced(precision):
    """The fused forward against the oracle on the EXACT graph (not on the device's own): a slot order that the featurizer, the message
    passes or the decoder consumed differently from how the k-NN produced it would move these numbers. And each protein alone, inside
    its ragged batch of (b), and next to lat_L600m (whose max_len selects the LDS rows) gives bit-identical ddG."""
    eng = engine(precision, 48)
    alone = {}
    for name in CONSUMED:
        r, _ = forward(eng, [name], want_log_probs=True)
        alone[name] = r
        assert_exact_graph(name, r["E_idx"], 48, f"ssm_forward[{precision}]")
        E, _ = exact_graph(name, 48)
        valid = backbone(name)["mask"] > 0
        want = oracle_table(name, E)
        f64 = lambda k: (lambda: oracle_table(name, E, f64=True)[k][valid])
        close(r["log_probs"][valid], want["log_probs"][valid], TOL_INTERMEDIATE, f"{precision}/{name}/log_probs", f64("log_probs"))
        close(r["ddg"][valid], want["ddg"][valid], TOL_DDG, f"{precision}/{name}/ddg", f64("ddg"))
    batches = [list(b) for b in RAGGED[:2]] + [[name, "lat_L600m"] for name in CONSUMED]
    seen = {name: 0 for name in CONSUMED}
    for names in batches:
        r, starts = forward(eng, names)
        for k, name in enumerate(names):
            if name in alone:
                s, e = int(starts[k]), int(starts[k + 1])
                assert_exact_graph(name, r["E_idx"][s:e], 48, f"ssm_forward[{precision}] of {names}", start=s)
                assert np.array_equal(r["ddg"][s:e].view(np.uint32), alone[name]["ddg"].view(np.uint32)), (name, names)
                seen[name] += 1
    assert all(n == 2 for n in seen.values()), seen


# ---- e. centrality on the same lattices ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lat_L100", "lat_L300m"])
def test_centrality_counts_strictly_inside_the_radius(name):
    """#{ j live, j != i : STEP^2 s2 < 100 } for live i, -1 for masked i; pairs at s2 = 25 lie at exactly 10.0 A and are not counted
    (test_knn_exact_host.test_pairs_at_exactly_the_centrality_radius_exist)."""
    P, mask = lattice(name)
    live = mask > 0
    s2 = row_keys(P, np.ones(len(P), np.float32))
    assert ((s2 == 25) & live[:, None] & live[None, :]).any() and STEP * STEP * 25 == 100.0
    inside = (int(STEP * STEP) * s2 < 100) & live[None, :]
    want = np.where(live, inside.sum(axis=1) - 1, -1)                         # (minus the residue itself)
    p = pack([name])
    got = engine().centrality(p["X"], p["mask"], p["offsets"], radius=10.0).cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
