"""The C-alpha edge kernels (tmpnn_graph_ca.hip) where the fixtures of test_gpu_ca.py do not reach: packs long enough for a workgroup to
walk three tiles and more (the software pipeline's steady state) and for the XCD split of the tile range; segments of 1 .. 7 rows in
the edge kernels and the forward; step lengths on and next to the 3.6 / 4.0 window. Inputs and their conditions: tests/ca_inputs.py
(asserted without a GPU by tests/test_ca_forms_host.py).

Every edge is judged by the rule of test_gpu_ca.py against the float64 restatement (tests/ca_restatement.py) of each member alone on
the device's own neighbour lists: well-conditioned edges meet TOL_INTERMEDIATE = 1e-5; the others stay within 2.5 x the largest
distance of the restatement's own float32 run from its float64 run on the ill-conditioned edges of the same pack (computed here from the
restatement, never from the device); invalid slots are exactly 0. An edge is well-conditioned when ca_restatement.well_conditioned
holds and both of its rows pass ca_inputs.frame_conditioned."""
import numpy as np
import pytest
import torch

import ca_inputs as ci
import ca_restatement as car
from test_gpu_ca import F64_FACTOR, PRECISIONS, TOL_INTERMEDIATE, ca_weights, engine, tm_cus

pytestmark = pytest.mark.gpu

_PACKS, _TRUTH = {}, {}


def get_pack(name):
    if name not in _PACKS:
        _PACKS[name] = ci.short_pack() if name == "short" else ci.long_pack(int(name))
    return _PACKS[name]


def to_device(pack, dev="cuda:0"):
    """A pack as the engine takes it: X [T,4,3] with the C-alpha atoms in slot 1, one segment per member."""
    cat = lambda k, dt: torch.from_numpy(np.concatenate([m[k] for m in pack])).to(dev, dt)
    starts = ci.offsets_of(pack)
    X = torch.zeros((int(starts[-1]), 4, 3), dtype=torch.float32)
    X[:, 1] = torch.from_numpy(np.concatenate([m["Ca"] for m in pack]))
    return dict(X=X.to(dev), S=cat("S", torch.int32), mask=cat("mask", torch.float32), ridx=cat("ridx", torch.int32), cenc=cat("cenc", torch.int32),
                offsets=torch.from_numpy(starts).to(torch.int32), starts=starts)


def run_pack(eng, q):
    """knn_topk, edge_featurize and the fused forward of one packed batch -> E_idx, E, h_E [T,48,...], hidden [3,T,128], log_probs [T,21]."""
    r = eng.ssm_forward(q["X"], q["S"], q["mask"], q["ridx"], q["cenc"], q["offsets"], want_ddg=False, want_hidden=True, want_log_probs=True,
                        want_E_idx=True)
    E_idx, D_nb = eng.knn_topk(q["X"], q["mask"], q["offsets"])
    assert torch.equal(E_idx, r["E_idx"])
    h_E, E = eng.edge_featurize(q["X"], q["ridx"], q["cenc"], E_idx, D_nb, want_E=True, offsets=q["offsets"])
    return dict(E_idx=E_idx, E=E, h_E=h_E, hidden=r["hidden"], log_probs=r["log_probs"])


def local_graphs(pack, starts, E_idx):
    """The device's E_idx [T,48] (global rows) -> one [n, Keff] int64 list per member, local rows; -1 beyond Keff = min(48, n), every
    entry inside the member, and each row's set the stable top-k of the masked distance."""
    out = []
    for m, a, b in zip(pack, starts[:-1], starts[1:]):
        n, rows = int(b - a), E_idx[a:b]
        Keff = min(48, n)
        assert (rows[:, Keff:] == -1).all()
        local = rows[:, :Keff].astype(np.int64) - int(a)
        assert (local >= 0).all() and (local < n).all()
        assert np.array_equal(np.sort(local, -1), np.sort(ci.host_graph(m).numpy(), -1)), "the device's neighbour sets differ from the stable top-k"
        out.append(torch.from_numpy(np.ascontiguousarray(local)))
    return out


def truth(name, E_idx):
    """The pack's float64 restatement on the device's graph, its well-conditioned edges and the float32 restatement's own distances.
    Computed once per pack and left unchanged; the graph does not depend on the precision, and every later caller's must be the same."""
    pack = get_pack(name)
    if name not in _TRUTH:
        graphs = local_graphs(pack, ci.offsets_of(pack), E_idx)
        _TRUTH[name] = dict(ci.pack_truth(ca_weights(), pack, graphs), E_idx=E_idx.copy())
    assert np.array_equal(_TRUTH[name]["E_idx"], E_idx)
    return _TRUTH[name]


def judge(tag, starts, tr, r):
    """Every valid edge of every member against the restatement, the invalid slots exactly 0, everything finite."""
    valid = r["E_idx"] >= 0
    zeros = bool((r["E"][~valid] == 0).all()) and bool((r["h_E"][~valid] == 0).all())
    finite = bool(torch.isfinite(r["E"]).all()) and bool(torch.isfinite(r["h_E"]).all())
    E = r["E"].cpu().numpy()
    err_well = err_ill = 0.0
    for a, b, x in zip(starts[:-1], starts[1:], tr["members"]):
        Keff = x["E64"].shape[1]
        d = np.abs(E[a:b, :Keff].astype(np.float64) - x["E64"]).max(-1)
        err_well = max(err_well, float(d[x["well"]].max()) if x["well"].any() else 0.0)
        err_ill = max(err_ill, float(d[~x["well"]].max()) if (~x["well"]).any() else 0.0)
    print(f"{tag}: T = {int(starts[-1])} on {tm_cus()} compute units; E vs float64: {err_well:.2e} on well-conditioned edges (line {TOL_INTERMEDIATE:g}; "
          f"restatement float32 {tr['ref_well']:.2e}), {err_ill:.2e} on the other {100 * tr['ill_share']:.1f} % (line {F64_FACTOR} x {tr['ref_ill']:.2e}); "
          f"invalid slots exactly 0: {zeros}, finite: {finite}")
    assert tr["ill_share"] <= ci.ILL_CAP
    assert zeros and finite
    assert err_well <= TOL_INTERMEDIATE
    assert err_ill <= F64_FACTOR * tr["ref_ill"]


KEYS = ("E", "h_E", "hidden", "log_probs")


def rows_of(r, a, b):
    return {k: (r[k][:, a:b] if k == "hidden" else r[k][a:b]) for k in KEYS}


# ---- A. long packs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [70, 260])
def test_long_pack(n, precision):
    """n = 70: every workgroup walks three tiles and more (the in-loop prefetch of tile i + 2 step, both s_ix buffers); n = 260: the
    XCD branch of xcd_tile_range. Edge by edge against float64; the first, second, middle and the two last members equal themselves
    run alone, bit for bit; a rerun and the pack in reversed member order give every member the same bits."""
    pack = get_pack(str(n))
    q = to_device(pack)
    starts, T, cus = q["starts"], int(q["starts"][-1]), tm_cus()
    if n == 70:
        assert 3 * cus + 1 <= T < 8 * cus, (T, cus)
    elif cus % 8 == 0:
        assert T >= 8 * cus, (T, cus)
    else:
        assert T >= 3 * cus + 1, (T, cus)
    eng = engine(precision)
    r = run_pack(eng, q)
    tr = truth(str(n), r["E_idx"].cpu().numpy())
    judge(f"long_pack({n})/{precision}", starts, tr, r)
    for b in (0, 1, n // 2, n - 2, n - 1):
        alone = run_pack(eng, to_device([pack[b]]))
        got = rows_of(r, int(starts[b]), int(starts[b + 1]))
        assert all(torch.equal(got[k], alone[k]) for k in KEYS), (b, [k for k in KEYS if not torch.equal(got[k], alone[k])])
    again = run_pack(eng, q)
    assert all(torch.equal(r[k], again[k]) for k in KEYS + ("E_idx",))
    qr = to_device(pack[::-1])
    rr = run_pack(eng, qr)
    sr = qr["starts"]
    perm = torch.cat([torch.arange(int(sr[n - 1 - b]), int(sr[n - b])) for b in range(n)]).cuda()      # row of the reversed pack, per row of this one
    assert all(torch.equal(rr[k][:, perm] if k == "hidden" else rr[k][perm], r[k]) for k in KEYS)


# ---- B. short segments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_short_segments(precision):
    """Segments of 1, 2, 3, 4, 5 and 7 rows between a 12-row member and a 16-row member with a missing C-alpha, through the edge kernels
    and the forward: most of every row's 48 slots are invalid, ca_row's zero coordinates outside [s, e) and the zero frames of n <= 3
    decide every feature."""
    pack = get_pack("short")
    q = to_device(pack)
    starts = q["starts"]
    eng = engine(precision)
    r = run_pack(eng, q)
    tr = truth("short", r["E_idx"].cpu().numpy())
    judge(f"short_pack/{precision}", starts, tr, r)
    O = eng.ca_frames(q["X"], q["offsets"]).cpu()
    want = car.frames_packed(torch.from_numpy(np.concatenate([m["Ca"] for m in pack])).double(), starts)
    assert torch.equal(O == 0, want == 0) and float((O.double() - want).abs().max()) <= 1e-6
    for (a, b), m in zip(zip(starts[:-1], starts[1:]), pack):
        if len(m["S"]) <= 3:
            assert bool((O[a:b] == 0).all())
    assert bool(torch.isfinite(r["hidden"]).all()) and bool(torch.isfinite(r["log_probs"]).all())
    dead = q["mask"] == 0
    assert int(dead.sum()) == 1 and bool((r["hidden"][:, dead] == 0).all())                     # rows with mask 0: exactly 0
    for b in range(len(pack)):
        alone = run_pack(eng, to_device([pack[b]]))
        got = rows_of(r, int(starts[b]), int(starts[b + 1]))
        assert all(torch.equal(got[k], alone[k]) for k in KEYS), (b, [k for k in KEYS if not torch.equal(got[k], alone[k])])


# ---- C. the window's edges -------------------------------------------------------------------------------------------------------------
def test_window_edges_through_ca_frames():
    """Steps of exactly 3.6f, 4.0f, their float32 neighbours and 3.8f: the device keeps the steps the restatement keeps (3.6 < n < 4.0,
    strict at both ends) — the zero pattern of O equals the float64 restatement's per row, per frame row and per element, and the
    values agree within 1e-6."""
    pack, _ = ci.window_pack()
    q = to_device(pack)
    O = engine("f16x2").ca_frames(q["X"], q["offsets"]).cpu()
    want = car.frames_packed(torch.from_numpy(np.concatenate([m["Ca"] for m in pack])).double(), q["starts"])
    T = O.shape[0]
    got_rows, want_rows = (O.view(T, 3, 3) != 0).any(-1), (want.view(T, 3, 3) != 0).any(-1)
    print("window pack: non-zero frame rows (o, n, o x n) per residue, device | restatement:")
    for a, b, names in zip(q["starts"][:-1], q["starts"][1:], ci.WINDOW_SEGMENTS):
        print("  ", " ".join(names), "|", got_rows[a:b].int().tolist(), "|", want_rows[a:b].int().tolist())
    err = float((O.double() - want).abs().max())
    print(f"window pack: O vs float64 {err:.2e} (line 1e-6)")
    assert torch.equal(got_rows.any(-1), want_rows.any(-1))
    assert torch.equal(got_rows, want_rows)
    assert torch.equal(O == 0, want == 0)
    assert err <= 1e-6
