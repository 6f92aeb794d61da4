"""The crafted inputs of tests/test_gpu_ca_forms.py without a GPU: every condition those tests rely on, asserted on the inputs and on the
float64 / float32 restatement alone (tests/ca_inputs.py, tests/ca_restatement.py) — window margins, frame conditioning, the
ill-conditioned share of at most 10 % per pack, the exact step vectors at the window's edges, and what the specification yields for
segments of fewer than 3 rows. The graphs here are the stable top-k of the masked float32 distance; on these packs Keff = L, so a row's
neighbour set is its whole segment whatever the device's order, and the shares and distances printed here are those of the GPU test."""
import numpy as np
import pytest
import torch

import ca_inputs as ci
import ca_restatement as car
from test_ca_host import ca_weights

# the compute units of an MI355X: the sizes of the long packs are asserted against the device's own count in the GPU test
CUS = 256


def conditions(pack):
    graphs = [ci.host_graph(m) for m in pack]
    tr = ci.pack_truth(ca_weights(), pack, graphs)
    margin = min(ci.window_margin(m["Ca"]) for m in pack)
    framed_ok = all(bool(ci.frame_conditioned(torch.from_numpy(m["Ca"]).double()).all()) for m in pack)
    return tr, margin, framed_ok


@pytest.mark.parametrize("n", [70, 260])
def test_long_packs_meet_their_conditions(n):
    pack = ci.long_pack(n)
    T = int(ci.offsets_of(pack)[-1])
    assert (3 * CUS + 1 <= T < 8 * CUS) if n == 70 else T >= 8 * CUS
    assert all(8 <= len(m["S"]) <= 16 for m in pack) and {len(m["S"]) for m in pack} == set(range(8, 17))
    dead = [m for m in pack if (m["mask"] == 0).any()]
    assert len(dead) == (n + 2) // 3 and all((m["Ca"][m["mask"] == 0] == 0).all() and (m["Ca"][m["mask"] == 1] != 0).any(-1).sum() >= len(m["S"]) - 2
                                              for m in dead)
    tr, margin, framed_ok = conditions(pack)
    print(f"long_pack({n}): T = {T}, {tr['edges']} edges, ill share {100 * tr['ill_share']:.1f} %, window margin {margin:.2e}, restatement float32 "
          f"vs float64 {tr['ref_well']:.2e} on well-conditioned edges and {tr['ref_ill']:.2e} on the rest")
    assert tr["ill_share"] <= ci.ILL_CAP and margin >= ci.WINDOW_MARGIN and framed_ok
    assert tr["ref_well"] <= 1e-5                                # the 1e-5 line is one a float32 evaluation can meet on these edges
    assert tr["ref_ill"] > tr["ref_well"]                        # (and the other edges are where float32 itself moves)


def test_short_pack_meets_its_conditions_and_the_zero_frame_specification():
    pack = ci.short_pack()
    assert [len(m["S"]) for m in pack] == [12, 1, 2, 3, 4, 5, 7, 16]
    assert int(pack[-1]["mask"].sum()) == 15 and (pack[-1]["Ca"][pack[-1]["mask"] == 0] == 0).all()
    tr, margin, framed_ok = conditions(pack)
    print(f"short_pack: {tr['edges']} edges, ill share {100 * tr['ill_share']:.1f} %, window margin {margin:.2e}, restatement float32 vs float64 "
          f"{tr['ref_well']:.2e} / {tr['ref_ill']:.2e}")
    assert tr["ill_share"] <= ci.ILL_CAP and margin >= ci.WINDOW_MARGIN and framed_ok
    assert tr["ref_well"] <= 1e-5
    W = ca_weights()
    t = torch.from_numpy
    for m in pack:
        n = len(m["S"])
        Ca = t(m["Ca"]).double()
        O = car.frames(Ca)
        framed = (O != 0).any(-1)
        # a frame has a non-zero row when one of its two steps is kept: its own C-alpha and one of the neighbours' present
        live = [i for i in range(1, n - 2) if m["mask"][i] and (m["mask"][i - 1] or m["mask"][i + 1])]
        assert framed.nonzero().flatten().tolist() == live, n
        if n == 4:
            assert live == [1]
        x = car.edge_inputs(Ca, t(m["mask"]).double(), t(m["ridx"]), t(m["cenc"]), ci.host_graph(m),
                            W["features.embeddings.linear.weight"].double(), W["features.embeddings.linear.bias"].double())
        assert x.shape == (n, n, 167) and bool(torch.isfinite(x).all())
        if n <= 3:                                             # no frame anywhere: dU = normalize(0) = 0, Q = normalize(0, 0, 0, 1/2)
            assert bool((O == 0).all()) and bool((x[..., 160:163] == 0).all())
            assert torch.equal(x[..., 163:], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(n, n, 4))
        E = car.edge_features(W, Ca, t(m["mask"]).double(), t(m["ridx"]), t(m["cenc"]), ci.host_graph(m))
        assert bool(torch.isfinite(E).all())


def test_the_classification_of_the_committed_cases_does_not_move():
    """frame_conditioned holds on every row of the fixtures that have a missing C-alpha or short chains, so the second rule leaves
    the well-conditioned sets of the existing cases as they are (and tiny_member(5, 55, masked=2), the input that showed the gap, fails it)."""
    from conftest import load_golden
    from test_ca_host import CASES
    for case in CASES:
        g = load_golden("ca_" + case)
        for b in range(g["S"].shape[0]):
            assert bool(ci.frame_conditioned(torch.from_numpy(g["Ca"][b]).double()).all()), (case, b)
    from tiny_backbones import tiny_member
    bad = ci.member(*tiny_member(5, 55, masked=2))
    fc = ci.frame_conditioned(torch.from_numpy(bad["Ca"]).double())
    assert fc.tolist() == [True, False, True, True, True]
    ei = ci.host_graph(bad)
    old = car.well_conditioned(car.frames(torch.from_numpy(bad["Ca"]).double()), ei).numpy()
    tr = ci.member_truth(ca_weights(), bad, ei)
    assert float(tr["d32"][old].max()) > 1e-2 and float(tr["d32"][tr["well"]].max()) <= 1e-5


def test_window_pack_is_exact_and_both_precisions_keep_the_same_steps():
    pack, steps = ci.window_pack()
    lengths = ci.window_lengths()
    assert len(lengths) == 7 and all(len(m["S"]) <= 7 for m in pack)
    for name, s in lengths.items():
        assert s.dtype == np.float32 and (float(s) * 2.0 ** 22).is_integer(), name
        assert np.sqrt(np.float32(s * s), dtype=np.float32) == s, name            # the float32 norm of a step along one axis is its length
    assert float(lengths["below_3.6"]) < float(lengths["3.6"]) < 3.6 < float(lengths["above_3.6"])   # 3.6f lies below 3.6: never kept
    assert float(lengths["below_4.0"]) < 4.0 == float(lengths["4.0"]) < float(lengths["above_4.0"])
    as_prev, as_next = set(), set()
    for m, st, names in zip(pack, steps, ci.WINDOW_SEGMENTS):
        assert np.array_equal(np.diff(m["Ca"], axis=0).view(np.uint32), st.view(np.uint32))   # bit for bit
        assert np.abs(m["Ca"]).max() <= 4.0 + 2.0 ** -21
        for k, name in enumerate(names):
            assert (np.abs(st[k]) == lengths[name]).sum() == 1 and (st[k] != 0).sum() == 1 and st[k][k % 3] != 0
        Ca = torch.from_numpy(m["Ca"])
        dX = Ca[1:] - Ca[:-1]
        assert torch.equal(torch.sqrt((dX * dX).sum(-1)), torch.tensor([float(lengths[k]) for k in names]))
        want = [k in ci.WINDOW_KEPT for k in names]
        assert ci.kept_steps(Ca).tolist() == want and ci.kept_steps(Ca.double()).tolist() == want
        O32, O64 = car.frames(Ca), car.frames(Ca.double())
        assert torch.equal(O32 == 0, O64 == 0) and float((O32.double() - O64).abs().max()) <= 1e-6
        assert bool(ci.frame_conditioned(Ca.double()).all())
        n = len(names) + 1
        as_prev |= {names[i - 1] for i in range(1, n - 2)}
        as_next |= {names[i] for i in range(1, n - 2)}
        # what a kept or dropped step does to the frame rows (o, n, o x n) of the two rows it belongs to
        for i in range(1, n - 2):
            rows = (O64[i].view(3, 3) != 0).any(-1).tolist()
            assert rows == [want[i - 1] or want[i], want[i - 1] and want[i], want[i - 1] and want[i]], (names, i)
    assert as_prev == set(lengths) and as_next == set(lengths)    # every length occurs as U[i-1] and as U[i] of a framed row
