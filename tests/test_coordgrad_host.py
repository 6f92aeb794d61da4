"""tests/coordgrad_restatement.py against central differences in float64, on the host: the restatement is what the GPU tests hold
tmpnn_seqloss_backward_x to on the layouts the reference's goldens cannot reach, so its autograd dX is checked here against the
function itself, under the same contract (the graph given, D_max of _dist a constant)."""
import numpy as np
import pytest
import torch

from coordgrad_restatement import d_max_of, dX_f64, objective
from masked_backbones import layout_arrays

STEP = 1e-5            # Angstrom
AGREE = 1e-6           # x max|dX|. A central difference at h = 1e-5 is off by h^2 f''' / 6 ~ 1e-10 and by rounding eps |f| / h ~
                       # 1e-16 * 1e2 / 1e-5 = 1e-9; max|dX| is 1.2 .. 6.3 on these layouts, so the line sits 1000 x above both.


def _case(name, K=48):
    from oracle import thermompnn_oracle as O
    from thermompnn_amd.weights import synthetic_state_dict
    X, S, mask, ridx, cenc = layout_arrays(name)
    L = len(S)
    Ei = O.knn(torch.from_numpy(X)[None, :, 1], torch.from_numpy(mask)[None], K)[1][0].numpy()
    ranks = np.random.default_rng(3).permutation(L)
    dlp = np.random.default_rng(1).normal(size=(L, 21))
    return synthetic_state_dict(0, "mpnn"), (X, S, mask, ridx, cenc, Ei, ranks, dlp)


def _selected_masked_row(mask, Ei):
    """A masked residue that an unmasked row lists as a neighbour (None when there is none)."""
    for j in np.nonzero(mask == 0)[0]:
        if any(j in Ei[i] for i in np.nonzero(mask > 0)[0]):
            return int(j)
    return None


@pytest.mark.parametrize("name,n_coords", [("msk_L2", None), ("msk_L17", 24), ("msk_L40", 24)])
def test_autograd_dX_matches_central_differences(name, n_coords):
    """Every coordinate at L = 2; at L = 17 (K = 17) and the masked L = 40 (K = 40) a seeded sample of ``n_coords`` coordinates, all 12
    coordinates of a masked residue that unmasked rows select, and four random directions over the whole tensor. D_max is held at
    its value at X, which is what `detached` means for a difference quotient."""
    sd, (X, S, mask, ridx, cenc, Ei, ranks, dlp) = _case(name)
    L = len(S)
    g = dX_f64(sd, X, S, mask, ridx, cenc, Ei, ranks, dlp)
    gmax = float(np.abs(g).max())
    assert g.shape == (L, 4, 3) and gmax > 0 and np.isfinite(g).all()
    d_max = d_max_of(X, mask)
    X0 = torch.from_numpy(X).double()

    def f(Xp):
        with torch.no_grad():
            return float(objective(sd, Xp, S, mask, ridx, cenc, Ei, ranks, dlp, d_max=d_max))

    rng = np.random.default_rng(5)
    flat = list(range(L * 12)) if n_coords is None else sorted(rng.choice(L * 12, n_coords, replace=False).tolist())
    j = _selected_masked_row(mask, Ei)
    if n_coords is not None:
        assert j is not None
        flat = sorted(set(flat) | set(range(12 * j, 12 * j + 12)))
    worst = 0.0
    for c in flat:
        e = torch.zeros(L * 12, dtype=torch.float64)
        e[c] = STEP
        fd = (f(X0 + e.view(L, 4, 3)) - f(X0 - e.view(L, 4, 3))) / (2 * STEP)
        worst = max(worst, abs(fd - g.reshape(-1)[c]))
    for _ in range(4):
        v = torch.from_numpy(rng.normal(size=(L, 4, 3)))
        v = v / v.norm()
        fd = (f(X0 + STEP * v) - f(X0 - STEP * v)) / (2 * STEP)
        worst = max(worst, abs(fd - float((torch.from_numpy(g) * v).sum())))
    print(f"{name}: max|dX| {gmax:.4g}, worst |central difference - autograd| / max|dX| {worst / gmax:.3g} over {len(flat)} coordinates")
    assert worst <= AGREE * gmax
    if j is not None and n_coords is not None:           # the selected masked row's (zero) coordinates carry a gradient
        assert float(np.abs(g[j]).max()) > 1e-3 * gmax


def test_attached_D_max_is_the_same_gradient_where_no_masked_residue_is_selected():
    """msk_L56 at K = 30 has 46 unmasked residues: an unmasked row's 30 neighbours are all unmasked, so the reference's definition
    (D_max with its graph) and the contract (D_max detached) give the same bits. On msk_L40 at K = L = 40 every unmasked row lists
    masked residues and the two differ: the reference leaks their pair-0 gradient into the row's farthest valid residue."""
    sd, (X, S, mask, ridx, cenc, Ei, ranks, dlp) = _case("msk_L56", 30)
    live = mask > 0
    assert Ei.shape == (56, 30) and live[Ei[live]].all()
    a = dX_f64(sd, X, S, mask, ridx, cenc, Ei, ranks, dlp, attach_dmax=True)
    d = dX_f64(sd, X, S, mask, ridx, cenc, Ei, ranks, dlp)
    assert np.array_equal(a, d) and float(np.abs(d).max()) > 0
    assert not np.abs(d[~live]).any()                    # rows that reach the loss through no edge: exactly 0
    sd, (X, S, mask, ridx, cenc, Ei, ranks, dlp) = _case("msk_L40")
    a = dX_f64(sd, X, S, mask, ridx, cenc, Ei, ranks, dlp, attach_dmax=True)
    d = dX_f64(sd, X, S, mask, ridx, cenc, Ei, ranks, dlp)
    assert float(np.abs(a - d).max()) > 1e-3 * float(np.abs(d).max())


def test_golden_files_hold_what_the_tests_read():
    """tests/golden/coordgrad_*.npz: dX [L,4,3] float64 per tag, the graph, the loss of the run they came from (the same loss as the
    parameter-gradient fixtures of the same recipe), d32 on the heavy draw, and tensors only."""
    from conftest import load_golden
    for kind, cases in (("seqloss", ("2OCJ_A", "2OCJ_A_gap", "2OCJ_A_fixed", "2OCJ_A_hot")), ("finetune", ("2OCJ_A", "2OCJ_A_hot"))):
        for case in cases:
            g, parent = load_golden(f"coordgrad_{kind}_{case}"), load_golden(f"{kind}_{case}")
            tags = ("drawn",) if case.endswith("hot") else ("ones", "drawn")
            assert np.array_equal(g["E_idx"], parent["E_idx"])
            for tag in tags:
                dX = g[f"{tag}_dX"]
                assert dX.dtype == np.float64 and dX.shape == (g["E_idx"].shape[0], 4, 3) and np.isfinite(dX).all()
                assert float(g[f"{tag}_loss"]) == float(parent[f"{tag}_loss"])
                assert (f"{tag}_dX_d32" in g) == case.endswith("hot")
