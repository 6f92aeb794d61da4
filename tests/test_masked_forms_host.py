"""The inputs of tests/test_gpu_masked_forms.py, checked on the host (no GPU): every layout of tests/masked_backbones.py puts masked
residues into the neighbour lists of its unmasked rows, layout_arrays is what the PDB reader gives, and the oracle's own fp32
rounding leaves two thirds of the project's lines to the kernels."""
import numpy as np
import pytest
import torch

from masked_backbones import CHAIN_CUT, LAYOUTS, SEEN, layout_arrays, oracle_trace, variants_of, write_layout

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for decoder states and log-probabilities
TOL_DDG = 1e-4            # kcal/mol
MOVES = 1e-2              # test_gpu_variants.MOVES
NAMES = sorted(LAYOUTS)


def test_the_set_of_layouts():
    shape = {n: (LAYOUTS[n][0], len(LAYOUTS[n][2]) + len(LAYOUTS[n][3])) for n in NAMES}
    assert shape == {"msk_L2": (2, 1), "msk_L17": (17, 4), "msk_L47": (47, 3), "msk_L49": (49, 4), "msk_L40": (40, 10),
                     "msk_L56": (56, 10), "msk_L56_2ch": (56, 10)}
    assert all(L - n < 48 for L, n in shape.values())                     # fewer than 48 unmasked residues
    a, b = layout_arrays("msk_L56"), layout_arrays("msk_L56_2ch")
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    cut = CHAIN_CUT["msk_L56_2ch"]
    assert b[4].tolist() == [1] * cut + [2] * (56 - cut) and b[3][cut] - b[3][cut - 1] == 101 and (a[4] == 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_unmasked_rows_list_masked_residues(name):
    from oracle import thermompnn_oracle as orc
    X, S, mask, _, _ = layout_arrays(name)
    L = len(S)
    _, E_idx = orc.knn(torch.from_numpy(X)[None, :, 1], torch.from_numpy(mask)[None], 48)
    E_idx = E_idx[0].numpy()
    assert E_idx.shape == (L, min(48, L))
    live, dead = np.nonzero(mask > 0)[0], set(np.nonzero(mask == 0)[0].tolist())
    seen, letter = SEEN[name]
    assert len(live) and dead and mask[seen] == 0 and S[seen] < 20 and letter < 20 and letter != S[seen]
    for i in live:
        assert set(E_idx[i].tolist()) & dead, f"row {i} lists no masked residue"
    assert any(seen in E_idx[i] for i in live)
    if name == "msk_L2":
        assert live.tolist() == [0] and sorted(E_idx[0].tolist()) == [0, 1]
    if name == "msk_L49":      # 3 of the 4 masked residues, whichever win the tie (4 where the farthest unmasked one, AT D_max, loses it)
        assert all(len(set(E_idx[i].tolist()) & dead) in (3, 4) for i in live)
    # the SEEN residue's letter reaches unmasked rows of the reference: the GPU test asserts the same of the device
    wt = oracle_trace(name)["ddg"]
    sub = oracle_trace(name, variants_of(name)["seen_masked_substitution"])["ddg"]
    assert float(np.abs(sub - wt)[live].max()) > MOVES


@pytest.mark.parametrize("name", [n for n in NAMES if n not in CHAIN_CUT])
def test_layout_arrays_are_what_the_pdb_reader_gives(tmp_path, name):
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    pdb = alt_parse_PDB(write_layout(name, tmp_path), ["A"])
    f = tied_featurize(pdb, "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask, ridx, cenc = layout_arrays(name)
    for got, want in ((f[0][0], X), (f[1][0], S), (f[2][0], mask), (f[12][0], ridx), (f[5][0], cenc)):
        assert got.numpy().dtype == want.dtype
        np.testing.assert_array_equal(got.numpy(), want)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_fp32_is_within_a_third_of_the_lines_of_float64(name):
    """The condition under which the fixed 1e-5 / 1e-4 lines of the GPU tests are fair on these layouts: the reference's own fp32
    evaluation (synthetic weight seed 0) is no further than a third of a line from its float64 evaluation on the same graph."""
    a = oracle_trace(name)
    b = oracle_trace(name, E_idx=a["E_idx"], f64=True)
    assert b["ddg"].dtype == np.float64 and np.array_equal(a["E_idx"], b["E_idx"])
    for what, tol in [(f"hV_dec{l}", TOL_INTERMEDIATE) for l in (1, 2, 3)] + [("log_probs", TOL_INTERMEDIATE), ("ddg", TOL_DDG)]:
        err = float(np.abs(a[what].astype(np.float64) - b[what]).max())
        print(f"{name}/{what}: |oracle fp32 - float64| = {err:.3e} (line {tol:g})")
        assert err <= tol / 3.0, (name, what, err)
