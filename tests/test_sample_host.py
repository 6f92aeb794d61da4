"""Host side of autoregressive sampling (no GPU): the torch restatement of a chain (tests/sample_restatement.py, one teacher-forced
decode per step with the project's draw rule) against the imported reference's ProteinMPNN.sample fixtures
(tests/golden/make_sample_golden.py), and ProteinMPNN.sample's host-side packing of order / free / bias / allowed against the
reference's expressions."""
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden, weights_for_case
from masked_backbones import layout_arrays
from sample_restatement import cumulative, draw, inverse_orders, sample_chains

TOL_INTERMEDIATE = 1e-5   # the project's line on log-probabilities; a softmax at temperature T moves at most 1 / (2 T) per unit of logit
MARGIN = 1e-3             # every stored draw sits at least this far from a cumulative boundary
CASES = ["syn_L32", "2OCJ_A_gap", "msk_L40"]


def inputs_of(case):
    """The structure of a case with the graph the reference sampled on."""
    if not case.startswith("msk_"):
        return load_golden(case)
    X, S, mask, ridx, cenc = layout_arrays(case)
    return dict(X=X, S=S, mask=mask, residue_idx=ridx, chain_enc=cenc, weight_seed=np.int64(0), E_idx=load_golden("sample_" + case)["E_idx"])


def packed_of(g, o):
    from thermompnn_amd.protein_mpnn_utils import pack_sample_args
    N = o["randn"].shape[0]
    mask = np.tile(g["mask"][None], (N, 1))
    return pack_sample_args(torch.from_numpy(o["randn"]), torch.from_numpy(o["chain_mask"]), torch.from_numpy(mask), float(o["temperature"]),
                            o["omit_AAs"], o["bias_AAs"], torch.from_numpy(o["chain_M_pos"]),
                            torch.from_numpy(o["omit_AA_mask"]) if "omit_AA_mask" in o else None, torch.from_numpy(o["bias_by_res"]))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    g, o = inputs_of(case), load_golden("sample_" + case)
    temperature = float(o["temperature"])
    assert float(o["min_margin"]) >= MARGIN
    pk = packed_of(g, o)
    bias, allowed = pk["bias"][0].numpy(), None if pk["allowed"] is None else pk["allowed"][0].numpy()
    r = sample_chains(weights_for_case(g), g, o["decoding_order"], o["S_true"], o["free"], o["u"], temperature, bias, allowed)
    err = float(np.abs(r["probs"].astype(np.float64) - o["probs"]).max())
    print(f"{case}: probs {err:.3e} (line {TOL_INTERMEDIATE / temperature:g}), min margin {r['min_margin']:.2e}")
    assert np.array_equal(r["S"], o["S"])
    assert err <= TOL_INTERMEDIATE / temperature
    fixed = (o["free"] * g["mask"][None]) != 1
    assert fixed.any() or case == "syn_L32"
    assert (o["probs"][fixed] == 0).all() and (r["probs"][fixed] == 0).all() and np.array_equal(o["S"][fixed], o["S_true"][fixed])


@pytest.mark.parametrize("case", CASES)
def test_packing_uses_the_reference_expressions(case):
    g, o = inputs_of(case), load_golden("sample_" + case)
    pk = packed_of(g, o)
    T = float(o["temperature"])
    assert np.array_equal(pk["decoding_order"].numpy(), o["decoding_order"])            # the reference's own argsort, recorded
    assert np.array_equal(pk["free"].numpy(), o["chain_mask"] * o["chain_M_pos"]) and np.array_equal(pk["free"].numpy(), o["free"])
    # reference :1351-1352: logits / T - omit * 1e8 + bias_AAs / T + bias_by_res / T
    want = torch.from_numpy(o["bias_AAs"])[None, None, :] / T + torch.from_numpy(o["bias_by_res"]) / T - torch.from_numpy(o["omit_AAs"])[None, None, :] * 1e8
    assert pk["bias"].shape == o["bias_by_res"].shape
    assert float((pk["bias"] - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()) / 1e8)
    if "omit_AA_mask" in o:
        assert np.array_equal(pk["allowed"].numpy(), 1.0 - o["omit_AA_mask"])
    else:
        assert pk["allowed"] is None


def test_decoding_order_is_factored_out_of_decoding_ranks():
    from thermompnn_amd.protein_mpnn_utils import decoding_order, decoding_ranks
    gen = torch.Generator().manual_seed(1)
    randn, om = torch.randn(3, 40, generator=gen), (torch.rand(3, 40, generator=gen) > 0.3).float()
    order, ranks = decoding_order(om, randn), decoding_ranks(om, randn)
    assert np.array_equal(order.numpy(), torch.argsort((om + 0.0001) * torch.abs(randn)).numpy())
    assert np.array_equal(inverse_orders(order.numpy()), ranks.numpy())


def test_the_draw_rule():
    p = np.array([0.25, 0.0, 0.5, 0.25] + [0.0] * 17, np.float32)
    assert list(cumulative(p)[:4]) == [0.25, 0.25, 0.75, 1.0]
    assert [draw(p, u)[0] for u in (0.0, 0.2499, 0.25, 0.5, 0.7499, 0.75, 0.999)] == [0, 0, 2, 2, 2, 3, 3]      # c_a > u c_20, strictly
    assert draw(p, 1.0)[0] == 3                                     # rounding leaves none: the largest letter with probs > 0
    assert abs(draw(p, 0.3)[1] - 0.05) < 1e-6


def test_sample_signature_is_the_reference_one_plus_the_stream():
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    names = [p.name for p in inspect.signature(ProteinMPNN.sample).parameters.values()]
    ref = ["self", "X", "randn", "S_true", "chain_mask", "chain_encoding_all", "residue_idx", "mask", "temperature", "omit_AAs_np",
           "bias_AAs_np", "chain_M_pos", "omit_AA_mask", "pssm_coef", "pssm_bias", "pssm_multi", "pssm_log_odds_flag",
           "pssm_log_odds_mask", "pssm_bias_flag", "bias_by_res"]
    assert names[:len(ref)] == ref and names[len(ref):] == ["generator", "uniforms"]
    assert not hasattr(ProteinMPNN, "tied_sample")
