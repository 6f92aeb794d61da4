"""Host side of tied sampling and the PSSM terms (no GPU): the torch restatement (tests/tied_restatement.py) against the imported
reference's tied_sample fixtures (tests/golden/make_tied_sample_golden.py); tied_decoding_order and pack_tied_args against the
reference's recorded order and expressions; the reference-named signatures; design.tied_featurize against the reference's 20-tuple.

Comparison line for probs: 1e-5 / temperature / min_den — the project's 1e-5 line on log-probabilities, scaled by the softmax's
1 / temperature and by a renormalisation's 1 / denominator (min_den is read from the fixture; 1 where nothing renormalises). The
weights of a group satisfy sum |weight| <= 1 in every fixture, so the weighted sum of logits adds nothing."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, weights_for_case
from masked_backbones import layout_arrays
from tied_restatement import sample_tied_chains

TOL_INTERMEDIATE = 1e-5
MARGIN = 1e-3
TIED_CASES = {"tied_syn_L32": "syn_L32", "tied_2OCJ_AB": "2OCJ_AB", "tied_msk_L56_2ch": "msk_L56_2ch"}


def inputs_of(fixture):
    """The structure of a tied fixture with the graph the reference sampled on."""
    struct = TIED_CASES.get(fixture, "syn_L32")
    if not struct.startswith("msk_"):
        return load_golden(struct)
    X, S, mask, ridx, cenc = layout_arrays(struct)
    return dict(X=X, S=S, mask=mask, residue_idx=ridx, chain_enc=cenc, weight_seed=np.int64(0), E_idx=load_golden(fixture)["E_idx"])


def groups_of(o):
    return [[int(k) for k in row if k >= 0] for row in o["tied_pos"]]


def packed_of(g, o):
    from thermompnn_amd.design import pack_tied_args
    N = o["randn"].shape[0]
    t = torch.from_numpy
    pssm = "pssm_coef" in o
    return pack_tied_args(t(o["randn"]), t(o["chain_mask"]), t(np.tile(g["mask"][None], (N, 1))), float(o["temperature"]), o["omit_AAs"],
                          o["bias_AAs"], t(o["chain_M_pos"]), t(o["omit_AA_mask"]) if "omit_AA_mask" in o else None, t(o["bias_by_res"]),
                          groups_of(o), t(o["tied_beta"]), t(o["pssm_coef"]) if pssm else None, t(o["pssm_bias"]) if pssm else None,
                          float(o["pssm_multi"]) if pssm else None, pssm, t(o["pssm_log_odds_mask"]) if pssm else None, pssm)


@pytest.mark.parametrize("fixture", ["tied_syn_L32", "tied_msk_L56_2ch"])
def test_restatement_reproduces_the_reference(fixture):
    g, o = inputs_of(fixture), load_golden(fixture)
    temperature, min_den = float(o["temperature"]), float(o["min_den"])
    assert float(o["min_margin"]) >= MARGIN and min_den >= 0.25
    pk = packed_of(g, o)
    first = lambda a: None if a is None else a[0].numpy()
    r = sample_tied_chains(weights_for_case(g), g, pk["decoding_order"].numpy(), pk["close"].numpy(), o["S_true"], o["free"], o["u"], temperature,
                           weight=pk["weight"].numpy(), bias=first(pk["bias"]), allowed=first(pk["allowed"]), pssm_mix=first(pk["pssm_mix"]),
                           pssm_bias=first(pk["pssm_bias"]), pssm_keep=first(pk["pssm_keep"]))
    line = TOL_INTERMEDIATE / temperature / min_den
    err = float(np.abs(r["probs"].astype(np.float64) - o["probs"]).max())
    print(f"{fixture}: probs {err:.3e} (line {line:g}), min margin {r['min_margin']:.2e}, non-zero rows {int((o['probs'].sum(-1) > 0).sum())}")
    assert np.array_equal(r["S"], o["S"])
    assert err <= line
    for grp in groups_of(o):                                        # a group shares its letter; a dead group's probs rows are 0
        assert (o["S"][:, grp] == o["S"][:, grp[:1]]).all()
        dead = any(g["mask"][k] == 0 for k in grp)
        assert ((o["probs"][:, grp] == 0).all() and (r["probs"][:, grp] == 0).all()) if dead else (o["probs"][:, grp].sum(-1) > 0.99).all()
    if fixture == "tied_msk_L56_2ch":
        assert int((o["probs"].sum(-1) > 0).sum()) == 72            # 18 live pairs x 2 members x 2 chains
        for grp in groups_of(o):
            masked = [k for k in grp if g["mask"][k] == 0]
            if masked:
                assert (o["S"][:, grp] == o["S_true"][:, masked[:1]]).all()
    else:
        assert (o["probs"][:, [5, 20]].sum(-1) > 0.99).all()        # probs is written at fixed positions (:1492)
        assert np.array_equal(o["S"][:, [4, 20]], o["S_true"][:, [20, 20]])      # fixed CLOSING member: the group takes S_true there
        assert (o["S"][:, 5] == o["S"][:, 21]).all()                             # fixed non-closing member: drawn with its group


@pytest.mark.parametrize("fixture", list(TIED_CASES))
def test_tied_decoding_order_equals_the_reference(fixture):
    from thermompnn_amd.design import tied_decoding_order
    g, o = inputs_of(fixture), load_golden(fixture)
    pk = packed_of(g, o)
    assert np.array_equal(pk["decoding_order"].numpy(), o["decoding_order"])
    order, close = pk["decoding_order"][0].numpy(), pk["close"][0].numpy()
    assert close[-1] == 1 and set(close.tolist()) <= {0, 1}
    ends = np.nonzero(close)[0]
    runs = [order[a:b + 1].tolist() for a, b in zip(np.concatenate([[0], ends[:-1] + 1]), ends)]
    tied = groups_of(o)
    assert [r for r in runs if len(r) > 1] == [grp for grp in sorted(tied, key=lambda grp: order.tolist().index(grp[0])) if len(grp) > 1]
    assert sorted(k for r in runs for k in r) == list(range(len(order)))
    # weight = tied_beta / len(group) (:1464)
    size = np.ones(len(order), np.float32)
    for grp in tied:
        size[grp] = len(grp)
    assert np.array_equal(pk["weight"][0].numpy(), o["tied_beta"] / size)
    assert all(np.abs(pk["weight"][0].numpy()[r]).sum() <= 1.0 + 1e-6 for r in runs)


def test_tied_decoding_order_walks_and_refuses():
    from thermompnn_amd.design import tied_decoding_order
    order, close = tied_decoding_order([3, 0, 4, 1, 2, 5], [[4, 1], [5, 0, 2]])
    assert order.tolist() == [3, 5, 0, 2, 4, 1] and close.tolist() == [1, 0, 0, 1, 0, 1]
    order, close = tied_decoding_order(torch.tensor([2, 1, 0]), [])
    assert order.tolist() == [2, 1, 0] and close.tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="overlap"):
        tied_decoding_order([0, 1, 2, 3], [[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="repeated"):
        tied_decoding_order([0, 1, 2, 3], [[0, 1, 0]])
    with pytest.raises(ValueError, match="outside"):
        tied_decoding_order([0, 1, 2, 3], [[0, 4]])
    with pytest.raises(ValueError, match="outside"):
        tied_decoding_order([0, 1, 2, 3], [[-1, 2]])


def test_packing_uses_the_reference_expressions():
    g, o = inputs_of("tied_2OCJ_AB"), load_golden("tied_2OCJ_AB")
    pk = packed_of(g, o)
    T = float(o["temperature"])
    t = torch.from_numpy
    assert np.array_equal(pk["free"].numpy(), o["chain_mask"] * o["chain_M_pos"])
    want = t(o["bias_AAs"])[None, None, :] / T + t(o["bias_by_res"]) / T - t(o["omit_AAs"])[None, None, :] * 1e8       # :1469-1470
    assert float((pk["bias"] - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()) / 1e8)
    assert np.array_equal(pk["allowed"].numpy(), 1.0 - o["omit_AA_mask"])                                              # :1484
    assert np.array_equal(pk["pssm_mix"].numpy(), (float(o["pssm_multi"]) * t(o["pssm_coef"])).numpy())                 # :1475
    assert np.array_equal(pk["pssm_bias"].numpy(), o["pssm_bias"]) and np.array_equal(pk["pssm_keep"].numpy(), o["pssm_log_odds_mask"])
    assert pk["close"].dtype == torch.int32 and pk["close"].shape == o["decoding_order"].shape
    plain = packed_of(inputs_of("tied_syn_L32"), load_golden("tied_syn_L32"))
    assert plain["pssm_mix"] is None and plain["pssm_bias"] is None and plain["pssm_keep"] is None and plain["allowed"] is None


def test_signatures_are_the_reference_ones_plus_the_stream():
    from thermompnn_amd.design import ProteinMPNNDesign
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    head = ["self", "X", "randn", "S_true", "chain_mask", "chain_encoding_all", "residue_idx", "mask", "temperature", "omit_AAs_np",
            "bias_AAs_np", "chain_M_pos", "omit_AA_mask", "pssm_coef", "pssm_bias", "pssm_multi", "pssm_log_odds_flag",
            "pssm_log_odds_mask", "pssm_bias_flag"]
    names = lambda f: [p.name for p in inspect.signature(f).parameters.values()]
    assert names(ProteinMPNNDesign.tied_sample) == head + ["tied_pos", "tied_beta", "bias_by_res", "generator", "uniforms"]
    assert names(ProteinMPNNDesign.sample) == head + ["bias_by_res", "generator", "uniforms"]
    assert issubclass(ProteinMPNNDesign, ProteinMPNN) and not hasattr(ProteinMPNN, "tied_sample")
    from thermompnn_amd import design, pdb_io
    assert names(design.tied_featurize) == names(pdb_io.tied_featurize)


def _parse_AB():
    from thermompnn_amd.pdb_io import alt_parse_PDB
    return alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A", "B"])[0]


def test_tied_featurize_reproduces_the_reference():
    from thermompnn_amd import design
    z = load_golden("tied_featurize_2OCJ_AB")
    spec, lists = json.loads(str(z["spec"])), json.loads(str(z["lists"]))
    pdb = _parse_AB()
    name = pdb["name"]
    assert name in spec["chain_dict"]
    pssm = {name: {c: {k: z[f"{k}_{c}"] for k in ("pssm_coef", "pssm_bias", "pssm_log_odds")} for c in "AB"}}
    by_res = {name: {c: z[f"bias_by_res_{c}"] for c in "AB"}}
    out = design.tied_featurize([pdb], "cpu", spec["chain_dict"], spec["fixed_position_dict"], spec["omit_AA_dict"],
                                spec["tied_positions_dict"], pssm, by_res)
    assert len(out) == 20
    for i, v in enumerate(out):
        if f"out{i}" in z:
            got = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            assert got.shape == z[f"out{i}"].shape, i
            if i == 0:
                assert np.abs(got - z["out0"]).max() <= 1e-6, i     # coordinates: the parser's own check elsewhere
            else:
                assert np.array_equal(got, z[f"out{i}"]), i
        else:
            assert json.loads(json.dumps(v)) == lists[str(i)], i
    assert out[14] == [[[0, 194], [1, 2, 195], [9, 10, 205]]]
    assert out[19][1] == 0.5 and out[19][2] == -0.25 and out[19][195] == 1.5 and float(out[19].sum()) == 388 - 3 + 1.75
    assert out[11].sum() == 3 * 3 + 1 + 2 * 2 and out[10][0, [0, 1, 49, 203]].sum() == 0


def test_tied_featurize_without_dictionaries_is_the_packer():
    from thermompnn_amd import design, pdb_io
    pdb = _parse_AB()
    fixed = {pdb["name"]: {"A": [3], "B": []}}
    a = design.tied_featurize([pdb], "cpu", None, fixed)
    b = pdb_io.tied_featurize([pdb], "cpu", None, fixed)
    for x, y in zip(a, b):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    with pytest.raises(NotImplementedError):
        pdb_io.tied_featurize([pdb], "cpu", None, tied_positions_dict={pdb["name"]: []})
