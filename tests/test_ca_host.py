"""The C-alpha-only flavour without a GPU: the torch restatement of the featurizer against the imported reference's float64 rows,
the ca_only parameter tree, the parser / packer with ca_only=True, the unchanged ca_only=False outputs, and the C-ABI's argument
checks. Fixtures: tests/golden/make_ca_golden.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ca_restatement as car
from conftest import GOLDEN, load_golden

CASES = ["syn_L32", "syn_L40", "msk_L40", "msk_L56_2ch", "pad_L32_L40", "2OCJ_A", "2OCJ_AB", "msk_L17", "msk_L47", "msk_L49"]


def ca_weights():
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0, "mpnn_ca")


def restated(g, b, dtype):
    t = torch.from_numpy
    return car.edge_features(ca_weights(), t(g["Ca"][b]).to(dtype), t(g["mask"][b]).to(dtype), t(g["residue_idx"][b].astype(np.int64)),
                             t(g["chain_enc"][b].astype(np.int64)), t(g["E_idx"][b].astype(np.int64)))


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_float64_reference(case):
    """The restatement, written from the specification, equals the reference's float64 E on the stored rows to 1e-12 (the generator
    asserted the same on every row), and in float32 it is as close to float64 as the reference-fp32 is, within the 2.5 x rule."""
    g = load_golden("ca_" + case)
    assert float(g["min_window_margin"]) >= 1e-3 and float(g["ill_fraction"]) <= 0.10
    for b in range(g["S"].shape[0]):
        E64 = restated(g, b, torch.float64)
        assert float((E64[g["rows"]] - torch.from_numpy(g["E64_rows"][b])).abs().max()) <= 1e-12
        well = car.well_conditioned(car.frames(torch.from_numpy(g["Ca"][b]).double()), torch.from_numpy(g["E_idx"][b].astype(np.int64)))
        d = (restated(g, b, torch.float32).double() - E64).abs().amax(-1)
        assert float(d[well].max()) <= 1e-5
        if (~well).any():
            assert float(d[~well].max()) <= 2.5 * float(g["ref32_ill"])


def test_segment_rule_padded_equals_alone_up_to_the_member_end():
    """The padded pair through the reference against each member alone: the longer member's rows are the same numbers; the shorter
    member's differ only where the rule says they may — its last two rows' frames and the neighbours that see them."""
    pad, alone = load_golden("ca_pad_L32_L40"), load_golden("ca_syn_L40")
    t = torch.from_numpy
    Ca = t(pad["Ca"][1]).double()
    assert np.array_equal(pad["Ca"][1], alone["Ca"][0])
    assert torch.equal(car.frames(Ca), car.frames(t(alone["Ca"][0]).double()))
    short = car.frames(t(pad["Ca"][0]).double())                       # 32 real rows inside a segment of 40
    own = car.frames(t(pad["Ca"][0][:32]).double())
    assert torch.equal(short[:30], own[:30]) and bool((own[30:] == 0).all())
    assert bool((short[30] != 0).any()) and bool((short[31, :3] != 0).any()) and bool((short[31, 3:] == 0).all()) and bool((short[32:] == 0).all())
    assert bool((car.frames(Ca[:2]) == 0).all()) and bool((car.frames(Ca[:1]) == 0).all()) and bool((car.frames(Ca[:3]) == 0).all())


def test_parameter_tree_is_the_reference_state_dict():
    from thermompnn_amd import weights
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    p = load_golden("ca_params")
    names, shapes = [str(n) for n in p["names"]], [tuple(s) for s in json.loads(str(p["shapes"]))]
    tree = weights.mpnn_param_shapes(ca_only=True)
    assert list(tree) == names and [tuple(v) for v in tree.values()] == shapes and len(tree) == 123
    assert weights.EDGE_IN_CA == 167 and tree["features.edge_embedding.weight"] == (128, 167)
    sd = ca_weights()
    assert weights.is_ca_state_dict(sd) and not weights.is_ca_state_dict(weights.synthetic_state_dict(0, "mpnn"))
    kept = weights.ca_engine_tensors(sd)
    assert len(kept) == 118 and list(kept) == list(weights.mpnn_param_shapes())
    assert set(sd) - set(kept) == {"features.node_embedding.weight", "features.norm_nodes.weight", "features.norm_nodes.bias", "W_v.weight",
                                   "W_v.bias"}
    m = ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0, ca_only=True)
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys and list(m.state_dict()) == names
    # the existing draws are what they were: the full tree's tensors do not move when the CA tree exists
    a, b = weights.synthetic_state_dict(0, "mpnn"), weights.synthetic_state_dict(0, "transfer")
    assert all(torch.equal(a[k], b["prot_mpnn." + k]) for k in a)
    g = load_golden("syn_L32")
    full = ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
    assert list(full.state_dict()) == list(weights.mpnn_param_shapes()) and int(g["weight_seed"]) == 0


def test_parser_and_packer_with_ca_only():
    from thermompnn_amd import design, pdb_io
    p = load_golden("ca_parse_2OCJ")
    for tag, path, chains in (("AB", os.path.join(GOLDEN, "2OCJ.pdb"), ["A", "B"]), ("gapA", os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"), "A")):
        d = pdb_io.alt_parse_PDB(path, chains, ca_only=True)[0]
        assert d["seq"] == str(p[tag + "_seq"])
        for ch in chains:
            assert list(d["coords_chain_" + ch]) == ["CA_chain_" + ch]
            got = np.asarray(d["coords_chain_" + ch]["CA_chain_" + ch], np.float64)
            want = p[f"{tag}_CA_chain_{ch}"]
            assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
        for fn in (pdb_io.tied_featurize, design.tied_featurize):
            f = fn([d], "cpu", None, ca_only=True)
            assert f[0].shape == p[tag + "_X"].shape and f[0].dim() == 3
            for i, key in ((0, "X"), (1, "S"), (2, "mask"), (4, "chain_M"), (5, "chain_enc"), (10, "chain_M_pos"), (12, "residue_idx")):
                assert np.array_equal(f[i].numpy(), p[f"{tag}_{key}"]), (tag, key)
        if tag == "gapA":                                      # the N atom of residue 120 is missing: present for a C-alpha model
            full = pdb_io.tied_featurize([pdb_io.alt_parse_PDB(path, chains)[0]], "cpu", None)
            assert int(f[2].sum()) == int(full[2].sum()) + 1
    with pytest.raises(NotImplementedError):
        pdb_io.alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), "A", ca_only=True, side_chains=True)


def test_ca_only_false_is_unchanged():
    from thermompnn_amd import pdb_io
    g, p = load_golden("2OCJ_AB"), load_golden("parser_2OCJ")
    d = pdb_io.alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A", "B"], ca_only=False)[0]
    assert d["seq"] == str(p["AB_seq"]) and sorted(d["coords_chain_A"]) == ["CA_chain_A", "C_chain_A", "N_chain_A", "O_chain_A"]
    f = pdb_io.tied_featurize([d], "cpu", None, ca_only=False)
    assert np.array_equal(f[0][0].numpy(), g["X"]) and np.array_equal(f[2][0].numpy(), g["mask"])
    assert np.array_equal(f[12][0].numpy(), g["residue_idx"]) and np.array_equal(f[5][0].numpy(), g["chain_enc"])
    # the C-alpha model's packer reads the same C-alpha atoms
    fc = pdb_io.tied_featurize([pdb_io.alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A", "B"], ca_only=True)[0]], "cpu", None, ca_only=True)
    assert np.array_equal(fc[0][0].numpy(), g["X"][:, 1])


def test_cabi_sizes_and_argument_errors():
    """The CA entries check their arguments before any launch; the full-backbone constants keep their values."""
    from thermompnn_amd import _lib
    lib = _lib.load()
    tables = (66 * 128 + 3 * 21 * 128 + 128 * 160) * 4
    assert lib.tmpnn_weights_ca_packed_bytes_p(b"fp32") == lib.tmpnn_weights_ca_packed_bytes_p(b"bf16x3") == tables
    assert lib.tmpnn_weights_ca_packed_bytes_p(b"f16x2") == tables + (122 - 12 - 2) * 65536
    assert lib.tmpnn_weights_ca_packed_bytes_p(b"fp64") == 0
    assert lib.tmpnn_weights_ca_packed_bytes_p(b"f16x2") < lib.tmpnn_weights_packed_bytes()
    assert [lib.tmpnn_tensor_numel_ca(i) for i in (0, 2, 117)] == [16 * 66, 128 * 167, 21] and lib.tmpnn_tensor_numel(2) == 128 * 416
    assert lib.tmpnn_tensor_numel_ca(118) == -1 and lib.tmpnn_tensor_numel_ca(-1) == -1
    assert all(lib.tmpnn_tensor_numel_ca(i) == lib.tmpnn_tensor_numel(i) for i in range(118) if i != 2)
    assert lib.tmpnn_num_tensors() == 130 and lib.tmpnn_version() == 200 and lib.tmpnn_weights_is_ca(None) == 0
    h = C.c_void_p()
    arr = (C.c_void_p * 130)(*([16] * 130))
    rc = lib.tmpnn_weights_create_ca(C.byref(h), arr, 130, C.c_void_p(16), 1 << 30, b"f16x2", None)      # head tensors: no CA flavour
    assert rc == -1 and b"118" in lib.tmpnn_last_error() and not h.value
    rc = lib.tmpnn_weights_create_ca(C.byref(h), arr, 118, C.c_void_p(16), 1 << 30, b"fp64", None)
    assert rc == -1 and b"unknown precision" in lib.tmpnn_last_error()
    rc = lib.tmpnn_weights_create_ca(C.byref(h), arr, 118, C.c_void_p(16), 1024, b"fp32", None)
    assert rc == -4 and b"packed buffer" in lib.tmpnn_last_error()
    assert lib.tmpnn_ca_frames(None, None, 1, 10, None, None) == -1 and b"null" in lib.tmpnn_last_error()
    assert lib.tmpnn_ca_frames(None, None, 0, 0, None, None) == 0                     # an empty batch is a no-op
    assert lib.tmpnn_ca_frames(None, None, 1, -1, None, None) == -1
    assert lib.tmpnn_edge_featurize_ca(None, None, None, None, None, 1, None, None, None, 4, None, None, None) == -1


def test_ca_model_has_no_cpu_path_and_checks_its_coordinates():
    """(A CA handle with head tensors is refused by the C-ABI above; a CA handle with a ddg output needs a handle, so a GPU:
    test_gpu_ca.test_ddg_and_the_plain_featurizer_entry_are_refused.)"""
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    m = ProteinMPNN(21, 128, 128, 128, k_neighbors=30, augment_eps=0.0, ca_only=True)
    assert m.ca_only and m.k_neighbors == 30
    args = (torch.zeros(1, 8, dtype=torch.long), torch.ones(1, 8), torch.ones(1, 8), torch.arange(8)[None], torch.ones(1, 8, dtype=torch.long), None)
    with pytest.raises(RuntimeError, match="MI355X"):            # no CPU path for this flavour either
        m(torch.zeros(1, 8, 3), *args)
    with pytest.raises(ValueError, match=r"\[B, L, 3\]"):         # full-backbone coordinates handed to a CA model
        m._backbone(torch.zeros(1, 8, 4, 3))
