"""Host side of order-masked decoding (no GPU): the torch restatement of the rank-select decoder against the imported
reference's conditional_probs / unconditional_probs fixtures (tests/golden/make_ordered_golden.py), decoding_ranks against
the reference's stored decoding orders, the signatures of the two new ProteinMPNN methods, and argument validation of
tmpnn_decode_ordered."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden, tol_scale, weights_for_case
from ordered_restatement import conditional_ranks, ordered_decode

TOL_INTERMEDIATE = 1e-5   # abs; the line test_oracle_golden.py holds the oracle's log_probs to
T_MAX = (1 << 31) // (48 * 4) - 1
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -4, -2
CASES = ["syn_L32", "2OCJ_A", "2OCJ_A_gap"]


@pytest.fixture(scope="module")
def lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    """fp32, on the fixture's own E_idx: every looped row of cond (one decode per position, the position last), the looped rows of
    cond_backbone_only (the position first) and uncond (all ranks equal). Rows that are not looped over are exactly 0."""
    g, o = load_golden(case), load_golden("ordered_" + case)
    W = weights_for_case(g)
    L = len(g["S"])
    looped = np.nonzero(g["mask"] == 1)[0]
    S = g["S"].astype(np.int64)
    tol = lambda ref: TOL_INTERMEDIATE * tol_scale(g, ref)
    unc = ordered_decode(W, g, S[None], np.zeros((1, L), np.int64), g["E_idx"])["log_probs"][0]
    np.testing.assert_allclose(unc, o["uncond"], atol=tol(o["uncond"]), rtol=0)
    ranks = np.stack([conditional_ranks(o["randn"], int(p), L) for p in looped])
    lp = ordered_decode(W, g, np.tile(S, (len(looped), 1)), ranks, g["E_idx"])["log_probs"]
    cond = np.zeros((L, 21), np.float32)
    cond[looped] = lp[np.arange(len(looped)), looped]
    np.testing.assert_allclose(cond, o["cond"], atol=tol(o["cond"]), rtol=0)
    dead = np.setdiff1d(np.arange(L), looped)
    assert (o["cond"][dead] == 0).all() and (o["cond_backbone_only"][dead] == 0).all()
    # backbone_only: the position decoded first. Three positions through their own ranks, all of them through the one decode
    pick = [int(p) for p in o["order_pos"]]
    bb = ordered_decode(W, g, np.tile(S, (3, 1)), np.stack([conditional_ranks(o["randn"], p, L, True) for p in pick]), g["E_idx"])["log_probs"]
    for k, p in enumerate(pick):
        np.testing.assert_allclose(bb[k, p], o["cond_backbone_only"][p], atol=tol(o["cond_backbone_only"]), rtol=0)
    np.testing.assert_allclose(unc[looped], o["cond_backbone_only"][looped], atol=tol(o["cond_backbone_only"]), rtol=0)
    # the modes are far apart on the scale of the line: a test at 1e-5 tells them apart
    assert np.abs(o["cond"] - o["uncond"])[looped].max() > 1e-2


@pytest.mark.parametrize("case", CASES)
def test_decoding_ranks_inverts_the_stored_decoding_order(case):
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    o = load_golden("ordered_" + case)
    L = o["randn"].shape[1]
    for p, order in zip(o["order_pos"], o["decoding_order"]):
        order_mask = torch.zeros(L)
        order_mask[int(p)] = 1.0
        rank = decoding_ranks(order_mask[None], torch.from_numpy(o["randn"]))
        assert rank.dtype == torch.int32 and rank.shape == (1, L)
        assert (rank[0, torch.from_numpy(order.astype(np.int64))] == torch.arange(L, dtype=torch.int32)).all()
        assert (rank[0].numpy() == conditional_ranks(o["randn"], int(p), L)).all()
    many = decoding_ranks(torch.eye(L), torch.from_numpy(o["randn"]))            # one row per looped position, as conditional_probs calls it
    assert (many[int(o["order_pos"][1])].numpy() == conditional_ranks(o["randn"], int(o["order_pos"][1]), L)).all()


def test_signatures_are_the_reference_ones():
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ProteinMPNN.conditional_probs) == [("self", E), ("X", E), ("S", E), ("mask", E), ("chain_M", E), ("residue_idx", E),
                                                  ("chain_encoding_all", E), ("randn", E), ("backbone_only", False)]
    assert sig(ProteinMPNN.unconditional_probs) == [("self", E), ("X", E), ("mask", E), ("residue_idx", E), ("chain_encoding_all", E)]


def test_symbols_are_exported_and_bound(lib):
    from thermompnn_amd import _lib
    for name in ("tmpnn_decode_ordered", "tmpnn_decode_ordered_workspace_bytes"):
        assert name in _lib.SIGNATURES
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == (15 if name == "tmpnn_decode_ordered" else 2)
    assert lib.tmpnn_version() == 200


def test_ordered_workspace_size(lib):
    size, plain = lib.tmpnn_decode_ordered_workspace_bytes, lib.tmpnn_decode_variants_workspace_bytes
    assert [size(256, v) for v in (0, 1, 2, 37, 64)] == sorted(size(256, v) for v in (0, 1, 2, 37, 64))
    # the plain decode's buffers + slot V of the projection table + one 8-byte word per row + the fp32 form's list
    assert size(256, 8) >= plain(256, 8) + 256 * (256 * 4 + 48 * 4) + 256 * 8 * 8
    assert size(-1, 1) == 0 and size(1, -1) == 0
    assert size(256, T_MAX // 256 + 1) == 0
    assert plain(1 << 23, 1) > 0 and size((1 << 23) - 1, 1) > 0 and size(1 << 23, 1) == 0      # (V + 1) T 256 stays below 2^32 floats


def test_decode_ordered_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p
    w, buf = p(256), p(256)          # never dereferenced: validation comes first
    T, V = 32, 3
    need = lib.tmpnn_decode_ordered_workspace_bytes(T, V)
    args = lambda **k: [k.get("w", w), k.get("ctx", buf), k.get("ctx_bytes", 1 << 30), k.get("S", buf), k.get("rank", buf), k.get("V", V),
                        k.get("mask", buf), k.get("T", T), None, k.get("hidden", None), k.get("lp", buf), None, k.get("ws", buf),
                        k.get("ws_bytes", need), None]
    f = lib.tmpnn_decode_ordered
    err = lambda: lib.tmpnn_last_error().decode()
    assert f(*args(w=None)) == E_INVALID and "null" in err()
    assert f(*args(S=None)) == E_INVALID and "null" in err()
    assert f(*args(rank=None)) == E_INVALID and "null" in err()
    assert f(*args(mask=None)) == E_INVALID
    assert f(*args(V=-1)) == E_INVALID and "V=-1" in err()
    assert f(*args(T=-1)) == E_INVALID
    assert f(*args(lp=None)) == E_INVALID and "no output" in err()
    assert f(*args(ctx=None)) == E_INVALID and "ctx" in err()
    assert f(*args(ctx_bytes=lib.tmpnn_encode_bytes(T) - 1)) == E_WORKSPACE and "ctx" in err()
    assert f(*args(ws=None)) == E_WORKSPACE
    assert f(*args(ws_bytes=need - 1)) == E_WORKSPACE and "workspace" in err()
    assert f(*args(ws_bytes=lib.tmpnn_decode_variants_workspace_bytes(T, V))) == E_WORKSPACE
    assert f(*args(V=T_MAX // T + 1, ws_bytes=1 << 62)) == E_UNSUPPORTED and "chunks" in err()
    assert f(*args(V=1, T=1 << 23, ws_bytes=1 << 62)) == E_UNSUPPORTED and "(V + 1)" in err()      # slot V would not be addressable
    assert f(*args(V=0, S=None, rank=None, ctx=None, ws=None, lp=None, mask=None, w=w)) == 0               # nothing to decode: a no-op
    assert f(*args(T=0, S=None, rank=None, ctx=None, ws=None, lp=None, mask=None)) == 0


def test_baseline_rejects_an_unknown_scoring():
    from thermompnn_amd.thermompnn_benchmarking import ProteinMPNNBaseline
    with pytest.raises(ValueError, match="bogus"):
        ProteinMPNNBaseline(None, scoring="bogus")
