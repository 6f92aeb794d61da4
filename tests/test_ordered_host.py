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
from masked_backbones import layout_arrays
from ordered_restatement import conditional_ranks, ordered_decode

TOL_INTERMEDIATE = 1e-5   # abs; the line test_oracle_golden.py holds the oracle's log_probs to
T_MAX = (1 << 31) // (48 * 4) - 1
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -4, -2
CASES = ["syn_L32", "2OCJ_A", "2OCJ_A_gap"]
MASKED_CASES = ["msk_L17", "msk_L40", "msk_L56_2ch"]     # layouts of masked_backbones.py; their fixtures carry the reference's own E_idx


def inputs_of(case):
    """The structure of a case with the graph the reference decoded on: a golden fixture, or a masked layout with the E_idx its
    ordered fixture stores (torch.topk's choice among the masked residues tied at D_max)."""
    if case not in MASKED_CASES:
        return load_golden(case)
    X, S, mask, ridx, cenc = layout_arrays(case)
    return dict(X=X, S=S, mask=mask, residue_idx=ridx, chain_enc=cenc, weight_seed=np.int64(0),
                E_idx=load_golden("ordered_" + case)["E_idx"])


@pytest.fixture(scope="module")
def lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


@pytest.mark.parametrize("case", CASES + MASKED_CASES)
def test_restatement_reproduces_the_reference(case):
    """fp32, on the fixture's own E_idx: every looped row of cond (one decode per position, the position last), the looped rows of
    cond_backbone_only (the position first) and uncond (all ranks equal). Rows that are not looped over are exactly 0."""
    g, o = inputs_of(case), load_golden("ordered_" + case)
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


@pytest.mark.parametrize("case", MASKED_CASES)
def test_masked_fixtures_hold_a_visible_masked_neighbour_of_an_unmasked_row(case):
    """What the three masked fixtures are for: in each, some unmasked row lists a masked residue on the reference's own graph, and
    that row's cond (the masked residue decoded earlier: its sequence term and zero decoder state enter) differs from its uncond
    (its encoder state enters). The reference masks by the row, not by the neighbour (mask_bw = mask_1D * mask_attend)."""
    g, o = inputs_of(case), load_golden("ordered_" + case)
    L = len(g["S"])
    ei = o["E_idx"].astype(np.int64)
    assert ei.shape == (L, min(48, L)) and ei.min() >= 0 and ei.max() < L
    assert o["cond"].shape == o["uncond"].shape == o["cond_backbone_only"].shape == (L, 21)
    dead = g["mask"] == 0
    rows = [i for i in np.nonzero(~dead)[0] if dead[ei[i]].any()]
    assert rows, "no unmasked row lists a masked residue"
    moved = np.abs(o["cond"][rows] - o["uncond"][rows]).max(1)
    assert (moved > 0).all() and moved.max() > 1e-2, moved
    # under the order of row i (i last) every listed masked residue is visible: randn orders the others, never i
    i = rows[0]
    rank = conditional_ranks(o["randn"], int(i), L)
    assert (rank[ei[i][dead[ei[i]]]] < rank[i]).all()


def test_restatement_ddg_is_the_head_on_the_restated_states_also_on_30_columns():
    """ddg of the restatement: relative to the variant's own residue, the oracle's head_table on the restated states (recomputed
    here from the returned hidden), float64 within the 1e-4 line of fp32, and a 30-column graph is accepted. The recomputation
    makes the same head_table call in the same argument order as the restatement, so it cannot tell a wrong order of the hidden
    list; that is held by the GPU comparisons of ddg against kernels that are themselves pinned to the reference's ddG fixtures."""
    from oracle import thermompnn_oracle as orc
    g = inputs_of("msk_L40")
    W = weights_for_case(g)
    L = len(g["S"])
    rng = np.random.default_rng(2)
    S = np.stack([g["S"].astype(np.int64), rng.integers(0, 21, L)])
    ranks = np.stack([rng.permutation(L), np.zeros(L, np.int64)])
    for ei in (g["E_idx"], np.ascontiguousarray(g["E_idx"][:, :30])):
        r32, r64 = ordered_decode(W, g, S, ranks, ei), ordered_decode(W, g, S, ranks, ei, f64=True)
        assert r32["ddg"].shape == (2, L, 21) and r32["ddg"].dtype == np.float32 and r64["ddg"].dtype == np.float64
        assert (r32["ddg"][np.arange(2)[:, None], np.arange(L), S] == 0).all()
        hd = orc.split_weights(W)[1]
        for v in range(2):
            h = [torch.from_numpy(r32["hidden"][v, l])[None] for l in (2, 1, 0)]
            h_S = torch.nn.functional.embedding(torch.from_numpy(S[v])[None], W["prot_mpnn.W_s.weight"])
            assert np.array_equal(orc.head_table(hd, h, h_S, torch.from_numpy(S[v])[None])[1][0].numpy(), r32["ddg"][v])
        for k in ("ddg", "hidden", "log_probs"):
            assert np.abs(r32[k] - r64[k]).max() < (1e-4 if k == "ddg" else TOL_INTERMEDIATE), k
    assert np.abs(r32["ddg"][0] - r32["ddg"][1]).max() > 1e-2


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
