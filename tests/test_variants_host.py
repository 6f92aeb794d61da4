"""Host side of the variant decoder (no GPU): argument validation of tmpnn_encode / tmpnn_decode_variants, their size
functions, variant-spec parsing and the index arithmetic of double_mutant_table."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

T_MAX = (1 << 31) // (48 * 4) - 1      # the kernels' 32-bit row arithmetic (csrc/tmpnn_api.hip)
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -4, -2


@pytest.fixture(scope="module")
def lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


def err(lib):
    return lib.tmpnn_last_error().decode()


def test_error_codes_match_the_header():
    import re
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "tmpnn.h")).read()
    for name, val in (("TMPNN_E_INVALID", E_INVALID), ("TMPNN_E_WORKSPACE", E_WORKSPACE), ("TMPNN_E_UNSUPPORTED", E_UNSUPPORTED)):
        assert int(re.search(name + r"\s*=\s*(-?\d+)", text).group(1)) == val


def test_size_functions_are_monotone_and_bounded(lib):
    enc = [lib.tmpnn_encode_bytes(t) for t in (0, 1, 47, 48, 256, 4096)]
    assert enc == sorted(enc) and enc[0] == 0 and enc[4] >= 256 * (48 * 4 + 48 * 128 * 4 + 128 * 4 + 256 * 4)
    ws = [lib.tmpnn_encode_workspace_bytes(t) for t in (0, 1, 48, 256, 4096)]
    assert ws == sorted(ws) and ws[3] >= lib.tmpnn_layer_workspace_bytes(256)
    assert lib.tmpnn_encode_bytes(-1) == 0 and lib.tmpnn_encode_workspace_bytes(-1) == 0
    dec = lib.tmpnn_decode_variants_workspace_bytes
    assert [dec(256, v) for v in (0, 1, 2, 37, 64)] == sorted(dec(256, v) for v in (0, 1, 2, 37, 64))
    assert [dec(t, 8) for t in (1, 32, 256, 1024)] == sorted(dec(t, 8) for t in (1, 32, 256, 1024))
    assert dec(256, 8) >= 256 * 8 * (256 + 5 * 128 + 2) * 4
    assert dec(-1, 1) == 0 and dec(1, -1) == 0
    assert dec(256, T_MAX // 256) > 0 and dec(256, T_MAX // 256 + 1) == 0      # V * T over the limit: no size


def test_encode_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p
    w, buf = p(256), p(256)          # never dereferenced: validation comes first
    args = lambda **k: [k.get("w", w), k.get("X", buf), buf, buf, buf, buf, k.get("N", 1), k.get("T", 32), k.get("max_len", 32),
                        k.get("K", 48), k.get("ctx", buf), k.get("ctx_bytes", 1 << 30), None, k.get("ws", buf), k.get("ws_bytes", 1 << 30),
                        None]
    assert lib.tmpnn_encode(*args(w=None)) == E_INVALID and "null" in err(lib)
    assert lib.tmpnn_encode(*args(X=None)) == E_INVALID and "null" in err(lib)
    assert lib.tmpnn_encode(*args(T=-1)) == E_INVALID
    assert lib.tmpnn_encode(*args(K=49)) == E_INVALID and "K=49" in err(lib)
    assert lib.tmpnn_encode(*args(max_len=0)) == E_INVALID
    assert lib.tmpnn_encode(*args(max_len=9000)) == E_UNSUPPORTED
    assert lib.tmpnn_encode(*args(ctx=None)) == E_INVALID and "ctx" in err(lib)
    assert lib.tmpnn_encode(*args(ctx=p(260))) == E_INVALID and "aligned" in err(lib)
    assert lib.tmpnn_encode(*args(ctx_bytes=lib.tmpnn_encode_bytes(32) - 1)) == E_WORKSPACE and "ctx" in err(lib)
    assert lib.tmpnn_encode(*args(ws=None)) == E_WORKSPACE
    assert lib.tmpnn_encode(*args(ws_bytes=lib.tmpnn_encode_workspace_bytes(32) - 512)) == E_WORKSPACE and "workspace" in err(lib)
    assert lib.tmpnn_encode(*args(T=0, X=None, ctx=None, ws=None)) == 0          # an empty batch is a no-op
    assert lib.tmpnn_encode(*args(N=0, X=None, ctx=None, ws=None)) == 0


def test_decode_variants_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p
    w, buf = p(256), p(256)
    T, V = 32, 3
    need = lib.tmpnn_decode_variants_workspace_bytes(T, V)
    # ddg = None throughout (the fake handle is never dereferenced): log_probs is the requested output
    args = lambda **k: [k.get("w", w), k.get("ctx", buf), k.get("ctx_bytes", 1 << 30), k.get("S", buf), k.get("V", V), k.get("mask", buf),
                        k.get("T", T), None, k.get("hidden", None), k.get("lp", buf), None, k.get("ws", buf), k.get("ws_bytes", need),
                        None]
    f = lib.tmpnn_decode_variants
    assert f(*args(w=None)) == E_INVALID and "null" in err(lib)
    assert f(*args(S=None)) == E_INVALID and "null" in err(lib)
    assert f(*args(mask=None)) == E_INVALID
    assert f(*args(V=-1)) == E_INVALID and "V=-1" in err(lib)
    assert f(*args(T=-1)) == E_INVALID
    assert f(*args(lp=None)) == E_INVALID and "no output" in err(lib)
    assert f(*args(ctx=None)) == E_INVALID and "ctx" in err(lib)
    assert f(*args(ctx_bytes=lib.tmpnn_encode_bytes(T) - 1)) == E_WORKSPACE and "ctx" in err(lib)
    assert f(*args(ws=None)) == E_WORKSPACE
    assert f(*args(ws_bytes=need - 1)) == E_WORKSPACE and "workspace" in err(lib)
    assert f(*args(ws_bytes=lib.tmpnn_decode_variants_workspace_bytes(T, V - 1))) == E_WORKSPACE
    assert f(*args(V=T_MAX // T + 1, ws_bytes=1 << 62)) == E_UNSUPPORTED and "chunks" in err(lib)
    assert f(*args(V=0, S=None, ctx=None, ws=None, lp=None)) == 0                # nothing to decode: a no-op
    assert f(*args(T=0, S=None, ctx=None, ws=None, lp=None)) == 0


def test_variant_specs_become_the_sequence_matrix():
    from thermompnn_amd.datasets import ALPHABET, Mutation
    from thermompnn_amd.variant_scan import parse_variant_line, sequence_indices, variant_matrix
    seq = "MK-LV"
    base = sequence_indices(seq)
    assert base.tolist() == [ALPHABET.index("M"), ALPHABET.index("K"), 20, ALPHABET.index("L"), ALPHABET.index("V")]
    S = variant_matrix(seq, [seq, "AK-LW", [Mutation(0, "M", "G")], [Mutation(3, "L", "A"), Mutation(4, "", "Y")], []])
    assert S.shape == (5, 5) and S.dtype == np.int64
    assert (S[0] == base).all() and (S[4] == base).all()
    assert S[1].tolist() == [0, base[1], 20, base[3], ALPHABET.index("W")]
    assert S[2].tolist() == [ALPHABET.index("G")] + base[1:].tolist()
    assert S[3].tolist() == base[:3].tolist() + [0, ALPHABET.index("Y")]
    for bad in (["MKLV"], ["MKALV"], ["MK-LZ"], [[Mutation(5, "V", "A")]], [[Mutation(-1, "M", "A")]], [[Mutation(0, "K", "A")]],
                [[Mutation(2, "-", "A")]], [[Mutation(2, "", "A")]], [[Mutation(0, "M", "Z")]], ["M-KLV"]):
        with pytest.raises(ValueError):
            variant_matrix(seq, bad)
    muts = parse_variant_line("M1G, l4a\n")
    assert [(m.position, m.wildtype, m.mutation) for m in muts] == [(0, "M", "G"), (3, "L", "A")]
    assert parse_variant_line("AK-LW\n") == "AK-LW"
    assert (variant_matrix(seq, [muts])[0] == variant_matrix(seq, ["GK-AV"])[0]).all()


def test_variant_specs_on_the_gapped_structure():
    """2OCJ_A_gap's parsed sequence carries '-' positions (token 20, mask 0)."""
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.variant_scan import sequence_indices, variant_matrix
    seq = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"), "A")[0]["seq"]
    gaps = [k for k, c in enumerate(seq) if c == "-"]
    assert gaps
    with np.load(os.path.join(GOLDEN, "2OCJ_A_gap.npz")) as z:
        assert (sequence_indices(seq) == z["S"]).all()
    live = next(k for k, c in enumerate(seq) if c != "-")
    S = variant_matrix(seq, [[Mutation(live, seq[live], "W")], seq])
    assert S[0, live] == 18 and (S[0, gaps] == 20).all() and (S[1] == sequence_indices(seq)).all()
    with pytest.raises(ValueError, match="'-'"):
        variant_matrix(seq, [[Mutation(gaps[0], "-", "A")]])
    with pytest.raises(ValueError):
        variant_matrix(seq, [seq[:gaps[0]] + "A" + seq[gaps[0] + 1:]])
    with pytest.raises(ValueError):
        variant_matrix(seq, [seq + "A"])


def test_double_mutant_table_index_arithmetic():
    """Against a numpy restatement, with a stub table function whose entries name their own (sequence, position, residue)."""
    import torch
    from thermompnn_amd.variant_scan import double_mutant_table, sequence_indices
    seq = "MK-LVA"
    L, base = len(seq), sequence_indices(seq)
    calls = []

    def stub(S):
        S = np.asarray(S)
        calls.append(len(S))
        w = (S * (np.arange(L) + 3)).sum(1).astype(np.float64)                   # a number that knows the whole background
        t = w[:, None, None] * 1e-3 + np.arange(L)[None, :, None] * 0.5 + np.arange(21)[None, None, :] * 0.01
        return torch.from_numpy(t)

    got = double_mutant_table(None, [{"seq": seq}], chunk=7, _tables=stub).numpy()
    positions = [0, 1, 3, 4, 5]
    assert got.shape == (5, 20, L, 20) and max(calls) <= 7
    wt = stub(base[None])[0].numpy()
    for k, p in enumerate(positions):
        for a in range(20):
            bg = base.copy()
            bg[p] = a
            want = wt[p, a] + stub(bg[None])[0].numpy()[:, :20]
            np.testing.assert_array_equal(got[k, a], want)
    sub = double_mutant_table(None, [{"seq": seq}], positions=[4, 1], _tables=stub).numpy()
    np.testing.assert_array_equal(sub[0], got[3])
    np.testing.assert_array_equal(sub[1], got[1])
    with pytest.raises(ValueError):
        double_mutant_table(None, [{"seq": seq}], positions=[2], _tables=stub)
