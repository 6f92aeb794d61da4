"""Conformer ensembles, the parts that need no GPU: the numpy restatement of tmpnn_ensemble_stats against a scalar brute-force loop
and against float64, the conditions that keep the device tests from passing while they test nothing (the order of the members and the
separate rounding of the multiply DO decide bits on these inputs; the tie draw holds every special bit pattern), the multi-MODEL
parser, ``align_members``, and the argument errors of the C entry (before any launch)."""
import ctypes as C

import numpy as np
import pytest

from ensemble_inputs import SHAPES, crafted, single, write_models
from ensemble_restatement import (ARRAYS, CANON, FLOATS, MAX_E, MAX_LEN, assert_ensemble_equal, ensemble_brute, ensemble_reference,
                                  filled, is_nan_bits)


def _ref(c, **kw):
    return ensemble_reference(c["ddg"], c["S"], c["desc"], c["T_out"], c["max_len"], **kw)


@pytest.mark.parametrize("draw", ["tie", "rounding"])
def test_restatement_equals_a_scalar_loop(draw):
    c = crafted(draw)
    for cutoff in (None, -0.5, 1.0):
        got = _ref(c, cutoff=cutoff)
        assert (got["status"] == 0).all()
        for (row0, M, L, out0) in c["desc"].tolist():
            want = ensemble_brute(c["ddg"], c["S"], row0, M, L, cutoff)
            assert_ensemble_equal(got, want, rows=slice(out0, out0 + L))
    assert not (got["mean"].view(np.uint32) == 0xdeadbeef).any()          # good ensembles tile the outputs: no sentinel is left


def test_restatement_is_close_to_float64_on_the_rounding_draw():
    """mean within 2^-23 sum|x| and spread within 2^-23 (sum|x| + (n + 4) sigma64) of float64: the first-order bounds of n
    sequential adds (each within 2^-24 of a partial sum <= sum|x|) plus the shift of the centre, doubled."""
    c = crafted("rounding")
    got = _ref(c)
    u = 2.0 ** -23
    seen = 0
    for (row0, M, L, out0) in c["desc"].tolist():
        b = ensemble_brute(c["ddg"], c["S"], row0, M, L)
        live = b["count"] > 0
        mean, spread = got["mean"][out0:out0 + L][live].astype(np.float64), got["spread"][out0:out0 + L][live].astype(np.float64)
        n = b["count"][live]
        assert (np.abs(mean - b["mean64"][live]) <= u * b["sum_abs"][live]).all()
        assert (np.abs(spread - b["spread64"][live]) <= u * (b["sum_abs"][live] + (n + 4) * b["spread64"][live])).all()
        one = b["count"] == 1
        assert (got["spread"][out0:out0 + L][one] == 0).all()             # the population form: 0 for one member
        seen += int(live.sum())
    assert seen > 2000


@pytest.mark.parametrize("M", [3, 17])
def test_order_and_contraction_decide_bits_on_the_rounding_draw(M):
    """Conditions on the reference alone (seed 7, L = 19: 380 entries): summing the members in another order moves the bits of
    some means, and a fused multiply-add moves the bits of some spreads — so an exact device comparison on this draw does test both.
    Counted with these inputs: 89 / 380 (M = 3) and 246 / 380 (M = 17) means move under the permutation, 49 and 63 spreads under
    the fused form; the test asks for 20 of each."""
    c = single("rounding", M, 19, 7)
    base = _ref(c)
    assert (base["count"] == M).all()
    perm = np.random.default_rng(7).permutation(M)
    while (perm == np.arange(M)).all():
        perm = np.roll(perm, 1)
    moved = _ref(c, order=perm)
    for name in ("lo", "hi", "count", "below"):                           # what does not depend on the order stays
        np.testing.assert_array_equal(base[name].view(np.uint32), moved[name].view(np.uint32))
    n_mean = int((base["mean"].view(np.uint32) != moved["mean"].view(np.uint32)).sum())
    fused = _ref(c, fma=True)
    np.testing.assert_array_equal(base["mean"].view(np.uint32), fused["mean"].view(np.uint32))
    n_spread = int((base["spread"].view(np.uint32) != fused["spread"].view(np.uint32)).sum())
    print(f"M={M}: {n_mean} / 380 means move under permutation, {n_spread} / 380 spreads under fma")
    assert n_mean >= 20 and n_spread >= 20


def test_tie_draw_holds_every_special_case():
    c = crafted("tie")
    bits = set(c["ddg"].view(np.uint32).ravel().tolist())
    assert {0x80000000, 0, 0x7f800000, 0xff800000, 0x3f800000, 0x3f800001} <= bits and any(0 < x < 0x00800000 for x in bits)
    assert any(is_nan_bits(np.uint32(x)) for x in bits)
    assert c["S"].min() == -2 and c["S"].max() == 21
    r = _ref(c)
    u = lambda name: r[name].view(np.uint32)
    for e in (2, 3):
        _, M, L, out0 = c["desc"][e].tolist()
        at = lambda q: out0 + q
        assert (r["count"][at(4)] == 0).all() and (u("mean")[at(4)] == CANON).all() and (r["lo_member"][at(4)] == -1).all()
        assert (u("lo")[at(4)] == CANON).all() and (u("spread")[at(4)] == CANON).all() and (r["below"][at(4)] == 0).all()
        assert r["count"][at(5), 3] == 0 and u("hi")[at(5), 3] == CANON and r["hi_member"][at(5), 3] == -1     # NaN only, members in
        assert r["count"][at(5), 4] > 0
        assert r["count"][at(6), 7] == M and u("mean")[at(6), 7] == CANON and u("spread")[at(6), 7] == CANON   # +inf + -inf
        assert (u("lo")[at(6), 7], u("hi")[at(6), 7]) == (0xff800000, 0x7f800000)
        assert (r["lo_member"][at(6), 7], r["hi_member"][at(6), 7]) == (1, 0)
        assert (u("lo")[at(7), 2], r["lo_member"][at(7), 2]) == (0x80000000, 1)      # -0.0 tied with +0.0: the first, its own bits
        assert (u("hi")[at(8), 2], r["hi_member"][at(8), 2]) == (0x00000000, 1)
        assert (u("lo")[at(9), 2], r["lo_member"][at(9), 2]) == (0x80000000, 0)
    _, _, L, out0 = c["desc"][4].tolist()                                 # M = 0: output rows of padding
    assert (r["count"][out0:out0 + L] == 0).all() and (u("mean")[out0:out0 + L] == CANON).all() and r["status"][4] == 0
    assert np.isinf(r["mean"]).any() and (r["spread"][~np.isnan(r["spread"])] >= 0).all()
    # a cutoff counts with a float compare: -0.0 <= +0.0, and +inf counts every participant
    assert (r["below"] == r["count"]).all()
    zero = _ref(c, cutoff=0.0)
    e, q = 2, 7
    assert zero["below"][c["desc"][e][3] + q, 2] == 2


def test_bad_descriptors_leave_their_rows_alone_in_the_restatement():
    c = crafted("rounding")
    good = _ref(c)
    desc = c["desc"].copy()
    desc[1, 1] += 1000                                                    # row0 + M L > T
    desc[3, 2] = 71                                                       # L > max_len
    out = filled(c["T_out"], 0x12345678)
    r = ensemble_reference(c["ddg"], c["S"], desc, c["T_out"], c["max_len"], out=out)
    assert r["status"].tolist() == [0, -1, 0, -1, 0]
    for e, (row0, M, L, out0) in enumerate(c["desc"].tolist()):
        rows = slice(out0, out0 + L)
        if r["status"][e] == 0:
            assert_ensemble_equal(r, good, rows=rows, want_rows=rows)
        else:
            assert all((r[name][rows].view(np.uint32) == 0x12345678).all() for name in ARRAYS)


# ---- the parser and the alignment ---------------------------------------------------------------------------------------------------
def test_parse_pdb_models_reads_every_model(tmp_path):
    from thermompnn_amd.pdb_io import alt_parse_PDB, parse_pdb_models
    from thermompnn_amd.synthetic import backbone_pdb_text
    path = str(tmp_path / "ens.pdb")
    X, seq = write_models(path, drop=(1, 7))
    models = parse_pdb_models(path, "A")
    assert [m["name"] for m in models] == ["ens_m1", "ens_m2", "ens_m3"]
    for k, m in enumerate(models):
        assert m["seq"] == seq and m["num_of_chains"] == 1 and m["seq_chain_A"] == seq
        for i, a in enumerate(("N", "CA", "C", "O")):
            got = np.array(m["coords_chain_A"][f"{a}_chain_A"])
            want = X[k, :, i].copy()
            if k == 1 and a == "N":
                assert np.isnan(got[7]).all()
                want[7] = got[7]
            np.testing.assert_array_equal(got, want)
    first = alt_parse_PDB(path, "A")                                      # unchanged: the first occurrence of every atom, model 1
    assert first[0]["coords_chain_A"] == models[0]["coords_chain_A"] and first[0]["name"] == "ens"
    assert sorted(first[0]) == sorted(models[0])
    ca = parse_pdb_models(path, "A", ca_only=True)
    np.testing.assert_array_equal(np.array(ca[2]["coords_chain_A"]["CA_chain_A"]), X[2, :, 1:2])    # [L, 1, 3]
    # a file without MODEL records: exactly alt_parse_PDB, key for key
    plain = str(tmp_path / "one.pdb")
    with open(plain, "w") as fh:
        fh.write(backbone_pdb_text(X[0], seq))
    a, b = parse_pdb_models(plain, "A"), alt_parse_PDB(plain, "A")
    assert len(a) == 1 and list(a[0]) == list(b[0]) and all(a[0][k] == b[0][k] for k in b[0])


def test_align_members_names_the_member_and_the_position(tmp_path):
    from thermompnn_amd.ensemble import align_members
    from thermompnn_amd.pdb_io import parse_pdb_models
    from thermompnn_amd.synthetic import synthetic_pdb_dict
    path = str(tmp_path / "ens.pdb")
    _, seq = write_models(path, drop=(1, 7))
    models = parse_pdb_models(path, "A")
    got_seq, S = align_members(models)
    assert got_seq == seq and S.shape == (3, 40) and S.dtype == np.int32
    alphabet = "ACDEFGHIKLMNPQRSTVWYX"
    want = np.array([alphabet.index(c) for c in seq])
    assert (S[0] == want).all() and (S[2] == want).all()
    assert S[1, 7] == 20 and (np.delete(S[1], 7) == np.delete(want, 7)).all()      # the missing N line: that member's row only
    gap = dict(models[2], seq=seq[:3] + "-" + seq[4:], seq_chain_A=seq[:3] + "X" + seq[4:])
    s2, S2 = align_members([gap, models[0]])
    assert s2 == seq and S2[0, 3] == 20 and S2[1, 3] == want[3]            # a member's own '-' drops out; the others name the letter
    short = synthetic_pdb_dict(39, 3, name="short")
    with pytest.raises(ValueError, match=r"member 2 \(short\) has 39 residues"):
        align_members([models[0], models[1], short])
    other = "A" if seq[11] != "A" else "G"
    wrong = dict(models[1], seq=seq[:11] + other + seq[12:], name="wrong")
    with pytest.raises(ValueError, match=rf"member 1 \(wrong\) holds {other} at position 11, member 0 holds {seq[11]}"):
        align_members([models[0], wrong])
    with pytest.raises(ValueError, match="at least one member"):
        align_members([])


# ---- the C entry before any launch -------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(256)                                                   # never dereferenced: every call below fails before a launch
    outs = ("mean", "spread", "lo", "hi", "lo_member", "hi_member", "count", "below")

    def call(ddg=d, ld=21, S=d, desc=d, E=3, T=100, T_out=40, max_len=40, cutoff=float("inf"), status=d, **kw):
        return lib.tmpnn_ensemble_stats(ddg, ld, S, desc, E, T, T_out, max_len, cutoff, *[kw.get(name, d) for name in outs], status, None)

    for name in ("ddg", "S", "desc", "status") + outs:
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(ld=19) == -1 and b"ld=19" in lib.tmpnn_last_error()
    assert call(cutoff=float("nan")) == -1 and b"NaN" in lib.tmpnn_last_error()
    for bad in (dict(E=-1), dict(T=-1), dict(T_out=-1), dict(max_len=-1)):
        assert call(**bad) == -1 and b"sizes" in lib.tmpnn_last_error(), bad
    assert call(E=70000) == -2 and b"65535" in lib.tmpnn_last_error()    # TMPNN_E_UNSUPPORTED
    assert call(E=MAX_E + 1) == -2
    assert call(max_len=MAX_LEN + 1) == -2 and b"8192" in lib.tmpnn_last_error()
    assert call(T=1 << 31) == -2 and b"2^31" in lib.tmpnn_last_error() and call(T_out=1 << 31) == -2
    # E == 0 is a no-op, and an empty table or empty outputs have no address
    assert call(E=0) == 0 and call(E=0, desc=None, status=None) == 0 and call(E=0, T=0, ddg=None, S=None) == 0
    assert call(E=0, ld=19) == -1 and call(E=0, cutoff=float("nan")) == -1                             # the errors come first
    assert (_lib.ENS_MAX_LEN, _lib.ENS_MAX_E) == (MAX_LEN, MAX_E)
    assert [name for name, _ in _lib.ENS_ARRAYS] == list(ARRAYS)
    assert [dt for name, dt in _lib.ENS_ARRAYS] == ["float32"] * len(FLOATS) + ["int32"] * 4
    assert lib.tmpnn_version() == 200


def test_engine_method_refuses_a_cpu_table():
    import torch
    from thermompnn_amd._lib import TmpnnError
    from thermompnn_amd.engine import Engine
    with pytest.raises(TmpnnError, match="device"):
        Engine.ensemble_stats(None, torch.zeros((4, 21)), np.zeros(4, np.int32), [2], [2])
    assert SHAPES[-1][0] == 0
