"""The packed sequence loss, host side (no GPU): the C-ABI entries tmpnn_seqloss_batch_* are declared, exported and bound, their
sizers refuse what the entries refuse, every argument error comes before any launch (fake pointers, never dereferenced), and the
module's switch is off by default."""
import ctypes as C

import pytest
import torch

E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4       # include/tmpnn.h
T_MAX = 65536                                            # SB_T_MAX (csrc/tmpnn_seqbatch.hip)
NEW = ("tmpnn_seqloss_batch_saved_bytes", "tmpnn_seqloss_batch_scratch_bytes", "tmpnn_seqloss_batch_mask_numel",
       "tmpnn_seqloss_batch_forward", "tmpnn_seqloss_batch_backward")


def _lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound():
    from test_cabi import declared_symbols
    from thermompnn_amd import _lib as L
    from thermompnn_amd import build
    lib = _lib()
    names = declared_symbols()
    for n in NEW:
        assert n in names and n in L.SIGNATURES and hasattr(lib, n), n
    assert len(L.SIGNATURES["tmpnn_seqloss_batch_forward"][1]) == 25 and len(L.SIGNATURES["tmpnn_seqloss_batch_backward"][1]) == 25
    assert "tmpnn_seqbatch.hip" in build.SOURCES and "tmpnn_ft.h" in build.HEADERS
    assert lib.tmpnn_version() == 200


def test_sizers_refuse_what_the_entries_refuse_and_grow_with_the_rows():
    lib = _lib()
    for sizer in (lib.tmpnn_seqloss_batch_saved_bytes, lib.tmpnn_seqloss_batch_scratch_bytes):
        assert sizer(1, 1, 1) == 0 and sizer(0, 1, 1) == 0 and sizer(-5, 1, 1) == 0            # T < 2
        assert sizer(T_MAX + 1, 4, 48) == 0 and sizer(1 << 40, 4, 48) == 0                     # above the bound
        assert sizer(T_MAX, 4, 48) > 0
        assert sizer(96, 0, 30) == 0 and sizer(96, -1, 30) == 0                                # n_proteins < 1
        assert sizer(96, 2, 0) == 0 and sizer(96, 2, 49) == 0 and sizer(96, 2, -3) == 0        # K outside 1..48
        assert sizer(40, 1, 41) == 0 and sizer(40, 1, 40) > 0                                  # K > T
        for n, K in ((1, 2), (3, 30), (8, 48)):
            sizes = [sizer(T, n, K) for T in (96, 97, 128, 129, 500, 3000, 10000, T_MAX)]
            assert all(s > 0 and s % 256 == 0 for s in sizes)
            assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizer(128, 3, 30) < sizer(128, 3, 48)                                           # carved for the call's K
    # what the backward reads: 416 features and >= 20 [E,128] activations per edge, log_probs
    assert lib.tmpnn_seqloss_batch_saved_bytes(128, 3, 30) > 128 * 30 * (416 + 20 * 128) * 4 + 128 * 21 * 4
    # about 0.8 MB per residue at K = 48
    assert 0.7e6 < lib.tmpnn_seqloss_batch_saved_bytes(4096, 64, 48) / 4096 < 0.9e6
    for L in (2, 17, 40, 47, 48, 49, 56, 1024, 8192):
        assert lib.tmpnn_seqloss_batch_mask_numel(L, min(48, L)) == lib.tmpnn_finetune_mask_numel(L)
    assert lib.tmpnn_seqloss_batch_mask_numel(128, 30) == (12 * 128 + 3 * 128 * 30) * 128
    for T, K in ((1, 1), (T_MAX + 1, 48), (96, 0), (96, 49), (40, 41)):
        assert lib.tmpnn_seqloss_batch_mask_numel(T, K) == -1
    # the one-protein sizers are where they were (tests/golden/workspace_sizes.json pins them; here: the batch carve at n = 1 and
    # K = min(48, L) is the one-protein carve)
    for L in (17, 40, 56, 300):
        assert lib.tmpnn_seqloss_batch_saved_bytes(L, 1, min(48, L)) == lib.tmpnn_seqloss_saved_bytes(L)
        assert lib.tmpnn_seqloss_batch_scratch_bytes(L, 1, min(48, L)) == lib.tmpnn_seqloss_scratch_bytes(L)


def test_argument_errors_come_before_any_launch():
    lib = _lib()
    numel = lib.tmpnn_seqloss_slab_numel()
    p = C.c_void_p(256)                            # never dereferenced: every call below is refused first
    base = dict(n=3, T=128, lo=32, hi=56, k=30)

    def sizes(a):
        K = min(a["k"], a["lo"])
        return lib.tmpnn_seqloss_batch_saved_bytes(a["T"], a["n"], K), lib.tmpnn_seqloss_batch_scratch_bytes(a["T"], a["n"], K)

    def fwd(X=p, offsets=p, numel=numel, p_mpnn=0.1, keep_in=None, keep_out=None, lp=p, saved=p, short=0, **kw):
        a = dict(base, **kw)
        sv, _ = sizes(a)
        return lib.tmpnn_seqloss_batch_forward(X, p, p, p, p, offsets, a["n"], a["T"], a["lo"], a["hi"], a["k"], None, p, numel, p_mpnn, keep_in,
                                               keep_out, 0, 0, lp, None, None, saved, sv - short, None)

    def bwd(S=p, numel=numel, dlp=p, grads=p, saved=p, scratch=p, short=0, short_sc=0, **kw):
        a = dict(base, **kw)
        sv, sc = sizes(a)
        return lib.tmpnn_seqloss_batch_backward(p, S, p, p, p, p, a["n"], a["T"], a["lo"], a["hi"], a["k"], p, p, numel, 0.0, None, 0, 0, dlp,
                                                grads, saved, sv - short, scratch, sc - short_sc, None)
    err = lambda: lib.tmpnn_last_error()
    for call in (fwd, bwd):
        assert call(n=0) == E_INVALID and b"n_proteins" in err()
        assert call(lo=57, hi=56) == E_INVALID and b"min_len" in err()
        assert call(lo=1, hi=56) == E_INVALID and b"min_len" in err()
        assert call(lo=32, hi=8193) == E_INVALID and b"8192" in err()
        assert call(T=95) == E_INVALID and b"cannot hold" in err()                   # T < n min_len
        assert call(T=169) == E_INVALID and b"cannot hold" in err()                  # T > n max_len
        for k in (0, 49, -1):
            assert call(k=k) == E_INVALID and b"k_neighbors" in err()
        assert call(numel=numel - 21) == E_INVALID and b"slab" in err()
        # the K rule: one K = min(k_neighbors, min_len) for the call; shorter proteins than k_neighbors only in a pack of one length
        assert call(lo=40, hi=56, k=48, T=140) == E_INVALID and b"40" in err() and b"48" in err()
        assert call(short=1) == E_WORKSPACE and b"saved" in err()
        assert call(saved=None) == E_WORKSPACE and b"saved" in err()
        # ... and these pass the rule: they are refused only by the byte count that is one short
        assert call(lo=40, hi=40, k=48, T=120, short=1) == E_WORKSPACE
        assert call(lo=40, hi=56, k=30, T=140, short=1) == E_WORKSPACE
        assert call(n=1600, lo=40, hi=56, T=T_MAX + 1, k=30) == E_UNSUPPORTED and b"65536" in err()
    assert fwd(X=None) == E_INVALID and b"null pointer" in err()
    assert fwd(offsets=None) == E_INVALID and b"null pointer" in err()
    assert fwd(lp=None) == E_INVALID and b"null pointer" in err()
    assert bwd(S=None) == E_INVALID and b"null pointer" in err()
    assert bwd(dlp=None) == E_INVALID and b"null pointer" in err()
    assert bwd(grads=None) == E_INVALID and b"null pointer" in err()
    assert fwd(p_mpnn=1.0) == E_INVALID and b"dropout" in err()
    assert fwd(keep_in=p, keep_out=p) == E_INVALID and b"exclude each other" in err()
    assert bwd(short_sc=1) == E_WORKSPACE and b"scratch" in err()
    assert bwd(scratch=None) == E_WORKSPACE and b"scratch" in err()


def test_packed_is_off_by_default_and_a_cpu_module_raises_the_device_error():
    from thermompnn_amd import model_utils as mu
    assert mu.ProteinMPNN.packed is False
    model = mu.ProteinMPNN(augment_eps=0.0)
    assert model.packed is False and "packed" not in model.state_dict()
    model.packed = True
    X = torch.zeros(2, 5, 4, 3)
    one, idx = torch.ones(2, 5), torch.arange(5)[None].repeat(2, 1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(X, torch.zeros(2, 5, dtype=torch.long), one, one, idx, torch.ones(2, 5, dtype=torch.long))
    with pytest.raises(RuntimeError, match="MI355X only"):
        mu.sequence_log_probs_batch(None, list(model.parameters()), X[0], one[0], one[0], idx[0], idx[0], idx[0], [0, 5], 48, 0.0)
    assert mu.ProteinMPNN.packed is False                                           # the instance's switch, not the class's
