"""C-ABI of tied sampling without a GPU: tmpnn_sample_tied validates its arguments before any launch (null pointers, sizes,
inv_temperature, pssm_bias without pssm_mix, a short ctx / workspace, the chunk bound, an fp32 handle), T == 0 or N == 0 is a
no-op, and tmpnn_sample_tied_workspace_bytes is monotone and 0 beyond the bound of the kernel's row arithmetic."""
import ctypes as C

import pytest

E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
T_MAX = (1 << 31) // (48 * 4) - 1
ROWS_MAX = (1 << 24) - 1          # 3 * N * T table rows


@pytest.fixture(scope="module")
def lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


def fake_handle(mode):
    """A zeroed block with the handle's second int (the precision: 0 = fp32, 1 = bf16x3, 2 = f16x2) set; nothing else of it is read
    before the launches, which these tests never reach."""
    buf = (C.c_int32 * 16384)()
    buf[1] = mode
    return buf


def test_symbols_are_exported_and_bound(lib):
    from thermompnn_amd import _lib
    assert len(_lib.SIGNATURES["tmpnn_sample_tied"][1]) == 24 and len(_lib.SIGNATURES["tmpnn_sample_tied_workspace_bytes"][1]) == 2
    assert lib.tmpnn_sample_tied.argtypes is not None and lib.tmpnn_sample_tied_workspace_bytes.restype is C.c_size_t
    assert len(_lib.SIGNATURES["tmpnn_sample"][1]) == 19 and lib.tmpnn_version() == 200         # the untied entry is untouched


def test_workspace_size(lib):
    size = lib.tmpnn_sample_tied_workspace_bytes
    ns = (0, 1, 2, 16, 17, 33, 64, 256)
    assert [size(256, n) for n in ns] == sorted(size(256, n) for n in ns) and size(256, 1) > size(256, 0) > 0
    ts = (0, 1, 32, 194, 256, 1024)
    assert [size(t, 8) for t in ts] == sorted(size(t, 8) for t in ts)
    # the table [N,3,T,128], the rank array [N,T] and two [T,256] projections of the encoder state
    assert size(256, 8) >= 8 * 3 * 256 * 128 * 4 + 8 * 256 * 4 + 2 * 256 * 256 * 4
    assert size(-1, 1) == 0 and size(1, -1) == 0 and size(T_MAX + 1, 1) == 0
    assert size(ROWS_MAX // 3, 1) > 0 and size(ROWS_MAX // 3 + 1, 1) == 0
    assert size(256, ROWS_MAX // 3 // 256) > 0 and size(256, ROWS_MAX // 3 // 256 + 1) == 0


def test_sample_tied_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p
    buf = p(256)                     # never dereferenced: validation comes first
    wp = C.cast(fake_handle(2), p)
    T, N = 32, 3
    need = lib.tmpnn_sample_tied_workspace_bytes(T, N)
    args = lambda **k: [k.get("w", wp), k.get("ctx", buf), k.get("ctx_bytes", 1 << 30), k.get("mask", buf), k.get("T", T), k.get("N", N),
                        k.get("order", buf), k.get("close", buf), k.get("S_fixed", buf), k.get("free", buf), k.get("u", buf),
                        k.get("inv_t", 1.0), None, None, None, k.get("mix", None), k.get("pbias", None), None,
                        k.get("S_out", buf), None, None, k.get("ws", buf), k.get("ws_bytes", need), None]
    f = lib.tmpnn_sample_tied
    err = lambda: lib.tmpnn_last_error().decode()
    assert f(*args(w=None)) == E_INVALID and "null" in err()
    for name in ("mask", "order", "close", "S_fixed", "free", "u", "S_out"):
        assert f(*args(**{name: None})) == E_INVALID and "null" in err(), name
    assert f(*args(N=-1)) == E_INVALID and "N=-1" in err()
    assert f(*args(T=-1)) == E_INVALID
    assert f(*args(inv_t=0.0)) == E_INVALID and "inv_temperature" in err()
    for bad in (-1.0, float("inf"), float("nan")):
        assert f(*args(inv_t=bad)) == E_INVALID
    assert f(*args(pbias=buf)) == E_INVALID and "pssm_bias" in err()                 # pssm_bias without pssm_mix
    assert f(*args(mix=buf)) == E_INVALID and "pssm_bias" in err()                   # ... and pssm_mix without pssm_bias
    assert f(*args(ctx=None)) == E_INVALID and "ctx" in err()
    assert f(*args(ctx_bytes=lib.tmpnn_encode_bytes(T) - 1)) == E_WORKSPACE and "ctx" in err()
    assert f(*args(ws=None)) == E_WORKSPACE
    assert f(*args(ws_bytes=need - 1)) == E_WORKSPACE and "workspace" in err()
    assert str(need - 1) in err() and str(need) in err()                             # both numbers in the message
    assert f(*args(N=ROWS_MAX // 3 // T + 1, ws_bytes=1 << 62)) == E_UNSUPPORTED and "chunks" in err()
    assert f(*args(w=C.cast(fake_handle(0), p))) == E_UNSUPPORTED and "bf16x3" in err()        # an fp32 handle: the documented refusal
    assert f(*args(w=C.cast(fake_handle(0), p), mix=buf, pbias=buf)) == E_UNSUPPORTED          # (both PSSM tables pass the pairing check)
    none = dict(mask=None, order=None, close=None, S_fixed=None, free=None, u=None, S_out=None, ctx=None, ws=None)
    assert f(*args(N=0, **none)) == 0                                                          # nothing to sample: a no-op
    assert f(*args(T=0, **none)) == 0
