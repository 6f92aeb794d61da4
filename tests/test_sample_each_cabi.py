"""C-ABI of per-protein sampling without a GPU: the four tmpnn_sample_each entries are exported and bound, their workspace is sized
by the protein range (monotone, 0 beyond the bound of the kernel's row arithmetic), the whole-axis entries' sizes are what they
were, and every argument error — null pointers, a bad protein or row range, negative sizes, inv_temperature, a short ctx or
workspace, the chunk bound, an fp32 handle — comes back as a code and a message before any launch."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN

E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
T_MAX = (1 << 31) // (48 * 4) - 1
ROWS_MAX = (1 << 24) - 1          # 3 * N * rows table rows


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
    assert len(_lib.SIGNATURES["tmpnn_sample_each"][1]) == 26 and len(_lib.SIGNATURES["tmpnn_sample_tied_each"][1]) == 31
    for name in ("tmpnn_sample_each_workspace_bytes", "tmpnn_sample_tied_each_workspace_bytes"):
        assert len(_lib.SIGNATURES[name][1]) == 2 and getattr(lib, name).restype is C.c_size_t
    assert lib.tmpnn_sample_each.argtypes is not None and lib.tmpnn_sample_tied_each.argtypes is not None
    # the whole-axis entries are untouched
    assert len(_lib.SIGNATURES["tmpnn_sample"][1]) == 19 and len(_lib.SIGNATURES["tmpnn_sample_tied"][1]) == 24
    assert lib.tmpnn_version() == 200


@pytest.mark.parametrize("name", ["tmpnn_sample_each_workspace_bytes", "tmpnn_sample_tied_each_workspace_bytes"])
def test_workspace_is_sized_by_the_range(lib, name):
    size = getattr(lib, name)
    ns = (0, 1, 2, 16, 17, 33, 64, 256)
    assert [size(256, n) for n in ns] == sorted(size(256, n) for n in ns) and size(256, 1) > size(256, 0) > 0
    rows = (0, 1, 32, 194, 256, 1024)
    assert [size(r, 8) for r in rows] == sorted(size(r, 8) for r in rows) and size(1024, 8) > size(256, 8)
    # the table [N,3,rows,128], the rank array [N,rows] and two [rows,256] projections of the encoder state
    assert size(256, 8) >= 8 * 3 * 256 * 128 * 4 + 8 * 256 * 4 + 2 * 256 * 256 * 4
    assert size(-1, 1) == 0 and size(1, -1) == 0 and size(T_MAX + 1, 1) == 0
    assert size(ROWS_MAX // 3, 1) > 0 and size(ROWS_MAX // 3 + 1, 1) == 0
    assert size(256, ROWS_MAX // 3 // 256) > 0 and size(256, ROWS_MAX // 3 // 256 + 1) == 0


def test_whole_axis_workspace_sizes_are_what_they_were(lib):
    golden = json.load(open(os.path.join(GOLDEN, "workspace_sizes.json")))
    rows = golden["tmpnn_sample_workspace_bytes"]
    assert len(rows) > 50
    for args, want in rows:
        assert lib.tmpnn_sample_workspace_bytes(*args) == want, args
        assert lib.tmpnn_sample_tied_workspace_bytes(*args) == want, args
    # one layout for all four entries: the range's rows where the whole-axis entries have T
    for T, N in ((32, 1), (145, 17), (1024, 64)):
        assert lib.tmpnn_sample_each_workspace_bytes(T, N) == lib.tmpnn_sample_workspace_bytes(T, N)
        assert lib.tmpnn_sample_tied_each_workspace_bytes(T, N) == lib.tmpnn_sample_tied_workspace_bytes(T, N)


@pytest.mark.parametrize("tied", [False, True])
def test_each_rejects_bad_arguments_before_any_launch(lib, tied):
    p = C.c_void_p
    buf = p(256)                     # never dereferenced: validation comes first
    wp = C.cast(fake_handle(2), p)
    T, P, N, rows = 145, 4, 3, 57
    size = lib.tmpnn_sample_tied_each_workspace_bytes if tied else lib.tmpnn_sample_each_workspace_bytes
    need = size(rows, N)

    def args(**k):
        g = lambda name, default: k.get(name, default)
        head = [g("w", wp), g("ctx", buf), g("ctx_bytes", 1 << 30), g("mask", buf), g("T", T), g("offsets", buf), g("P", P), g("p0", 1),
                g("p1", 3), g("row0", 32), g("rows", rows), g("sched", None), g("N", N), g("order", buf)]
        mid = [g("S_fixed", buf), g("free", buf), g("u", buf), g("inv_t", 1.0)]
        if tied:
            mid = [g("close", buf)] + mid + [None, None, None, g("mix", None), g("pbias", None), None]
        else:
            mid = mid + [None, None]
        return head + mid + [g("S_out", buf), None, None, g("ws", buf), g("ws_bytes", need), None]

    f = lib.tmpnn_sample_tied_each if tied else lib.tmpnn_sample_each
    err = lambda: lib.tmpnn_last_error().decode()
    assert f(*args(w=None)) == E_INVALID and "null" in err()
    for name in ("mask", "offsets", "order", "S_fixed", "free", "u", "S_out") + (("close",) if tied else ()):
        assert f(*args(**{name: None})) == E_INVALID and "null" in err(), name
    assert f(*args(p0=3, p1=2)) == E_INVALID and "p0=3" in err()                     # p0 > p1
    assert f(*args(p1=P + 1)) == E_INVALID and "protein range" in err()              # p1 > P
    assert f(*args(p0=-1)) == E_INVALID
    assert f(*args(rows=-1)) == E_INVALID and "rows=-1" in err()
    assert f(*args(N=-1)) == E_INVALID and "N=-1" in err()
    assert f(*args(T=-1)) == E_INVALID
    assert f(*args(row0=-1)) == E_INVALID and f(*args(row0=T - rows + 1)) == E_INVALID and "row range" in err()
    assert f(*args(inv_t=0.0)) == E_INVALID and "inv_temperature" in err()
    for bad in (-1.0, float("inf"), float("nan")):
        assert f(*args(inv_t=bad)) == E_INVALID
    if tied:
        assert f(*args(pbias=buf)) == E_INVALID and "pssm_bias" in err()
        assert f(*args(mix=buf)) == E_INVALID and "pssm_bias" in err()
    assert f(*args(ctx=None)) == E_INVALID and "ctx" in err()
    assert f(*args(ctx_bytes=lib.tmpnn_encode_bytes(T) - 1)) == E_WORKSPACE and "ctx" in err()
    assert f(*args(ws=None)) == E_WORKSPACE
    assert f(*args(ws_bytes=need - 1)) == E_WORKSPACE and "workspace" in err()
    assert str(need - 1) in err() and str(need) in err()                             # both numbers in the message
    assert f(*args(N=ROWS_MAX // 3 // rows + 1, ws_bytes=1 << 62)) == E_UNSUPPORTED and "chunks" in err()
    assert f(*args(w=C.cast(fake_handle(0), p))) == E_UNSUPPORTED and "bf16x3" in err()        # an fp32 handle: the documented refusal
    none = dict(mask=None, offsets=None, order=None, close=None, S_fixed=None, free=None, u=None, S_out=None, ctx=None, ws=None)
    assert f(*args(N=0, **none)) == 0                                                          # nothing to sample: a no-op
    assert f(*args(rows=0, **none)) == 0
    assert f(*args(p0=2, p1=2, **none)) == 0
