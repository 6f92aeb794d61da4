"""The contract of tmpnn_select_variant_hits (include/tmpnn.h) restated in numpy: every candidate of a call, the np.float32 sum, its
integer order key, np.lexsort over (key, tag, position, letter), the first k; a state is the k 64-bit keys and takes part in the next
call. Shared by tests/test_pair_hits_host.py and tests/test_gpu_pair_hits.py; every device comparison against it is exact."""
import numpy as np

CYS = 1                                  # 'C' in ACDEFGHIKLMNPQRSTVWYX
NONE = np.uint64(0xffffffffffffffff)     # the key of "no hit"
MAX_TAG, MAX_LEN = 65535, 2048


def ord32(bits):
    """The order-preserving image of IEEE-754 single bits on uint32, -0.0 taken as +0.0."""
    b = np.asarray(bits, dtype=np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b).astype(np.uint32)
    return b ^ np.where(b >> np.uint32(31) == 1, np.uint32(0xffffffff), np.uint32(0x80000000))


def unord32(o):
    """ord32 undone (an image has one preimage once -0.0 is +0.0)."""
    o = np.asarray(o, dtype=np.uint32)
    return np.where(o >> np.uint32(31) == 1, o ^ np.uint32(0x80000000), ~o).astype(np.uint32)


def pack_low(tag, q, b):
    """The key's low word: tag << 16 | q << 5 | b (16 + 11 + 5 bits)."""
    return (np.asarray(tag, dtype=np.uint64) << np.uint64(16)) | (np.asarray(q, dtype=np.uint64) << np.uint64(5)) | np.asarray(b, dtype=np.uint64)


def unpack_low(lo):
    lo = np.asarray(lo, dtype=np.uint64)
    return ((lo >> np.uint64(16)) & np.uint64(0xffff)).astype(np.int64), ((lo >> np.uint64(5)) & np.uint64(2047)).astype(np.int64), \
        (lo & np.uint64(31)).astype(np.int64)


def candidates(ddg, S_var, base, tag, skip, cutoff=None, include_cys=False, upper=False):
    """ddg [V, L, >= 20] float32, S_var [V, L], base / tag / skip [V] -> (o uint32, tag, q, b int64): every candidate of the call."""
    ddg = np.asarray(ddg, dtype=np.float32)[:, :, :20]
    V, L = ddg.shape[:2]
    s = np.asarray(S_var).astype(np.int64).reshape(V, L)[:, :, None]
    base = np.asarray(base, dtype=np.float32).reshape(V)
    tag, skip = np.asarray(tag).astype(np.int64).reshape(V), np.asarray(skip).astype(np.int64).reshape(V)
    cut = np.float32(np.inf if cutoff is None else cutoff)
    with np.errstate(invalid="ignore", over="ignore"):              # inf - inf: the NaN is the point
        val = base[:, None, None] + ddg                             # np.float32 + np.float32: one IEEE add
        ok = ~np.isnan(val) & (val <= cut)
    assert val.dtype == np.float32
    q = np.arange(L, dtype=np.int64)[None, :, None]
    b = np.arange(20, dtype=np.int64)[None, None, :]
    ok &= ((tag >= 0) & (tag <= MAX_TAG))[:, None, None] & (s >= 0) & (s < 20) & (b != s)
    ok &= (q > skip[:, None, None]) if upper else (q != skip[:, None, None])
    if not include_cys:
        ok &= b != CYS
    v_i, q_i, b_i = np.nonzero(ok)
    return ord32(val[ok].view(np.uint32)), tag[v_i], q_i.astype(np.int64), b_i.astype(np.int64)


def variant_hits_reference(ddg, S_var, base, tag, skip, k, cutoff=None, include_cys=False, upper=False, state=None):
    """One call. ``state``: None (a selection starts) or the uint64 [k] keys an earlier call returned. -> dict(hit_ddg [k] float32
    padded with NaN (a -0.0 sum as +0.0), hit_tag / hit_pos / hit_aa [k] int32 padded with -1, hit_count [1] int32, state uint64 [k]
    padded with all ones)."""
    skip = np.full(len(np.asarray(tag).reshape(-1)), -1) if skip is None else skip
    o, t, q, b = candidates(ddg, S_var, base, tag, skip, cutoff, include_cys, upper)
    if state is not None:
        old = np.asarray(state, dtype=np.uint64)
        assert old.shape == (k,)
        old = old[old != NONE]
        t0, q0, b0 = unpack_low(old & np.uint64(0xffffffff))
        o = np.concatenate([o, (old >> np.uint64(32)).astype(np.uint32)])
        t, q, b = np.concatenate([t, t0]), np.concatenate([q, q0]), np.concatenate([b, b0])
    order = np.lexsort((b, q, t, o))[:k]
    n = len(order)
    out = dict(hit_ddg=np.full(k, np.nan, np.float32), hit_tag=np.full(k, -1, np.int32), hit_pos=np.full(k, -1, np.int32),
               hit_aa=np.full(k, -1, np.int32), hit_count=np.array([n], np.int32), state=np.full(k, NONE, np.uint64))
    out["hit_ddg"][:n] = unord32(o[order]).view(np.float32)
    out["hit_tag"][:n], out["hit_pos"][:n], out["hit_aa"][:n] = t[order], q[order], b[order]
    out["state"][:n] = (o[order].astype(np.uint64) << np.uint64(32)) | pack_low(t[order], q[order], b[order])
    return out


def _np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def assert_variant_hits_equal(got, want):
    """Exact: counts, tags, positions, letters, the state's keys, and the value BITS with -0.0 taken as +0.0."""
    g = {k_: _np(v) for k_, v in got.items()}
    np.testing.assert_array_equal(g["hit_count"], want["hit_count"])
    for name in ("hit_tag", "hit_pos", "hit_aa"):
        np.testing.assert_array_equal(g[name], want[name], err_msg=name)
    a, b = g["hit_ddg"].astype(np.float32).view(np.uint32).copy(), want["hit_ddg"].view(np.uint32).copy()
    a[a == 0x80000000], b[b == 0x80000000] = 0, 0
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(g["state"].view(np.uint64), want["state"].view(np.uint64))
