"""Global alignment on the device (tmpnn_align_global, Engine.align_global) against the numpy restatement of the contract
(tests/align_restatement.py, which tests/test_align_host.py holds against datasets.global_alignment_map). Every comparison is exact:
out, aligned and status. The sequences are crafted (tests/align_inputs.py)."""
import functools

import numpy as np
import pytest
import torch

from align_inputs import KINDS, LONG, SMALL, make_pair, mixed_batch, pack, small_batch
from align_restatement import MAX_LEN, align_map, align_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


@functools.lru_cache(maxsize=None)
def _mixed():
    """The P = 300 batch and its restatement, computed once; left unchanged by the tests that share it."""
    pairs = mixed_batch()
    adds = [0 if k % 3 == 0 else (1000 + k if k % 3 == 1 else -5 * k) for k in range(len(pairs))]
    A, B, desc, NO = pack(pairs, adds)
    return pairs, A, B, desc, NO, align_reference(A, B, desc, NO, 257, 257)


def _equal(got, want):
    np.testing.assert_array_equal(got["status"].cpu().numpy(), want["status"])
    np.testing.assert_array_equal(got["aligned"].cpu().numpy(), want["aligned"])
    np.testing.assert_array_equal(got["out"].cpu().numpy(), want["out"])


def test_every_kind_at_every_small_size(engine):
    batch = small_batch()
    assert {(n, m) for _, n, m, _, _ in batch} == set(SMALL) and {k for k, *_ in batch} == set(KINDS)
    A, B, desc, NO = pack([(a, b) for *_, a, b in batch])
    want = align_reference(A, B, desc, NO, 257, 257)
    got = engine.align_global(A, B, desc)
    assert got["out"].dtype == torch.int32 and got["out"].is_cuda and got["out"].numel() == NO
    _equal(got, want)
    out = got["out"].cpu().numpy()
    for (kind, n, m, a, b), d in zip(batch, desc.tolist()):
        mine = out[d[4]:d[4] + n]
        if kind == "identical":
            assert mine.tolist() == list(range(n))                                   # the identity
        if kind == "disjoint":
            assert (mine == -1).all()
        if kind == "deletions":
            assert (mine >= 0).sum() == n - 5                                        # (which of two equal neighbours stays out is the tie rule's)
        assert all(0 <= a[q] < 20 and a[q] == b[j] for q, j in enumerate(mine) if j >= 0)     # mapped letters are identical
    # each pair alone: the same entries
    for k in (4, len(batch) - 6, len(batch) - 1):
        _, n, m, a, b = batch[k]
        alone = engine.align_global(a, b, [(0, n, 0, m, 0, 0)])
        assert alone["out"].cpu().numpy().tolist() == out[desc[k, 4]:desc[k, 4] + n].tolist()


@pytest.mark.parametrize("n,m", LONG)
def test_diagonals_longer_than_one_pass(engine, n, m):
    rng = np.random.default_rng(n)
    pairs = [make_pair(kind, n, m, rng) for kind in ("two", "nonmatch", "deletions")]
    A, B, desc, NO = pack(pairs, adds=[0, 7, -3])
    want = align_reference(A, B, desc, NO, n, max(m, n))
    _equal(engine.align_global(A, B, desc), want)
    assert want["aligned"][2] == n - 5


def test_the_longest_pair(engine):
    rng = np.random.default_rng(8)
    a, b = make_pair("two", MAX_LEN, MAX_LEN - 1, rng)
    mp, count = align_map(a, b)
    got = engine.align_global(a, b, [(0, MAX_LEN, 0, MAX_LEN - 1, 0, 0)])
    assert got["status"].tolist() == [0] and got["aligned"].tolist() == [count]
    np.testing.assert_array_equal(got["out"].cpu().numpy(), mp.astype(np.int32))
    from thermompnn_amd._lib import TmpnnError
    with pytest.raises(TmpnnError, match="8192"):
        engine.align_global(a, b, [(0, 5, 0, 5, 0, 0)], max_n=MAX_LEN + 1)


def test_batch_of_300_alone_reversed_one_slot_and_rerun(engine):
    pairs, A, B, desc, NO, want = _mixed()
    assert len(pairs) == 300 and (desc[:, 5] > 0).any() and (desc[:, 5] < 0).any()
    first = engine.align_global(A, B, desc)
    _equal(first, want)
    again = engine.align_global(A, B, desc)                                          # a rerun: the same bits
    one_slot = engine.align_global(A, B, desc, slots=1)                              # one workgroup takes all 300 in turn
    seven = engine.align_global(A, B, desc, slots=7)
    for other in (again, one_slot, seven):
        for name in ("out", "aligned", "status"):
            assert torch.equal(first[name], other[name]), name
    # reversed order of the pairs, the same out ranges
    rev = engine.align_global(A, B, desc[::-1].copy())
    assert torch.equal(rev["out"], first["out"]) and torch.equal(rev["aligned"], first["aligned"].flip(0))
    # pairs alone, as their own call on their own buffers
    out = first["out"].cpu().numpy()
    for k in (0, 7, 57, 150, 299):
        a, b = pairs[k]
        alone = engine.align_global(a, b, [(0, len(a), 0, len(b), 0, int(desc[k, 5]))])
        assert alone["out"].cpu().numpy().tolist() == out[desc[k, 4]:desc[k, 4] + len(a)].tolist()
        assert alone["aligned"].tolist() == [int(want["aligned"][k])]


def _raw(A, B, desc, max_n, max_m, out, NA=None, NB=None, NO=None, ws_bytes=None, P=None, null=()):
    """The C entry itself on caller-made descriptors and prefilled outputs -> (rc, out, aligned, status)."""
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import _ptr, _stream
    lib = _lib.load()
    dA, dB = torch.from_numpy(np.asarray(A, np.int32)).cuda(), torch.from_numpy(np.asarray(B, np.int32)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.int32)).cuda()
    P = len(desc) if P is None else P
    dout = torch.from_numpy(np.asarray(out, np.int32).copy()).cuda()
    aligned = torch.full((max(len(desc), 1),), 66, dtype=torch.int32, device="cuda")
    status = torch.full((max(len(desc), 1),), 77, dtype=torch.int32, device="cuda")
    need = lib.tmpnn_align_workspace_bytes(min(max_n, MAX_LEN), min(max_m, MAX_LEN), max(P, 1)) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    ptr = lambda name, t: None if name in null else _ptr(t)
    rc = lib.tmpnn_align_global(ptr("A", dA), len(A) if NA is None else NA, ptr("B", dB), len(B) if NB is None else NB, ptr("desc", d), P,
                                max_n, max_m, ptr("out", dout), len(out) if NO is None else NO, ptr("aligned", aligned),
                                ptr("status", status), ptr("ws", ws), need, _stream())
    torch.cuda.synchronize()
    return rc, dout.cpu().numpy(), aligned.cpu().numpy(), status.cpu().numpy()


def test_bad_descriptors_write_status_and_nothing_else():
    pairs, A, B, desc, NO, want = _mixed()
    keep = slice(0, 12)
    desc = desc[keep].copy()
    NA, NB = int(desc[-1, 0] + desc[-1, 1]), int(desc[-1, 2] + desc[-1, 3])
    NO = NA
    A, B = A[:NA], B[:NB]
    assert all(desc[e, 1] > 0 for e in (2, 3, 5, 8, 9, 11))
    bad = {"a0 < 0": (2, 0, -1), "n > max_n": (3, 1, 258), "b0 + m > NB": (11, 2, NB - int(desc[11, 3]) + 1), "m < 0": (5, 3, -4),
           "out0 + n > NO": (8, 4, NO - int(desc[8, 1]) + 1), "a0 + n > NA, beyond 32 bits": (9, 0, 0x7fffffff), "n < 0": (2, 1, -9),
           "m > max_m": (3, 3, 258)}
    assert len(bad) >= 6
    for what, (e, col, value) in bad.items():
        dd = desc.copy()
        dd[e, col] = value
        sentinel = np.full(NO, 0x5e5e5e5e, np.int32)
        ref = align_reference(A, B, dd, NO, 257, 257, out=sentinel, aligned=np.full(len(dd), 66, np.int32))
        assert ref["status"][e] == -1 and (np.delete(ref["status"], e) == 0).all(), what
        rc, out, aligned, status = _raw(A, B, dd, 257, 257, sentinel)
        assert rc == 0, what
        assert status.tolist() == ref["status"].tolist(), what
        np.testing.assert_array_equal(out, ref["out"], err_msg=what)                  # the pair's own entries keep the sentinel,
        np.testing.assert_array_equal(aligned, ref["aligned"], err_msg=what)          # the neighbours are exact
        o0, n = int(desc[e, 4]), int(desc[e, 1])
        assert (out[o0:o0 + n] == 0x5e5e5e5e).all() and aligned[e] == 66, what


def test_host_side_errors_and_empty_calls(engine):
    from thermompnn_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4                                      # TMPNN_E_* of include/tmpnn.h
    a, b = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32)
    desc = [(0, 5, 0, 5, 0, 0)]
    fill = np.full(5, 9, np.int32)
    rc, out, aligned, status = _raw(a, b, desc, 5, 5, fill)
    assert rc == 0 and out.tolist() == [0, 1, 2, 3, 4] and aligned.tolist() == [5] and status.tolist() == [0]
    for kw, code in ((dict(null=("A",)), INVALID), (dict(null=("out",)), INVALID), (dict(null=("desc",)), INVALID),
                     (dict(null=("status",)), INVALID), (dict(null=("ws",)), INVALID), (dict(NA=-1), INVALID), (dict(P=-1), INVALID),
                     (dict(ws_bytes=0), WORKSPACE)):
        rc, out, aligned, status = _raw(a, b, desc, 5, 5, fill, **kw)
        assert rc == code, (kw, rc, lib.tmpnn_last_error())
        assert out.tolist() == fill.tolist() and status.tolist() == [77]              # nothing was launched
    for max_n, max_m in ((MAX_LEN + 1, 5), (5, MAX_LEN + 1)):
        rc, out, _, status = _raw(a, b, desc, max_n, max_m, fill)
        assert rc == UNSUPPORTED and status.tolist() == [77]
    rc, out, _, status = _raw(a, b, desc, -1, 5, fill)
    assert rc == INVALID
    assert lib.tmpnn_align_workspace_bytes(MAX_LEN + 1, 5, 1) == 0 and lib.tmpnn_align_workspace_bytes(5, 5, 0) == 0
    assert lib.tmpnn_align_workspace_bytes(256, 256, 1) < lib.tmpnn_align_workspace_bytes(256, 256, 2)
    rc, out, _, status = _raw(a, b, desc, 5, 5, fill, P=0)                            # P == 0: a no-op
    assert rc == 0 and out.tolist() == fill.tolist() and status.tolist() == [77]
    none = engine.align_global(a, b, np.zeros((0, 6), np.int32))
    assert none["out"].numel() == 0 and none["aligned"].numel() == 0 and none["status"].numel() == 0
    empty = engine.align_global(np.zeros(0, np.int32), b, [(0, 0, 0, 5, 0, 0), (0, 0, 0, 0, 0, 3)])
    assert empty["status"].tolist() == [0, 0] and empty["aligned"].tolist() == [0, 0] and empty["out"].numel() == 0
