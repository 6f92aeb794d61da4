"""Sizes and carves of the caller-owned buffers, without a GPU.

Every *_bytes() function of the C-ABI is its buffer's layout function run on a Carver without a base (csrc/tmpnn_internal.h).
tests/golden/workspace_sizes.json holds what the sizers returned BEFORE that rewrite (make_workspace_golden.py, never regenerated
from the code under test): every row must still come out, the zeros at and beyond the bounds included. The entries are then held to
their sizers with fake, never dereferenced pointers: one byte less than a pre-checking entry's size is refused with both numbers in
the message; an entry that takes whatever its carve fits is refused one byte below what the carve takes. tmpnn_sample, the one entry
with a refusal behind its workspace check (an fp32 handle), also shows the other side on any base alignment; for the others that
side needs launches and is tests/test_gpu_workspace.py, whose table of covered entries is held to include/tmpnn.h here. The
range-retry helper of engine.py is tested here with stub callables."""
import ctypes as C
import json
import os
import sys
import warnings

import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from make_workspace_golden import call  # noqa: E402

E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
P = C.c_void_p
BUF = P(0x1000)                          # never dereferenced: every check here comes before any launch
DIMS = [384, 64, 32, 21]                 # the released head: n_final 2, LightAttention
SIZES = json.load(open(os.path.join(GOLDEN, "workspace_sizes.json")))


@pytest.fixture(scope="module")
def lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


def err(lib):
    return lib.tmpnn_last_error().decode()


def refused_below(lib, entry, need):
    """``entry(ws, bytes)`` with one byte less than ``need`` -> TMPNN_E_WORKSPACE, and the message states both sizes."""
    assert need > 0
    assert entry(BUF, need - 1) == E_WORKSPACE and f"{need - 1} < {need} bytes" in err(lib), err(lib)
    assert entry(None, need) == E_WORKSPACE


@pytest.mark.parametrize("name", sorted(SIZES))
def test_sizers_return_what_they_returned_before(lib, name):
    rows = SIZES[name]
    assert len(rows) >= 11
    for args, want in rows:
        assert call(lib, name, args) == want, (name, args)


def test_the_fixture_is_the_recorded_one():
    """The anchors of the tree the fixture was recorded on, and both sides of every bound."""
    at = lambda f, a: dict((json.dumps(k), v) for k, v in SIZES[f])[json.dumps(a)]
    assert at("tmpnn_workspace_bytes", [17]) == 503552 and at("tmpnn_encode_bytes", [17]) == 447232
    assert at("tmpnn_decode_ordered_workspace_bytes", [17, 5]) == 327424 and at("tmpnn_sample_workspace_bytes", [17, 17]) == 480256
    T_MAX, ROWS = (1 << 31) // 192 - 1, (1 << 24) - 1
    for f in ("tmpnn_decode_variants_workspace_bytes", "tmpnn_decode_ordered_workspace_bytes"):
        assert at(f, [2048, T_MAX // 2048]) > 0 and at(f, [2048, T_MAX // 2048 + 1]) == 0
        assert at(f, [T_MAX + 1, 1]) == 0 and at(f, [-1, 5]) == 0 and at(f, [17, -1]) == 0
    assert at("tmpnn_decode_ordered_workspace_bytes", [ROWS // 2, 1]) > 0                 # (V + 1) T = 2^24 - 2
    assert at("tmpnn_decode_ordered_workspace_bytes", [ROWS // 2 + 1, 1]) == 0
    assert at("tmpnn_decode_variants_workspace_bytes", [ROWS // 2 + 1, 1]) > 0            # that bound is the ordered decode's alone
    assert at("tmpnn_decode_variants_workspace_bytes", [T_MAX, 1]) > 0 and at("tmpnn_decode_ordered_workspace_bytes", [T_MAX, 1]) == 0
    assert at("tmpnn_sample_workspace_bytes", [2048, ROWS // 3 // 2048]) > 0
    assert at("tmpnn_sample_workspace_bytes", [2048, ROWS // 3 // 2048 + 1]) == 0
    assert at("tmpnn_layer_workspace_bytes", [T_MAX + 1]) > 0 and at("tmpnn_workspace_bytes", [-1]) == 0
    assert at("tmpnn_finetune_workspace_bytes", [40, 17, 3, 1, 3, [500, 64, 32, 21]]) == 0


def test_decode_and_sample_need_exactly_their_size(lib):
    T, V, N = 17, 3, 17
    ctx_bytes = lib.tmpnn_encode_bytes(T)
    for ordered in (False, True):
        sizer = lib.tmpnn_decode_ordered_workspace_bytes if ordered else lib.tmpnn_decode_variants_workspace_bytes
        f = lib.tmpnn_decode_ordered if ordered else lib.tmpnn_decode_variants
        rank = [BUF] if ordered else []
        refused_below(lib, lambda ws, n: f(BUF, BUF, ctx_bytes, BUF, *rank, V, BUF, T, None, None, BUF, None, ws, n, None), sizer(T, V))
    handle = (C.c_int32 * 16384)()       # a zeroed handle: precision 0 = fp32, the chain kernel's documented refusal
    sample = lambda ws, n: lib.tmpnn_sample(C.cast(handle, P), BUF, ctx_bytes, BUF, T, N, BUF, BUF, BUF, BUF, 1.0, None, None, BUF, None, None,
                                            ws, n, None)
    need = lib.tmpnn_sample_workspace_bytes(T, N)
    refused_below(lib, sample, need)
    for base in (0x1000, 0x1010, 0x10f0, 0x10ff):        # the measured carve plus the skipped bytes fits the size on any alignment
        assert sample(P(base), need) == E_UNSUPPORTED and "fp32" in err(lib), base
        assert sample(P(base), need - 1) == E_WORKSPACE


def test_entries_that_take_what_fits_need_exactly_their_carve(lib):
    """ssm_forward, encode and the layer entries: the size is the carve + 256 bytes per alignment of the base (two for ssm_forward);
    an aligned base one byte below the carve is refused. (Above it they launch: test_gpu_workspace.py.)"""
    T = 17
    size_of = lambda fn: [r for r in SIZES[fn] if r[0] == [T]][0][1]
    ssm = lambda ws, n: lib.tmpnn_ssm_forward(BUF, BUF, BUF, BUF, BUF, BUF, BUF, 1, T, T, 48, None, BUF, None, None, None, ws, n, None)
    enc = lambda ws, n: lib.tmpnn_encode(BUF, BUF, BUF, BUF, BUF, BUF, 1, T, T, 48, BUF, 1 << 30, None, ws, n, None)
    enc_layer = lambda ws, n: lib.tmpnn_enc_layer(BUF, 0, BUF, BUF, BUF, BUF, T, ws, n, None)
    dec_layer = lambda ws, n: lib.tmpnn_dec_layer(BUF, 0, BUF, BUF, BUF, BUF, BUF, BUF, T, ws, n, None)
    for entry, fn, slack in ((ssm, "tmpnn_workspace_bytes", 512), (enc, "tmpnn_encode_workspace_bytes", 256),
                             (enc_layer, "tmpnn_layer_workspace_bytes", 256), (dec_layer, "tmpnn_layer_workspace_bytes", 256)):
        carve = size_of(fn) - slack
        assert entry(BUF, carve - 1) == E_WORKSPACE and "workspace" in err(lib), fn
        assert entry(P(0x1010), carve + 0xf0 - 1) == E_WORKSPACE, fn        # the bytes skipped up to the boundary are charged
        assert entry(P(0x1010), 0xef) == E_WORKSPACE and entry(None, 1 << 30) == E_WORKSPACE, fn
    assert lib.tmpnn_encode(BUF, BUF, BUF, BUF, BUF, BUF, 1, T, T, 48, P(0x1010), 1 << 30, None, BUF, 1 << 30, None) == E_INVALID
    assert "aligned" in err(lib)                                                # a ctx that is not 256-byte aligned is still refused


def test_head_and_training_entries_need_exactly_their_size(lib):
    cd = (C.c_int32 * 4)(*DIMS)
    M, L = 17, 40
    generic = lambda ws, n: lib.tmpnn_ddg_head_generic((P * 2)(0x1000, 0x1000), 2, BUF, BUF, M, BUF, BUF, 3, (P * 3)(0x1000, 0x1000, 0x1000),
                                                       (P * 3)(0x1000, 0x1000, 0x1000), cd, BUF, BUF, BUF, None, ws, n, None, None)
    refused_below(lib, generic, lib.tmpnn_head_generic_workspace_bytes(M, 2, 3, cd))
    numel = lib.tmpnn_head_slab_numel(2, 1, 3, cd)
    step = lambda ws, n: lib.tmpnn_head_train_step(BUF, M, BUF, BUF, BUF, BUF, M, 2, 1, 3, cd, 1, BUF, BUF, numel, 0.25, None, None, 0, 1, BUF,
                                                   None, ws, n, None)
    evaluate = lambda ws, n: lib.tmpnn_head_eval(BUF, M, BUF, BUF, BUF, M, 2, 1, 3, cd, 1, BUF, numel, BUF, ws, n, None)
    need = lib.tmpnn_head_train_workspace_bytes(M, 2, 1, 3, cd)
    refused_below(lib, step, need)
    refused_below(lib, evaluate, need)
    numel = lib.tmpnn_finetune_slab_numel(2, 1, 3, cd)
    model = (L, BUF, BUF, BUF)
    ft_step = lambda ws, n: lib.tmpnn_finetune_step(BUF, BUF, BUF, BUF, BUF, *model, BUF, M, 2, 1, 3, cd, 1, BUF, BUF, numel, 0.1, 0.25, None,
                                                    None, None, 0, 1, BUF, None, None, None, ws, n, None)
    ft_eval = lambda ws, n: lib.tmpnn_finetune_eval(BUF, BUF, BUF, BUF, BUF, *model, M, 2, 1, 3, cd, 1, BUF, numel, BUF, None, None, ws, n, None)
    ft_fwd = lambda ws, n: lib.tmpnn_finetune_forward(BUF, BUF, BUF, BUF, BUF, *model, M, 2, 1, 3, cd, 1, BUF, numel, 0.1, 0.25, None, None,
                                                      None, 0, 1, BUF, None, None, ws, n, None)
    saved = lib.tmpnn_finetune_saved_bytes(L, M, 2, 1, 3, cd)
    ft_bwd = lambda sv, nsv, sc, nsc: lib.tmpnn_finetune_backward(BUF, BUF, BUF, BUF, BUF, *model, M, 2, 1, 3, cd, 1, BUF, numel, 0.1, 0.25,
                                                                  None, None, 0, 1, BUF, BUF, 1, sv, nsv, sc, nsc, None)
    need = lib.tmpnn_finetune_workspace_bytes(L, M, 2, 1, 3, cd)
    refused_below(lib, ft_step, need)
    refused_below(lib, ft_eval, need)
    refused_below(lib, ft_fwd, saved)
    refused_below(lib, lambda ws, n: ft_bwd(ws, n, BUF, 1 << 40), saved)
    refused_below(lib, lambda ws, n: ft_bwd(BUF, saved, ws, n), lib.tmpnn_finetune_scratch_bytes(L, M, 2, 1, 3, cd))


def test_every_entry_with_a_caller_owned_buffer_has_a_window_test():
    """include/tmpnn.h: every function with a ``void *`` or ``const void *`` parameter named workspace, saved, scratch, packed or ctx
    is a key of tests/test_gpu_workspace.py's COVERED table, the table names nothing else, and every test it names exists."""
    import importlib
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "tmpnn.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    takes_buffer = re.compile(r"\b(?:const\s+)?void\s*\*\s*(?:workspace|saved|scratch|packed|ctx)\b")
    declared = {name for name, params in re.findall(r"\b(tmpnn_\w+)\s*\(([^;{]*?)\)\s*;", header) if takes_buffer.search(params)}
    assert len(declared) >= 34 and {"tmpnn_ssm_forward", "tmpnn_weights_create", "tmpnn_seqloss_batch_backward_x"} <= declared
    covered = importlib.import_module("test_gpu_workspace").COVERED
    assert sorted(covered) == sorted(declared)
    for entry, tests in covered.items():
        assert tests, entry
        for where in tests:
            module, test = where.split("::")
            assert module in ("test_gpu_workspace", "test_gpu_workspace_entries") and callable(getattr(importlib.import_module(module), test)), where


# ---- engine.range_retry: the one range contract of ssm_forward, decode_variants, decode_ordered and sample --------------------------
RANGE, MAXLEN = 1, 2
TEXT = "ThermoMPNN HIP engine: non-finite result in f16x2 (an operand left the fp16 range); rerunning this batch at precision bf16x3"


def runs(*words):
    """A stub ``run``: returns the given status words in turn and records the precisions it was called at."""
    seen, left = [], list(words)

    def run(precision):
        seen.append(precision)
        return left.pop(0)
    return run, seen


def public_method(run, used, retry):
    """Stands for Engine.sample: the frame the warning must NOT be attributed to."""
    from thermompnn_amd.engine import range_retry
    range_retry(run, used, retry, "demo")


def test_range_retry(lib):
    from thermompnn_amd._lib import TmpnnError, TmpnnRangeError
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        run, seen = runs(0)
        public_method(run, "f16x2", "bf16x3")                     # no RANGE bit: one run
        assert seen == ["f16x2"] and not rec
        run, seen = runs(RANGE, 0)
        here = sys._getframe().f_lineno + 1
        public_method(run, "f16x2", "bf16x3")
        assert seen == ["f16x2", "bf16x3"]
        assert len(rec) == 1 and str(rec[0].message) == TEXT and rec[0].category is RuntimeWarning
        assert os.path.samefile(rec[0].filename, __file__) and rec[0].lineno == here         # the public method's caller, not the method
        del rec[:]
        for used, retry in (("f16x2", None), ("f16x2", "f16x2"), ("bf16x3", "fp32"), ("fp32", "bf16x3")):
            run, seen = runs(RANGE, 0)
            with pytest.raises(TmpnnRangeError, match=rf"tmpnn_demo\[{used}\]"):
                public_method(run, used, retry)
            assert seen == [used] and not rec
        run, seen = runs(RANGE, RANGE)                            # a bit left after the rerun
        with pytest.raises(TmpnnRangeError, match=r"tmpnn_demo\[bf16x3\]"):
            public_method(run, "f16x2", "bf16x3")
        assert seen == ["f16x2", "bf16x3"] and len(rec) == 1
        del rec[:]
        run, seen = runs(RANGE, MAXLEN)
        with pytest.raises(TmpnnError, match="max_len"):
            public_method(run, "f16x2", "bf16x3")
        run, seen = runs(MAXLEN | RANGE, 0)                       # an over-long protein is no range problem: no rerun
        with pytest.raises(TmpnnError, match="max_len"):
            public_method(run, "f16x2", "bf16x3")
        assert seen == ["f16x2"] and len(rec) == 1
