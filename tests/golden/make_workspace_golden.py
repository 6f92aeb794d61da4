"""Record what every *_bytes() function of the C-ABI returns, on the grid tests/test_workspace_host.py checks.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_workspace_golden.py

Run ONCE, on the commit before the sizers were rewritten as their carve run without a base (Carver, csrc/tmpnn_internal.h): the file
holds that commit's answers, and a refactor of the carving is held to them. It is never regenerated from the code under test. The sizers launch
nothing: a machine without a GPU gives the same numbers. workspace_sizes.json: {function: [[arguments, value], ...]}; a head's
``dims`` is a list inside the arguments.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

T_MAX = (1 << 31) // 192 - 1          # int32 tile arithmetic inside the kernels
ROWS_MAX = (1 << 24) - 1              # (V + 1) T rows of the ordered decode, 3 N T rows of the sampler
TS = [-1, 0, 1, 17, 32, 40, 57, 256, 2048, T_MAX, T_MAX + 1]
# n_final, lightattn, dims: the released head (384 -> 64 -> 32 -> 21 over the last two decoder states) and the same widths over three
# states (512 -> ...), each with and without LightAttention; the fixtures 2OCJ_A_headB / _headC of test_gpu_e2e.py; and a first width
# that is not 128 * n_final + 128
HEADS = [(2, 1, [384, 64, 32, 21]), (2, 0, [384, 64, 32, 21]), (3, 1, [512, 64, 32, 21]), (3, 0, [512, 64, 32, 21]), (1, 0, [256, 32, 21]),
         (0, 1, [128, 21]), (3, 1, [500, 64, 32, 21])]


def two_sides(T, limit):
    """The largest V with V * T <= limit, and the one after it."""
    return [(T, limit // T), (T, limit // T + 1)]


def grid():
    rows = {}
    for f in ("tmpnn_layer_workspace_bytes", "tmpnn_workspace_bytes", "tmpnn_encode_bytes", "tmpnn_encode_workspace_bytes"):
        rows[f] = [[T] for T in TS]
    tv = [(T, V) for T in TS for V in (-1, 0, 1, 5, 300)]
    for T in (1, 17, 2048):
        tv += two_sides(T, T_MAX)
    # (V + 1) T <= ROWS_MAX binds below V T <= T_MAX for V = 1 only (T_MAX < ROWS_MAX): the two sides in T, and V = 2 beside them
    tv += [(ROWS_MAX // 2, 1), (ROWS_MAX // 2 + 1, 1), (ROWS_MAX // 3, 2), (ROWS_MAX // 3 + 1, 2)]
    rows["tmpnn_decode_variants_workspace_bytes"] = [list(a) for a in tv]
    rows["tmpnn_decode_ordered_workspace_bytes"] = [list(a) for a in tv]
    tn = [(T, N) for T in TS for N in (-1, 0, 1, 16, 17, 300)]
    for T in (1, 17, 2048):
        tn += two_sides(T, ROWS_MAX // 3)
    rows["tmpnn_sample_workspace_bytes"] = [list(a) for a in tn]
    ms, ls = (0, 1, 17, 300), (2, 17, 40, 256)
    rows["tmpnn_head_generic_workspace_bytes"] = [[M, nf, len(d) - 1, d] for nf, _, d in HEADS for M in ms]
    rows["tmpnn_head_train_workspace_bytes"] = [[M, nf, la, len(d) - 1, d] for nf, la, d in HEADS for M in ms]
    for f in ("tmpnn_finetune_workspace_bytes", "tmpnn_finetune_saved_bytes", "tmpnn_finetune_scratch_bytes"):
        rows[f] = [[L, M, nf, la, len(d) - 1, d] for nf, la, d in HEADS for L in ls for M in ms]
    return rows


def call(lib, name, args):
    """One sizer on one row of arguments (a list among them is the head's dims, passed as int32[])."""
    return int(getattr(lib, name)(*[(C.c_int32 * len(a))(*a) if isinstance(a, list) else a for a in args]))


if __name__ == "__main__":
    from thermompnn_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    out = {f: [[a, call(lib, f, a)] for a in rows] for f, rows in grid().items()}
    anchors = {"tmpnn_workspace_bytes": ([17], 503552), "tmpnn_encode_bytes": ([17], 447232),
               "tmpnn_decode_ordered_workspace_bytes": ([17, 5], 327424), "tmpnn_sample_workspace_bytes": ([17, 17], 480256)}
    for f, (a, v) in anchors.items():
        assert [a, v] in out[f], (f, a, v)
    with open(os.path.join(HERE, "workspace_sizes.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(f' "{f}": {json.dumps(rows, separators=(",", ":"))}' for f, rows in out.items()) + "\n}\n")
    print({f: len(rows) for f, rows in out.items()})
