"""The contract of tmpnn_beam_step_each (include/tmpnn.h) restated in numpy: a loop over the proteins of a pack of
beam_restatement.beam_step_reference on each protein's slices, behind the range check the device makes on the offsets (count -1 and
padding for a refused protein, none of its columns of out_S written), and the assembly of out_S [k, T]. Shared by
tests/test_beam_each_host.py and tests/test_gpu_beam_each.py; every device comparison against it is exact."""
import numpy as np

from beam_restatement import OUTPUTS, _np, assert_beam_equal, beam_step_reference, duplicate_fixture


def range_ok(offsets, p, T, max_len):
    """The device's predicate, on Python integers: 0 <= offsets[p] <= offsets[p + 1] <= T and L_p <= max_len."""
    lo, hi = int(offsets[p]), int(offsets[p + 1])
    return 0 <= lo <= hi <= T and hi - lo <= max_len


def beam_step_each_reference(ddg, S_var, score, muts, offsets, depth, k, allowed=None, cutoff=None, include_cys=False, max_len=None,
                             fill=20):
    """ddg [V, T, >= 20], S_var [V, T], score [P, V], muts [P, V, depth - 1] or None, offsets [P + 1], allowed [T] or None ->
    dict(out_muts [P, k, depth], out_score [P, k], out_parent [P, k], out_count [P], out_S [k, T]) and, per protein, ``good`` and
    ``dropped``. ``fill``: what out_S holds before the call (the engine allocates it with 20); only good proteins' columns are
    written. ``max_len`` None: the longest range that lies in the table."""
    ddg, S_var = np.asarray(ddg, dtype=np.float32), np.asarray(S_var)
    V, T = S_var.shape
    offsets = np.asarray(offsets).astype(np.int64).reshape(-1)
    P = len(offsets) - 1
    score = np.asarray(score, dtype=np.float32).reshape(P, V)
    if max_len is None:
        max_len = max([int(offsets[p + 1] - offsets[p]) for p in range(P) if range_ok(offsets, p, T, T)], default=0)
    out = dict(out_muts=np.full((P, k, depth), -1, np.int32), out_score=np.full((P, k), np.nan, np.float32),
               out_parent=np.full((P, k), -1, np.int32), out_S=np.full((k, T), fill, np.int32), out_count=np.zeros(P, np.int32),
               good=[], dropped=[])
    for p in range(P):
        good = range_ok(offsets, p, T, max_len)
        out["good"].append(good)
        if not good:
            out["out_count"][p] = -1
            out["dropped"].append(0)
            continue
        o, e = int(offsets[p]), int(offsets[p + 1])
        one = beam_step_reference(ddg[:, o:e], S_var[:, o:e], score[p], None if muts is None or depth == 1 else np.asarray(muts)[p], depth, k,
                                  None if allowed is None else np.asarray(allowed)[o:e], cutoff, include_cys)
        out["out_muts"][p], out["out_score"][p], out["out_parent"][p] = one["out_muts"], one["out_score"], one["out_parent"]
        out["out_count"][p] = one["out_count"][0]
        out["out_S"][:, o:e] = one["out_S"]
        out["dropped"].append(one["dropped"])
    return out


def protein_outputs(res, p, offsets):
    """Protein p's part of a packed result (device tensors or numpy) in the layout of one ``beam_step``."""
    o, e = int(offsets[p]), int(offsets[p + 1])
    return dict(out_muts=_np(res["out_muts"])[p], out_score=_np(res["out_score"])[p], out_parent=_np(res["out_parent"])[p],
                out_S=_np(res["out_S"])[:, o:e], out_count=_np(res["out_count"])[p:p + 1])


def assert_beam_each_equal(got, want, offsets, proteins=None):
    """``assert_beam_equal`` per protein. Refused proteins (count -1) are compared on count and padding; they have no columns."""
    counts = _np(got["out_count"]).reshape(-1)
    np.testing.assert_array_equal(counts, want["out_count"])
    for p in range(len(counts)) if proteins is None else proteins:
        if want["out_count"][p] < 0:
            g = {name: _np(got[name])[p] for name in ("out_muts", "out_score", "out_parent")}
            assert (g["out_muts"] == -1).all() and (g["out_parent"] == -1).all() and np.isnan(g["out_score"]).all(), p
        else:
            assert_beam_equal(protein_outputs(got, p, offsets), protein_outputs(want, p, offsets))


def pack_fixture(depth, V, lens, seed, n_pool=6, ld=21):
    """``duplicate_fixture``s of seeds ``seed``, ``seed`` + 1, ... and lengths ``lens`` side by side along the row axis, with common V
    and depth; a length 0 is a protein without a row. -> dict(ddg [V, T, ld], S_var [V, T], score [P, V], muts [P, V, depth - 1] or
    None, depth, offsets [P + 1] int32, parts: the proteins' own fixtures (None for an empty one))."""
    parts = [duplicate_fixture(depth, V, L, seed + i, n_pool=n_pool, ld=ld) if L > 0 else None for i, L in enumerate(lens)]
    live = [fx for fx in parts if fx is not None]
    ddg = np.concatenate([fx["ddg"] for fx in live], axis=1) if live else np.zeros((V, 0, ld), np.float32)
    S_var = np.concatenate([fx["S_var"] for fx in live], axis=1) if live else np.zeros((V, 0), np.int32)
    score = np.stack([fx["score"] if fx is not None else np.zeros(V, np.float32) for fx in parts]) if parts else np.zeros((0, V), np.float32)
    muts = None
    if depth > 1:
        muts = np.stack([fx["muts"] if fx is not None else np.zeros((V, depth - 1), np.int32) for fx in parts]) if parts else \
            np.zeros((0, V, depth - 1), np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return dict(ddg=ddg, S_var=S_var, score=score, muts=muts, depth=depth, offsets=offsets, parts=parts)


def reorder_pack(fx, order):
    """The same proteins in another order (an index may repeat) -> a fixture of the same form."""
    o = fx["offsets"]
    cols = [np.arange(int(o[p]), int(o[p + 1])) for p in order]
    idx = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
    return dict(ddg=fx["ddg"][:, idx], S_var=fx["S_var"][:, idx], score=fx["score"][list(order)],
                muts=None if fx["muts"] is None else fx["muts"][list(order)], depth=fx["depth"],
                offsets=np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32), parts=[fx["parts"][p] for p in order])


__all__ = ["OUTPUTS", "assert_beam_each_equal", "beam_step_each_reference", "pack_fixture", "protein_outputs", "range_ok", "reorder_pack"]
