"""What the coordinates' gradient costs: tmpnn_seqloss_backward_x against tmpnn_seqloss_backward over the same `saved` (one forward,
then only backwards), and the packed pair tmpnn_seqloss_batch_backward_x / _backward, at the sizes of tools/seqloss_bench.py:
proteins of L in [40, 72], L = 256, L = 1024, and a pack of 64 proteins of L in [40, 72]. Synthetic weights and backbones, dropout
on (p = 0.1), a random decoding order, a random dL / dlog_probs. One process, the legs alternated inside every round, --rounds rounds
(default 5); reported per leg: the median over rounds of the mean ms per call, and the rounds' min and max.

With --parent-lib PATH (a libtmpnn.so built from the parent commit) the plain tmpnn_seqloss_backward of both libraries is timed the
same way, alternated, to show that the path without dX did not move.

    python tools/coordgrad_bench.py [--rounds 5] [--parent-lib PATH] [--out profiles/coordgrad_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def protein(L, seed):
    from thermompnn_amd.synthetic import AA20, synthetic_backbone
    X, seq = synthetic_backbone(L, seed)
    t = lambda a, dt: torch.as_tensor(np.asarray(a)).to("cuda", dt).contiguous()
    rng = np.random.default_rng(seed)
    return dict(X=t(X, torch.float32), S=t([AA20.index(c) for c in seq], torch.int32), mask=torch.ones(L, device="cuda"),
                ridx=t(np.arange(L), torch.int32), cenc=torch.ones(L, dtype=torch.int32, device="cuda"),
                ranks=t(rng.permutation(L), torch.int32), dlp=t(rng.normal(size=(L, 21)), torch.float32), L=L)


class Single:
    """One protein: forward once, then the two backwards over its `saved`."""

    def __init__(self, lib, slab, p, parent=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        self.lib, self.parent, self.p, self.slab = lib, parent, p, slab
        L = p["L"]
        self.saved = torch.empty(lib.tmpnn_seqloss_saved_bytes(L), dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(lib.tmpnn_seqloss_scratch_bytes(L), dtype=torch.uint8, device="cuda")
        self.grads = torch.zeros(slab.numel(), device="cuda")
        self.dX = torch.empty((L, 4, 3), device="cuda")
        self.head = (_ptr(p["X"]), _ptr(p["S"]), _ptr(p["mask"]), _ptr(p["ridx"]), _ptr(p["cenc"]), L, 48, _ptr(p["ranks"]), _ptr(slab),
                     slab.numel())
        lp = torch.empty((L, 21), device="cuda")
        check(lib.tmpnn_seqloss_forward(*self.head, 0.1, None, None, 7, 3, _ptr(lp), None, _ptr(self.saved), self.saved.numel(), _stream()))
        self.tail = (_ptr(self.saved), self.saved.numel(), _ptr(self.scratch), self.scratch.numel(), _stream())
        self._ptr = _ptr

    def plain(self, lib=None):
        rc = (lib or self.lib).tmpnn_seqloss_backward(*self.head, 0.1, None, 7, 3, self._ptr(self.p["dlp"]), self._ptr(self.grads), *self.tail)
        assert rc == 0, rc

    def with_x(self):
        rc = self.lib.tmpnn_seqloss_backward_x(*self.head, 0.1, None, 7, 3, self._ptr(self.p["dlp"]), self._ptr(self.grads),
                                               self._ptr(self.dX), *self.tail)
        assert rc == 0, rc

    def parent_plain(self):
        self.plain(self.parent)


class Packed:
    def __init__(self, lib, slab, prots):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        self.lib = lib
        cat = lambda k: torch.cat([p[k] for p in prots]).contiguous()
        self.t = {k: cat(k) for k in ("X", "S", "mask", "ridx", "cenc", "ranks", "dlp")}
        lens = [p["L"] for p in prots]
        starts = np.concatenate([[0], np.cumsum(lens)])
        self.offsets = torch.as_tensor(starts).to("cuda", torch.int32)
        n, T, K = len(prots), int(starts[-1]), min(48, min(lens))
        self.saved = torch.empty(lib.tmpnn_seqloss_batch_saved_bytes(T, n, K), dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(lib.tmpnn_seqloss_batch_scratch_bytes(T, n, K), dtype=torch.uint8, device="cuda")
        self.grads = torch.zeros(slab.numel(), device="cuda")
        self.dX = torch.empty((T, 4, 3), device="cuda")
        t = self.t
        self.head = (_ptr(t["X"]), _ptr(t["S"]), _ptr(t["mask"]), _ptr(t["ridx"]), _ptr(t["cenc"]), _ptr(self.offsets), n, T, min(lens),
                     max(lens), K, _ptr(t["ranks"]), _ptr(slab), slab.numel())       # one K for the pack: the shortest member's
        lp = torch.empty((T, 21), device="cuda")
        check(lib.tmpnn_seqloss_batch_forward(*self.head, 0.1, None, None, 7, 3, _ptr(lp), None, None, _ptr(self.saved), self.saved.numel(),
                                              _stream()))
        self.tail = (_ptr(self.saved), self.saved.numel(), _ptr(self.scratch), self.scratch.numel(), _stream())
        self._ptr, self.T, self.n, self.K = _ptr, T, n, K

    def plain(self):
        rc = self.lib.tmpnn_seqloss_batch_backward(*self.head, 0.1, None, 7, 3, self._ptr(self.t["dlp"]), self._ptr(self.grads), *self.tail)
        assert rc == 0, rc

    def with_x(self):
        rc = self.lib.tmpnn_seqloss_batch_backward_x(*self.head, 0.1, None, 7, 3, self._ptr(self.t["dlp"]), self._ptr(self.grads),
                                                     self._ptr(self.dX), *self.tail)
        assert rc == 0, rc


def ms_per_call(fns, reps):
    """Mean ms of one pass over ``fns``, ``reps`` passes between two device synchronisations."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        for f in fns:
            f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (reps * len(fns))


def alternated(legs, rounds, reps):
    """legs: {name: [callables]} -> {name: {median, min, max} ms per call}; every round runs every leg once, in turn."""
    for fns in legs.values():
        ms_per_call(fns, 1)                                                # warm-up: code objects, buffers
    seen = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fns in legs.items():
            seen[k].append(ms_per_call(fns, reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in seen.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from thermompnn_amd import _lib
    from thermompnn_amd.weights import synthetic_state_dict
    lib = _lib.load()
    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        res, args = _lib.SIGNATURES["tmpnn_seqloss_backward"]
        parent.tmpnn_seqloss_backward.restype, parent.tmpnn_seqloss_backward.argtypes = res, args
    slab = torch.cat([v.reshape(-1).float() for v in synthetic_state_dict(0, "mpnn").values()]).cuda()
    rng = np.random.default_rng(0)
    short = [protein(int(L), 1000 + i) for i, L in enumerate(rng.integers(40, 73, 64))]
    sets = {"L40_72": (short, 2), "L256": ([protein(256, 5256)], 10), "L1024": ([protein(1024, 6024)], 3)}
    out = {"metric": "coordgrad_backward", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "unit": "ms per backward call: median over rounds of the mean, with the rounds' min and max"}
    for name, (prots, reps) in sets.items():
        calls = [Single(lib, slab, p, parent) for p in prots]
        legs = {"backward": [c.plain for c in calls], "backward_x": [c.with_x for c in calls]}
        if parent is not None:
            legs["parent_backward"] = [c.parent_plain for c in calls]
        r = alternated(legs, a.rounds, reps)
        r["x_over_plain"] = round(r["backward_x"]["median_ms"] / r["backward"]["median_ms"], 4)
        if parent is not None:
            r["plain_over_parent"] = round(r["backward"]["median_ms"] / r["parent_backward"]["median_ms"], 4)
        out[name] = dict(proteins=len(prots), **r)
        del calls
    pk = Packed(lib, slab, short)
    r = alternated({"backward": [pk.plain], "backward_x": [pk.with_x]}, a.rounds, 3)
    r["x_over_plain"] = round(r["backward_x"]["median_ms"] / r["backward"]["median_ms"], 4)
    out["packed_64_L40_72"] = dict(proteins=pk.n, rows=pk.T, K=pk.K, **r)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
