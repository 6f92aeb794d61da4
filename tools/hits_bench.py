"""What the ranked hit lists cost: one run on one box, the legs alternated in one process, medians of --rounds rounds (default 5)
with the rounds' min and max.

 (a) selection: Engine.select_hits (k = 32) on the table of the bench batch (64 proteins x L = 256), against the fused forward of that
     batch and against torch.topk on the NaN-masked table padded to [P, Lmax * 20] (what a torch user would write: it gives values and
     flat indices, no tie order, no one-per-position form). Device events around `reps` calls.
 (b) end to end: the 1 024 files of tools/e2e_bench.py (bench.end_to_end's set) scanned to the hit CSV (--top 32), to the binary tables
     and to the full CSV, wall clock from the path list to the closed file. The binary and full-CSV routes are the parent commit's code
     unchanged (this change adds a branch in front of them), timed here in the same process.
 (c) headline: the fused forward of the bench batch through this library and, with --parent-lib PATH (a libtmpnn.so built from the
     parent commit), through the parent's, alternated: the forward must not move beyond the rounds' spread.

    python tools/hits_bench.py [--rounds 5] [--files 1024] [--parent-lib PATH] [--out profiles/hits_bench.json]

--lds-workload K: nothing is timed; the bench table is made by one forward and tmpnn_select_hits runs three times at that k — the
program of a counter run of its own, e.g.
    rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS --output-format csv -d OUT -o hits -- \
        python tools/hits_bench.py --lds-workload 32
(SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of hits_block_kernel and hits_merge_kernel = the share of LDS-array cycles lost to conflicts).
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ms_per_call(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternated(legs, rounds, measure):
    """legs: {name: callable} -> {name: {median, min, max}}; every round runs every leg once, in turn; one untimed pass first."""
    for fn in legs.values():
        measure(fn, True)
    seen = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            seen[k].append(measure(fn, False))
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in seen.items()}


class LibForward:
    """tmpnn_ssm_forward of one libtmpnn.so (this commit's, the parent commit's) on the same tensors, through ctypes alone: its own
    handle, packed buffer, workspace and status word, so that the two libraries' legs are made the same way."""

    def __init__(self, path, eng, batch, out):
        from thermompnn_amd import _lib
        from thermompnn_amd.engine import _ptr, _stream
        lib = C.CDLL(path)
        for name in ("tmpnn_weights_packed_bytes_p", "tmpnn_weights_create_p", "tmpnn_workspace_bytes", "tmpnn_ssm_forward"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        self.packed = torch.empty(lib.tmpnn_weights_packed_bytes_p(eng.precision.encode()), dtype=torch.uint8, device=eng.device)
        n = len(eng.w.tensors)
        arr = (C.c_void_p * n)(*[t.data_ptr() for t in eng.w.tensors])
        self.handle = C.c_void_p()
        rc = lib.tmpnn_weights_create_p(C.byref(self.handle), arr, n, _ptr(self.packed), self.packed.numel(), eng.precision.encode(), _stream())
        assert rc == 0, rc
        self.ws = torch.empty(lib.tmpnn_workspace_bytes(batch["T"]), dtype=torch.uint8, device=eng.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=eng.device)
        b = batch
        self.args = (self.handle, _ptr(b["X"]), _ptr(b["S"]), _ptr(b["mask"]), _ptr(b["ridx"]), _ptr(b["cenc"]), _ptr(b["offsets"]), b["n"],
                     b["T"], b["L"], eng.K, _ptr(out), None, None, None, _ptr(self.status), _ptr(self.ws), self.ws.numel())
        self.lib, self._stream = lib, _stream

    def __call__(self):
        rc = self.lib.tmpnn_ssm_forward(*self.args, self._stream())
        assert rc == 0, rc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lds-workload", type=int, default=None, metavar="K")
    a = ap.parse_args(argv)
    import bench
    from thermompnn_amd import ssm_scan
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    from thermompnn_amd.weights import synthetic_state_dict
    eng = Engine(synthetic_state_dict(0), "cuda:0", 48)
    out = {"metric": "hit_lists", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}

    # (a) + (c): the bench batch
    P, L, k = 64, 256, a.lds_workload or 32
    b = bench.build_batch(P, L, 0, "cuda:0")
    table = torch.empty((b["T"], 21), dtype=torch.float32, device="cuda:0")
    fwd = lambda: eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], max_len=L, out={"ddg": table}, check_status=False)
    fwd()
    eng.check_last_status()
    offs = np.arange(P + 1) * L
    sel = lambda: eng.select_hits(table, b["S"], offs, k)
    sel_one = lambda: eng.select_hits(table, b["S"], offs, k, one_per_position=True)
    own = torch.zeros((b["T"], 20), dtype=torch.bool, device="cuda:0")
    own[torch.arange(b["T"], device="cuda:0"), b["S"].long()] = True
    own[:, 1] = True                                                    # cysteine

    def topk():
        v = table[:, :20]
        masked = torch.where(own | torch.isnan(v), torch.full_like(v, float("inf")), v)
        return torch.topk(masked.reshape(P, L * 20), k, dim=1, largest=False)

    # the two launches alone (the C entry on buffers made once): Engine.select_hits adds the outputs' and the workspace's allocation
    # and the upload of the offsets
    from thermompnn_amd.engine import _ptr, _stream
    d_off = torch.as_tensor(offs).to("cuda:0", torch.int32)
    bufs = [torch.empty((P, k), dtype=dt, device="cuda:0") for dt in (torch.float32, torch.int32, torch.int32)] + \
           [torch.empty(P, dtype=torch.int32, device="cuda:0")]
    ws = torch.empty(eng.lib.tmpnn_hits_workspace_bytes(b["T"], P, k), dtype=torch.uint8, device="cuda:0")

    def sel_raw():
        rc = eng.lib.tmpnn_select_hits(_ptr(table), 21, _ptr(b["S"]), _ptr(d_off), P, b["T"], k, float("inf"), 0, *[_ptr(t) for t in bufs],
                                       _ptr(ws), ws.numel(), _stream())
        assert rc == 0, rc

    if a.lds_workload:
        for _ in range(3):
            sel_raw()
        torch.cuda.synchronize()
        return
    legs = {"fused_forward": fwd, "select_hits_k32": sel, "select_hits_k32_launches_only": sel_raw,
            "select_hits_k32_one_per_position": sel_one, "torch_topk_k32": topk}
    parent = None
    if a.parent_lib:
        from thermompnn_amd import _lib
        this_out, parent_out = torch.empty_like(table), torch.empty_like(table)
        parent = LibForward(a.parent_lib, eng, b, parent_out)
        legs["headline_this_library"] = this = LibForward(_lib.LIB_PATH, eng, b, this_out)
        legs["headline_parent_library"] = parent
    ra = alternated(legs, a.rounds, lambda fn, warm: ms_per_call(fn, 3 if warm else 30))
    out["selection"] = dict(workload=f"{P} proteins x L = {L}: {P * L * 20} predictions, k = {k}", unit="ms per call (device events, 30 calls)", **ra)
    out["selection"]["select_over_forward"] = round(ra["select_hits_k32"]["median"] / ra["fused_forward"]["median"], 4)
    out["selection"]["launches_over_forward"] = round(ra["select_hits_k32_launches_only"]["median"] / ra["fused_forward"]["median"], 4)
    out["selection"]["select_over_topk"] = round(ra["select_hits_k32"]["median"] / ra["torch_topk_k32"]["median"], 4)
    if parent is not None:
        this()
        parent()
        torch.cuda.synchronize()
        t_ms, p_ms = ra["headline_this_library"]["median"], ra["headline_parent_library"]["median"]
        out["headline"] = {"this_over_parent": round(t_ms / p_ms, 4),
                           "same_bits": bool(torch.equal(this_out.view(torch.int32), parent_out.view(torch.int32))),
                           "preds_per_s_this": round(P * L * 20 / t_ms * 1e3), "preds_per_s_parent": round(P * L * 20 / p_ms * 1e3),
                           "note": "both legs call tmpnn_ssm_forward through ctypes with a handle, packed buffer and workspace of their own"}

    # (b) the many-file scan
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="tmpnn_hits_", dir=base)
    try:
        lens = np.random.default_rng(1).integers(64, 513, size=a.files)
        paths = []
        for i, n in enumerate(lens):
            X, seq = synthetic_backbone(int(n), 1000 + i)
            paths.append(os.path.join(d, f"syn_{i:04d}.pdb"))
            with open(paths[-1], "w") as fh:
                fh.write(backbone_pdb_text(X, seq))
        chains, T = ["A"] * a.files, int(lens.sum())
        sizes = {}

        def scan(name, **kw):
            def run():
                path = os.path.join(d, "out." + name)
                ssm_scan.scan_to_file(eng, paths, chains, path, include_cys=True, **kw)
                sizes[name] = os.path.getsize(path)
                os.remove(path)
            return run

        def wall(fn, warm):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        rb = alternated({"to_hit_csv_top32": scan("hits.csv", top=32), "to_npz": scan("npz"), "to_full_csv": scan("csv")}, a.rounds, wall)
        out["scan"] = dict(workload=f"{a.files} backbone-only PDB files on {'tmpfs' if base else 'the temp directory'}, {T} residues, "
                                    f"{20 * T} predictions; path list -> closed output file", unit="wall seconds",
                           output_bytes=sizes, **rb)
        for name in rb:
            out["scan"][name]["preds_per_s"] = round(20 * T / rb[name]["median"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out["not_measured"] = ["LDS bank conflicts (a counter run of its own: --lds-workload)", "k other than 32", "proteins above L = 512 in the scan",
                           "multi-GPU (the hit list is single rank)"] + ([] if a.parent_lib else ["the headline against the parent library"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
