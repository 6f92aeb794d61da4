"""What the bootstrap of the benchmark metrics costs: one run on one box, the legs alternated in one process, medians of --rounds
rounds (default 5) with the rounds' min and max, device events, one untimed pass of every leg first.

Sizes, M = 1 prediction column: (N, B) = (669, 10 000) an S669-sized set, (8 192, 10 000), (262 144, 1 000) a Megascale-sized set.
 (a) bootstrap.bootstrap_metrics as called: the upload, torch.unique, the draws in blocks, the launches, the copies back.
 (b) the launch alone (the C entry on idx drawn once and buffers made once), all B resamples in one call.
 (c) torch.randint alone, in the blocks leg (a) draws.
 (d) the reference's loop shape in torch on the device with the same draws, per iteration: a gather of both columns, a sort-based
     tie-averaged rank of each (sort, run boundaries, a cumulative maximum / minimum: torchmetrics is not installed, so its rank is
     restated without its Python loop over ties), the five metrics, one copy back. Run on --loop-iters iterations (default 40) and
     SCALED to B: ms = measured * B / iterations. That is stated in the output.
Per form also: the bytes and the LDS operations per resample computed from the shapes, and the kernel's registers, LDS and occupancy
as hipcc's -Rpass-analysis=kernel-resource-usage reports them for csrc/tmpnn_bootstrap.hip.

    python tools/bootstrap_bench.py [--rounds 5] [--loop-iters 40] [--out profiles/bootstrap_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = ((669, 10000), (8192, 10000), (262144, 1000))


def dataset(N):
    rng = np.random.default_rng(N)
    raw = rng.normal(-0.7, 1.5, N)
    truth = (np.round(raw * 20) / 20).astype(np.float32)                   # measured ddG: two decimals' worth of ties
    pred = (0.6 * raw + rng.normal(0.0, 1.0, N)).astype(np.float32)       # predictions: hardly any ties
    return pred, truth


def torch_rank(x):
    """1-based tie-averaged ranks by one sort"""
    n = x.numel()
    s, order = torch.sort(x)
    pos = torch.arange(n, device=x.device)
    start = torch.ones(n, dtype=torch.bool, device=x.device)
    start[1:] = s[1:] != s[:-1]
    end = torch.ones(n, dtype=torch.bool, device=x.device)
    end[:-1] = start[1:]
    first = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0)[0]
    last = torch.flip(torch.cummin(torch.flip(torch.where(end, pos, torch.full_like(pos, n)), [0]), 0)[0], [0])
    r = torch.empty(n, dtype=torch.float64, device=x.device)
    r[order] = 0.5 * (first + last).double() + 1.0
    return r


def torch_metrics(p, t):
    p, t = p.double(), t.double()
    def corr(a, b):
        ac, bc = a - a.mean(), b - b.mean()
        return (ac * bc).sum() / torch.sqrt((ac * ac).sum() * (bc * bc).sum())
    see = ((p - t) ** 2).sum()
    mse = see / p.numel()
    return torch.stack([1.0 - see / ((t - t.mean()) ** 2).sum(), mse, mse.sqrt(), corr(torch_rank(p), torch_rank(t)), corr(p, t)])


def model(N, M, lds):
    """bytes and array operations of ONE resample, from the shapes (the kernel's passes, csrc/tmpnn_bootstrap.hip)"""
    npad = (N + 3) & ~3
    cols = 1 + M
    idx_bytes = 4 * N * (1 + 2 * M)                                       # the row is read once per pass
    gathers = 4 * N * (2 * cols + 4 * M)                                   # gid + value per count pass; two of each in a column's last pass
    bins = dict(zero_words=npad * cols, atomic_adds=N * cols, scan_b128_loads=npad // 4 * cols, scan_b128_stores=npad // 4 * cols,
                x_gathers=2 * N * M)
    out = dict(idx_bytes_read=idx_bytes, gathered_bytes=gathers, output_bytes=M * 64 + 4)
    out["lds_operations" if lds else "workspace_operations"] = bins
    if not lds:
        out["workspace_bytes_moved"] = 4 * (bins["zero_words"] + bins["atomic_adds"] + bins["x_gathers"]) + 32 * bins["scan_b128_loads"]
    return out


def kernel_resources():
    from thermompnn_amd import build
    src = os.path.join(build.CSRC, "tmpnn_bootstrap.hip")
    cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS["tmpnn_bootstrap.hip"], "--offload-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = "lds_form" if "ILb1E" in m.group(1) else "workspace_form"
            out[name] = {"symbol": m.group(1)}
        m = re.search(r"\s(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    out["note"] = ("LDS Size is the static part; the LDS form adds 2 * 4 * N bytes of dynamic LDS per workgroup of 1024 threads, which bounds "
                   "the workgroups per CU at larger N (160 KB per CU)")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from hits_bench import alternated, ms_per_call
    from thermompnn_amd import _lib
    from thermompnn_amd.bootstrap import bootstrap_metrics, bootstrap_stats, default_draw_block, dense_rank, draw_blocks
    dev = "cuda:0"
    out = {"metric": "bootstrap_metrics", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "M": 1,
           "unit": "ms per call, median over rounds with the rounds' min and max; legs alternated inside every round, one process",
           "lds_form_up_to_N": _lib.BOOT_LDS_N, "sizes": {}}
    for N, B in SIZES:
        pred, truth = dataset(N)
        v = torch.from_numpy(np.stack([truth, pred])).to(dev)
        gid = dense_rank(v)
        idx = torch.cat(list(draw_blocks(N, B, 0, dev)))
        bufs = dict(metrics=torch.empty((B, 1, 5), dtype=torch.float64, device=dev), ranks=torch.empty((B, 1, 3), dtype=torch.int64, device=dev),
                    status=torch.empty(B, dtype=torch.int32, device=dev))
        lds = N <= _lib.BOOT_LDS_N
        it = min(a.loop_iters, B)

        def loop():
            for b in range(it):
                row = idx[b].long()
                torch_metrics(v[1][row], v[0][row]).cpu()

        legs = {"a_bootstrap_metrics_as_called": lambda: bootstrap_metrics(pred, truth, B, seed=0),
                "b_launch_only": lambda: bootstrap_stats(v, gid, idx, out=bufs),
                "c_torch_randint_only": lambda: [None for _ in draw_blocks(N, B, 0, dev)],
                "d_torch_loop_subset": loop}
        if lds:
            legs["b_launch_only_forced_workspace_form"] = lambda: bootstrap_stats(v, gid, idx, force_workspace=True, out=bufs)
        r = alternated(legs, a.rounds, lambda fn, warm: ms_per_call(fn, 1 if warm else 3))
        scale = B / it
        d = r.pop("d_torch_loop_subset")
        r["d_torch_loop_scaled"] = {k: round(x * scale, 3) for k, x in d.items()}
        r["d_torch_loop_scaled"]["note"] = f"measured on {it} iterations ({d['median']} ms) and scaled by {scale:g} to B = {B}"
        # the two routes agree on the iterations the loop ran
        got = bootstrap_stats(v, gid, idx[:it])[0][:, 0]
        ref = torch.stack([torch_metrics(v[1][idx[b].long()], v[0][idx[b].long()]) for b in range(it)])
        r["max_abs_difference_to_torch_loop"] = float((got - ref).abs().max())
        r["form"] = "lds" if lds else "workspace"
        r["draw_block"] = default_draw_block(N, B)
        r["idx_bytes"] = int(idx.numel() * 4)
        r["workspace_bytes"] = int(_lib.load().tmpnn_bootstrap_workspace_bytes(2, N, B, 0))
        r["per_resample_model"] = model(N, 1, lds)
        k, c = r["b_launch_only"]["median"], r["c_torch_randint_only"]["median"]
        r["launch_us_per_resample"] = round(k / B * 1e3, 3)
        r["draws_over_launch"] = round(c / k, 3)
        r["torch_loop_over_as_called"] = round(r["d_torch_loop_scaled"]["median"] / r["a_bootstrap_metrics_as_called"]["median"], 2)
        out["sizes"][f"N={N},B={B}"] = r
        del idx, bufs
        torch.cuda.empty_cache()
    out["kernel_resources"] = kernel_resources()
    out["not_measured"] = ["M > 1", "other N / B", "the command line end to end (CSV parsing and writing)", "torchmetrics itself (not installed)",
                           "the reference's pandas sampling and host-to-device copies per iteration"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
