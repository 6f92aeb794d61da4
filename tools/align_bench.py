"""What aligning ensemble members of unequal length costs: one run on one box, the legs alternated in one process, medians of --rounds
rounds (default 5) with the rounds' min and max, device events.

Workload: E = 16 ensembles x M = 16 members. Member m of an ensemble is its 256-residue synthetic backbone (N(0, 0.25 A) jitter)
without (3 m) % 13 residues at the N terminus, (5 m) % 13 at the C terminus (staggered terminal deletions of 0 - 12) and one internal
residue (at 60 + 7 m); the axis is the full sequence. 256 pairs of (256, 231 .. 255) codes.
 (a) the align_global launch alone (the C entry on buffers made once) and Engine.align_global; datasets.global_alignment_map on the
     host for the pairs of ONE ensemble (16 of the 256 pairs, time.perf_counter, once per round), scaled by 16.
 (b) Engine.ensemble_stats with identity rows against the plain entry, on one table of E x M x 256 rows (standard normal values).
 (c) the packed forward of the ragged members alone; the same forward + align_global + ensemble_stats(rows=): the whole aligned scan
     at the engine (parsing and featurizing files on the host is not in either leg).
 (d) one 8192 x 8192 pair over a two-letter alphabet: the worst case of one call.
 (e) with --headline FILE: the JSON lines of `python bench.py --gpus 1 --steps 50 --warmup 20` in this tree and in a checkout of the
     parent commit, alternated, three runs each ({"tree": "this" | "parent", ...bench.py's line} per line): preds/s and ms per step.

Also `kernel_resources`: registers, scratch, static LDS and occupancy of the alignment kernel and of both forms of the statistics
kernel as hipcc's -Rpass-analysis=kernel-resource-usage reports them with the flags of the shipped build (needs hipcc, no GPU;
--add-resources FILE writes them into an existing result file and does nothing else).

    python tools/align_bench.py [--rounds 5] [--headline FILE] [--out profiles/align_bench.json] [--add-resources FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, M, L = 16, 16, 256
LETTERS = "ACDEFGHIKLMNPQRSTVWY"


def build(device):
    """-> (ragged packed batch of the E * M members, axis codes [E * L], member codes, pair descriptors, member lengths)."""
    from thermompnn_amd.synthetic import synthetic_backbone
    rng = np.random.default_rng(0)
    xs, ss, ridx, lens, axes, seqs = [], [], [], [], [], []
    for e in range(E):
        X0, seq = synthetic_backbone(L, e)
        code = np.array([LETTERS.index(c) for c in seq], np.int32)
        axes.append(code)
        for m in range(M):
            keep = np.ones(L, bool)
            keep[:(3 * m) % 13] = False
            keep[L - (5 * m) % 13:] = False
            keep[60 + 7 * m] = False
            xs.append((X0 + rng.normal(0.0, 0.25, size=X0.shape))[keep])
            ss.append(code[keep])
            seqs.append("".join(np.array(list(seq))[keep]))
            ridx.append(np.arange(int(keep.sum())))
            lens.append(int(keep.sum()))
    T = sum(lens)
    starts = np.concatenate([[0], np.cumsum(lens)])
    desc = [(e * L, L, starts[e * M + m], lens[e * M + m], (e * M + m) * L, starts[e * M + m]) for e in range(E) for m in range(M)]
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=device)
    batch = dict(X=t(np.concatenate(xs), torch.float32), S=t(np.concatenate(ss), torch.int32), mask=torch.ones(T, device=device),
                 ridx=t(np.concatenate(ridx), torch.int32), cenc=torch.ones(T, dtype=torch.int32, device=device),
                 offsets=t(starts, torch.int32), T=T, max_len=max(lens))
    return batch, np.concatenate(axes), np.concatenate(ss), np.array(desc, np.int64), lens, seqs


def kernel_resources():
    from thermompnn_amd import build
    out = {}
    for src in ("tmpnn_align.hip", "tmpnn_ensemble.hip"):
        cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(src, build.DEVICE_FLAGS), "--offload-device-only", "-c", os.path.join(build.CSRC, src),
               "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        name = None
        for line in r.stdout.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = {"_Z12align_kernel9AlignArgs": "align_kernel", "_Z16ens_stats_kernelILb0EEv7EnsArgs": "ens_stats_kernel_plain",
                        "_Z16ens_stats_kernelILb1EEv7EnsArgs": "ens_stats_kernel_rows"}.get(m.group(1), m.group(1))
                out[name] = {"symbol": m.group(1)}
            m = re.search(r"\s(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                out[name][m.group(1)] = int(m.group(2))
    out["note"] = ("LDS Size is the static part; align_kernel adds 3 * 2 * (max_n + 2) + max_n + max_m bytes of dynamic LDS per workgroup of 1024 "
                   "threads: 2 060 bytes at 256 x 256, 65 548 at 8192 x 8192 (160 KB per CU)")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--add-resources", default=None, metavar="FILE")
    a = ap.parse_args(argv)
    if a.add_resources:
        d = json.load(open(a.add_resources))
        d["kernel_resources"] = kernel_resources()
        with open(a.add_resources, "w") as fh:
            json.dump(d, fh, indent=1)
            fh.write("\n")
        return
    from hits_bench import alternated, ms_per_call
    from thermompnn_amd import _lib
    from thermompnn_amd.datasets import global_alignment_map
    from thermompnn_amd.engine import Engine, _ptr, _stream
    from thermompnn_amd.synthetic import synthetic_backbone
    from thermompnn_amd.weights import synthetic_state_dict
    dev = "cuda:0"
    eng = Engine(synthetic_state_dict(0), dev, 48, precision="f16x2")
    out = {"metric": "align_global", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}
    b, A, B, desc, lens, seqs = build(dev)
    T, P = b["T"], E * M
    # (a) the launch alone, the engine call, the host function on one ensemble's pairs
    dA, dB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    ddesc = torch.from_numpy(desc.astype(np.int32)).to(dev)
    rows = torch.full((P * L,), -1, dtype=torch.int32, device=dev)
    aligned, status = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    ws = torch.empty(eng.lib.tmpnn_align_workspace_bytes(L, L, P), dtype=torch.uint8, device=dev)

    def align_raw():
        rc = eng.lib.tmpnn_align_global(_ptr(dA), dA.numel(), _ptr(dB), dB.numel(), _ptr(ddesc), P, L, L, _ptr(rows), rows.numel(), _ptr(aligned),
                                        _ptr(status), _ptr(ws), ws.numel(), _stream())
        assert rc == 0, rc

    align_eng = lambda: eng.align_global(dA, dB, desc, out=rows)
    axis0 = synthetic_backbone(L, 0)[1]
    host_ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        maps = [global_alignment_map(axis0, seqs[m]) for m in range(M)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    align_raw()
    torch.cuda.synchronize()
    got = rows[:M * L].view(M, L).cpu().numpy()
    local = np.where(got >= 0, got - desc[:M, 5][:, None], -1)                       # (add = the member's first table row)
    same = all([(-1 if j is None else j) for j in maps[m]] == local[m].tolist() for m in range(M))
    assert int(status.abs().sum()) == 0
    # (b) statistics through identity rows against the plain entry
    eq_table = torch.randn((E * M * L, 21), device=dev)
    S_eq = np.tile(A.reshape(E, 1, L), (1, M, 1)).reshape(-1)
    ident = torch.arange(E * M * L, dtype=torch.int32, device=dev)
    stats_plain = lambda: eng.ensemble_stats(eq_table, S_eq, [M] * E, [L] * E, cutoff=-0.5)
    stats_rows = lambda: eng.ensemble_stats(eq_table, S_eq, [M] * E, [L] * E, cutoff=-0.5, rows=ident)
    p_, r_ = stats_plain(), stats_rows()
    same_bits = all(torch.equal(p_[k].view(torch.int32), r_[k].view(torch.int32)) for k, _ in _lib.ENS_ARRAYS)
    # (c) the ragged forward alone, and with the alignment and the statistics behind it
    table = torch.empty((T, 21), dtype=torch.float32, device=dev)
    fwd = lambda: eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], max_len=b["max_len"], out={"ddg": table},
                                  check_status=False)
    fwd()
    eng.check_last_status()
    S_host = B

    def scan():
        fwd()
        al = eng.align_global(dA, dB, desc, out=rows)
        return eng.ensemble_stats(table, S_host, [M] * E, [L] * E, cutoff=-0.5, rows=al["out"])

    legs = {"align_global_launch_only": align_raw, "align_global_engine_call": align_eng, "ensemble_stats_plain": stats_plain,
            "ensemble_stats_identity_rows": stats_rows, "packed_forward_ragged": fwd, "forward_plus_align_plus_stats_rows": scan}
    ra = alternated(legs, a.rounds, lambda fn, warm: ms_per_call(fn, 2 if warm else 10))
    count = scan()["count"]
    host = {"median": round(statistics.median(host_ms) * E, 3), "min": round(min(host_ms) * E, 3), "max": round(max(host_ms) * E, 3)}
    f = ra["packed_forward_ragged"]["median"]
    out["aligned_ensembles"] = dict(
        workload=f"{E} ensembles x {M} members, lengths {min(lens)} .. {max(lens)} of {L}: {P} pairs, T = {T} rows", unit="ms per call (device events, 10 calls)",
        **ra, host_global_alignment_map_256_pairs_ms=host,
        host_note=f"datasets.global_alignment_map timed on the {M} pairs of ensemble 0 (perf_counter, once per round) and multiplied by {E}",
        host_over_launch=round(host["median"] / ra["align_global_launch_only"]["median"], 1), device_equals_host_on_ensemble_0=bool(same),
        identity_rows_same_bits_as_plain=bool(same_bits), align_launch_over_forward=round(ra["align_global_launch_only"]["median"] / f, 5),
        scan_over_forward=round(ra["forward_plus_align_plus_stats_rows"]["median"] / f, 5),
        columns_with_all_members=int((count[:, 0] == M).sum()), columns=int(count.shape[0]))
    # (d) the worst case of one call
    n = _lib.ALIGN_MAX_LEN
    rng = np.random.default_rng(1)
    a8, b8 = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).to(dev), torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).to(dev)
    out8 = torch.empty(n, dtype=torch.int32, device=dev)
    big = lambda: eng.align_global(a8, b8, [(0, n, 0, n, 0, 0)], out=out8)
    rb = alternated({"one_pair_8192_x_8192": big}, a.rounds, lambda fn, warm: ms_per_call(fn, 1 if warm else 3))
    out["worst_case"] = dict(workload="one pair of 8192 x 8192 codes over two letters: 67 108 864 cells on one workgroup", unit="ms per call (device events, 3 calls)",
                             **rb, workspace_bytes=int(eng.lib.tmpnn_align_workspace_bytes(n, n, 1)))
    if a.headline:
        runs = [json.loads(ln) for ln in open(a.headline) if ln.strip().startswith("{")]
        runs = [{"tree": r["tree"], "preds_per_s": round(r["value"]), "ms_per_step": round(r["ms_per_step"], 4)} for r in runs]
        out["headline_bench_py"] = dict(what="python bench.py --gpus 1 --steps 50 --warmup 20 in a checkout of the parent commit and in this tree, "
                                             "alternated, one process per run, one box", runs=runs,
                                        preds_per_s_range={t: [min(r["preds_per_s"] for r in runs if r["tree"] == t),
                                                               max(r["preds_per_s"] for r in runs if r["tree"] == t)] for t in ("parent", "this")})
    out["kernel_resources"] = kernel_resources()
    out["not_measured"] = ["other E / M / lengths", "the command line end to end (parsing and featurizing on the host)", "multi-GPU",
                           "bf16x3 and fp32 forwards", "many long pairs in one call"] + ([] if a.headline else ["bench.py against the parent commit"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
