"""What superposing ensemble members costs: one run on one box, the legs alternated in one process, medians of --rounds rounds
(default 5) with the rounds' min and max, device events.

Workloads: (equal) the ensemble bench's shape, E = 16 ensembles x M = 16 members x L = 256, every member its ensemble's synthetic
backbone with N(0, 0.25 A) jitter, turned and shifted as a rigid body, through the identity map; (ragged) the align bench's members
(staggered terminal deletions and one internal one, lengths 231 .. 255) turned and shifted the same way, through the row map
tmpnn_align_global writes.
 (a) the two launches alone (the C entry on buffers made once), both workloads, and split by launch with the library's event timers;
 (b) Engine.superpose as called (descriptor upload and output allocation included), both workloads;
 (c) the same results of the equal workload by batched torch.linalg.svd in float64 on the device (centroids, covariance, Kabsch with the
     determinant correction, residuals, per-column RMSF), and its largest differences from the kernel's;
 (d) the packed forward the superposition precedes, both workloads;
 (e) one ensemble of M = 4 096 members of L = 256: launch 2 loops 4 096 times per thread, twice; split by launch;
 (f) with --headline FILE: the JSON lines of `python bench.py --gpus 1 --steps 50 --warmup 20` in this tree and in a checkout of the
     parent commit, alternated, three runs each ({"tree": "this" | "parent", ...bench.py's line} per line).
Also `kernel_resources`: registers, scratch, LDS and occupancy of the two kernels as hipcc's -Rpass-analysis=kernel-resource-usage
reports them with the flags of the shipped build (needs hipcc, no GPU; --add-resources FILE writes them into an existing result file
and does nothing else).

    python tools/superpose_bench.py [--rounds 5] [--headline FILE] [--out profiles/superpose_bench.json] [--add-resources FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, M, L = 16, 16, 256
BIG_M = 4096


def rotation(rng):
    w, x, y, z = (q := rng.standard_normal(4)) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def turn(X, sizes, rng):
    """Every member (``sizes`` rows each, in order) of the packed [T, 4, 3] backbone turned and shifted as a rigid body, in place."""
    at = 0
    for n in sizes:
        X[at:at + n] = X[at:at + n] @ rotation(rng).T + rng.standard_normal(3) * 30.0
        at += n
    return X


def equal_batch(device, members=M, ensembles=E):
    from thermompnn_amd.synthetic import synthetic_backbone
    rng = np.random.default_rng(0)
    xs, ss = [], []
    for e in range(ensembles):
        X0, seq = synthetic_backbone(L, e)
        code = np.array(["ACDEFGHIKLMNPQRSTVWY".index(c) for c in seq], np.int32)
        xs.append(X0[None] + rng.normal(0.0, 0.25, size=(members,) + X0.shape))
        ss.append(np.tile(code, members))
    X = turn(np.concatenate(xs).reshape(-1, 4, 3), [L] * (ensembles * members), rng)
    T = X.shape[0]
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=device)
    return dict(X=t(X, torch.float32), S=t(np.concatenate(ss), torch.int32), mask=torch.ones(T, device=device),
                ridx=t(np.tile(np.arange(L), ensembles * members), torch.int32), cenc=torch.ones(T, dtype=torch.int32, device=device),
                offsets=t(np.arange(ensembles * members + 1) * L, torch.int32), T=T, max_len=L)


def kernel_resources():
    from thermompnn_amd import build
    src = "tmpnn_superpose.hip"
    cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(src, build.DEVICE_FLAGS), "--offload-device-only", "-c", os.path.join(build.CSRC, src),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = {"_Z14sup_fit_kernel7SupArgs": "sup_fit_kernel", "_Z14sup_col_kernel7SupArgs": "sup_col_kernel"}.get(m.group(1), m.group(1))
            out[name] = {"symbol": m.group(1)}
        m = re.search(r"\s(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def kernel_ms(lib, f, n=10):
    """Average milliseconds per launch of every kernel ``f`` launches, from the library's event timers."""
    f()
    torch.cuda.synchronize()
    lib.tmpnn_profile_enable(1)
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    cap = 64
    names, ms, cnt = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    k = lib.tmpnn_profile_fetch(names, ms, cnt, cap)
    lib.tmpnn_profile_enable(0)
    return {names[i].decode(): round(ms[i] / cnt[i], 5) for i in range(k)}


def svd_superpose(X, members, ensembles):
    """The equal workload's results by batched torch.linalg.svd, float64 on the device: every row valid, fit_to = 0, identity map."""
    P = X[:, 1].double().view(ensembles, members, L, 3)
    F = P[:, :1]
    cm, cf = P.mean(dim=2, keepdim=True), F.mean(dim=2, keepdim=True)
    S = torch.einsum("emla,emlb->emab", P - cm, (F - cf).expand_as(P))
    U, _, Vh = torch.linalg.svd(S)
    V = Vh.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(-1, -2)))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1))
    R = V @ D @ U.transpose(-1, -2)
    t = cf.squeeze(2) - torch.einsum("emab,emb->ema", R, cm.squeeze(2))
    moved = torch.einsum("emab,emlb->emla", R, P) + t[:, :, None]
    dev = (moved - F).norm(dim=-1)
    rmsd = dev.pow(2).mean(dim=-1).sqrt()
    mu = moved.mean(dim=1, keepdim=True)
    rmsf = (moved - mu).pow(2).sum(dim=-1).mean(dim=1).sqrt()
    return dict(rmsd=rmsd.reshape(-1).float(), dev=dev.reshape(-1).float(), rmsf=rmsf.reshape(-1).float(), R=R.reshape(-1, 9))


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
    import align_bench
    from hits_bench import alternated, ms_per_call
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import Engine, _ptr, _stream
    from thermompnn_amd.weights import synthetic_state_dict
    dev = "cuda:0"
    eng = Engine(synthetic_state_dict(0), dev, 48, precision="f16x2")
    lib = eng.lib
    out = {"metric": "superpose", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}

    def raw_call(X, mask, rows, members, lengths):
        """-> (a closure that makes the two launches on buffers made once, its outputs)."""
        Mv, Lv = np.asarray(members, np.int64), np.asarray(lengths, np.int64)
        map0, mem0, out0 = (np.concatenate([[0], np.cumsum(v)])[:-1] for v in (Mv * Lv, Mv, Lv))
        desc = torch.from_numpy(np.stack([map0, Mv, Lv, out0, mem0, np.zeros_like(Mv)], 1).astype(np.int32)).to(dev)
        R, NM, T_out = int((Mv * Lv).sum()), int(Mv.sum()), int(Lv.sum())
        shape = dict(n_fit=(NM,), rmsd=(NM,), xform=(NM, 12), dev=(R,), rmsf=(T_out,), col_count=(T_out,))
        res = {name: torch.empty(shape[name], dtype=getattr(torch, dt), device=dev) for name, dt in _lib.SUP_ARRAYS}
        status = torch.zeros(len(Mv), dtype=torch.int32, device=dev)

        def call():
            rc = lib.tmpnn_superpose(_ptr(X), _ptr(mask), _ptr(rows), R, _ptr(desc), len(Mv), X.shape[0], NM, T_out, int(Lv.max()),
                                     *[_ptr(res[name]) for name, _ in _lib.SUP_ARRAYS], _ptr(status), _stream())
            assert rc == 0, rc
        return call, res, status

    # the equal workload
    eq = equal_batch(dev)
    eq_raw, eq_res, eq_status = raw_call(eq["X"], eq["mask"], None, [M] * E, [L] * E)
    eq_eng = lambda: eng.superpose(eq["X"], eq["mask"], [M] * E, [L] * E)
    eq_svd = lambda: svd_superpose(eq["X"], M, E)
    table = torch.empty((eq["T"], 21), dtype=torch.float32, device=dev)
    eq_fwd = lambda: eng.ssm_forward(eq["X"], eq["S"], eq["mask"], eq["ridx"], eq["cenc"], eq["offsets"], max_len=L, out={"ddg": table},
                                     check_status=False)
    eq_raw()
    torch.cuda.synchronize()
    assert int(eq_status.abs().sum()) == 0
    svd = eq_svd()
    diff = {k: float((eq_res[k].double() - svd[k].double()).abs().max()) for k in ("rmsd", "dev", "rmsf")}
    diff["R"] = float((eq_res["xform"][:, :9] - svd["R"]).abs().max())
    eq_fwd()
    eng.check_last_status()
    # the ragged workload, through the map align_global writes
    rb, A, B, pair_desc, lens, _ = align_bench.build(dev)
    turned = turn(rb["X"].cpu().numpy().astype(np.float64), lens, np.random.default_rng(1))
    rb["X"] = torch.tensor(turned, dtype=torch.float32, device=dev)
    rows = eng.align_global(A, B, pair_desc)["out"]
    rg_raw, rg_res, rg_status = raw_call(rb["X"], rb["mask"], rows, [M] * E, [L] * E)
    rg_eng = lambda: eng.superpose(rb["X"], rb["mask"], [M] * E, [L] * E, rows=rows)
    rtable = torch.empty((rb["T"], 21), dtype=torch.float32, device=dev)
    rg_fwd = lambda: eng.ssm_forward(rb["X"], rb["S"], rb["mask"], rb["ridx"], rb["cenc"], rb["offsets"], max_len=rb["max_len"],
                                     out={"ddg": rtable}, check_status=False)
    rg_raw()
    torch.cuda.synchronize()
    assert int(rg_status.abs().sum()) == 0
    rg_fwd()
    eng.check_last_status()
    legs = {"equal_two_launches_only": eq_raw, "equal_engine_call": eq_eng, "equal_torch_svd_float64": eq_svd, "equal_packed_forward": eq_fwd,
            "ragged_two_launches_only": rg_raw, "ragged_engine_call": rg_eng, "ragged_packed_forward": rg_fwd}
    ra = alternated(legs, a.rounds, lambda fn, warm: ms_per_call(fn, 2 if warm else 10))
    out["ensembles_16x16x256"] = dict(
        workload=f"{E} ensembles x {M} members x L = {L}: equal (identity map, T = {eq['T']}) and ragged (lengths {min(lens)} .. {max(lens)}, "
                 f"the map of align_global, T = {rb['T']})", unit="ms per call (device events, 10 calls)", **ra,
        equal_by_launch_ms=kernel_ms(lib, eq_raw), ragged_by_launch_ms=kernel_ms(lib, rg_raw),
        largest_difference_from_torch_svd=diff, rmsd_range_equal=[float(eq_res["rmsd"].min()), float(eq_res["rmsd"].max())],
        n_fit_range_ragged=[int(rg_res["n_fit"].min()), int(rg_res["n_fit"].max())],
        launches_over_forward_equal=round(ra["equal_two_launches_only"]["median"] / ra["equal_packed_forward"]["median"], 5),
        launches_over_forward_ragged=round(ra["ragged_two_launches_only"]["median"] / ra["ragged_packed_forward"]["median"], 5),
        svd_over_launches_equal=round(ra["equal_torch_svd_float64"]["median"] / ra["equal_two_launches_only"]["median"], 2))
    # one ensemble of 4 096 members
    big = equal_batch(dev, members=BIG_M, ensembles=1)
    big_raw, big_res, big_status = raw_call(big["X"], big["mask"], None, [BIG_M], [L])
    big_raw()
    torch.cuda.synchronize()
    assert int(big_status.abs().sum()) == 0
    rbig = alternated({"one_ensemble_4096_members_two_launches": big_raw}, a.rounds, lambda fn, warm: ms_per_call(fn, 1 if warm else 5))
    out["one_ensemble_4096x256"] = dict(workload=f"one ensemble of {BIG_M} members of L = {L}, T = {big['T']} rows", unit="ms per call (device events, 5 calls)",
                                        **rbig, by_launch_ms=kernel_ms(lib, big_raw, 5),
                                        note="launch 2 is one thread per column: 256 threads, each looping over the 4 096 members twice")
    if a.headline:
        runs = [json.loads(ln) for ln in open(a.headline) if ln.strip().startswith("{")]
        runs = [{"tree": r["tree"], "preds_per_s": round(r["value"]), "ms_per_step": round(r["ms_per_step"], 4)} for r in runs]
        out["headline_bench_py"] = dict(what="python bench.py --gpus 1 --steps 50 --warmup 20 in a checkout of the parent commit and in this tree, "
                                             "alternated, one process per run, one box", runs=runs,
                                        preds_per_s_range={t: [min(r["preds_per_s"] for r in runs if r["tree"] == t),
                                                               max(r["preds_per_s"] for r in runs if r["tree"] == t)] for t in ("parent", "this")})
    out["kernel_resources"] = kernel_resources()
    out["not_measured"] = ["other E / M / L", "the command line end to end (parsing and featurizing on the host)", "multi-GPU",
                           "many ensembles of thousands of members", "a two-level fold of launch 2 (not built)"] + \
                          ([] if a.headline else ["bench.py against the parent commit"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
