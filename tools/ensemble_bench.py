"""What the statistics over conformer ensembles cost: one run on one box, the legs alternated in one process, medians of --rounds
rounds (default 5) with the rounds' min and max.

Workload: E = 16 ensembles x M = 16 members x L = 256 residues (T = 65 536 table rows, 1 310 720 predictions reduced to 16 x 256 x 20
entries of eight statistics), f16x2. A member is its ensemble's synthetic backbone with N(0, 0.25 A) jitter, the sequence shared.
 (a) the packed forward alone; the forward + Engine.ensemble_stats; the forward + the same eight reductions written in torch on the
     [E, M, L, 20] view (what a torch user would write: masked sums, min / max with indices; no order contract, no NaN canonical form).
     Device events around `reps` calls; peak device memory of every leg (torch's allocator, reset before the leg).
 (b) the stats launch alone (the C entry on buffers made once) by the same event timers.
 (c) headline: the fused forward of the bench batch (64 x 256) through this library and, with --parent-lib PATH (a libtmpnn.so built
     from the parent commit), through the parent's, alternated: the forward's sources are untouched, so the two should agree within
     the rounds' spread.

    python tools/ensemble_bench.py [--rounds 5] [--parent-lib PATH] [--out profiles/ensemble_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E, M, L = 16, 16, 256


def build_ensembles(device):
    from thermompnn_amd.synthetic import AA20, synthetic_backbone
    rng = np.random.default_rng(0)
    xs, ss = [], []
    for e in range(E):
        X0, seq = synthetic_backbone(L, e)
        for _ in range(M):
            xs.append(X0 + rng.normal(0.0, 0.25, size=X0.shape))
            ss.append([AA20.index(c) for c in seq])
    T = E * M * L
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=device)
    return dict(X=t(np.concatenate(xs), torch.float32), S=t(np.concatenate(ss), torch.int32), mask=torch.ones(T, device=device),
                ridx=t(np.tile(np.arange(L), E * M), torch.int32), cenc=torch.ones(T, dtype=torch.int32, device=device),
                offsets=t(np.arange(E * M + 1) * L, torch.int32), T=T, L=L, n=E * M)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import bench
    from hits_bench import LibForward, alternated, ms_per_call
    from thermompnn_amd import _lib
    from thermompnn_amd.engine import Engine, _ptr, _stream
    from thermompnn_amd.weights import synthetic_state_dict
    dev = "cuda:0"
    eng = Engine(synthetic_state_dict(0), dev, 48, precision="f16x2")
    out = {"metric": "ensemble_stats", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}
    b = build_ensembles(dev)
    T = b["T"]
    table = torch.empty((T, 21), dtype=torch.float32, device=dev)
    fwd = lambda: eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], max_len=L, out={"ddg": table}, check_status=False)
    fwd()
    eng.check_last_status()
    S_host = b["S"].cpu().numpy()
    members, lengths = [M] * E, [L] * E
    stats = lambda: eng.ensemble_stats(table, S_host, members, lengths, cutoff=-0.5)
    live = (b["S"] >= 0) & (b["S"] < 20)
    cut = torch.tensor(-0.5, device=dev)

    def torch_stats():
        v = table[:, :20].view(E, M, L, 20)
        ok = live.view(E, M, L, 1) & ~torch.isnan(v)
        n = ok.sum(1)
        mean = torch.where(ok, v, torch.zeros((), device=dev)).sum(1) / n
        d = torch.where(ok, v - mean[:, None], torch.zeros((), device=dev))
        spread = ((d * d).sum(1) / n).sqrt()
        lo, lo_m = torch.where(ok, v, torch.full((), float("inf"), device=dev)).min(1)
        hi, hi_m = torch.where(ok, v, torch.full((), float("-inf"), device=dev)).max(1)
        below = (ok & (v <= cut)).sum(1)
        return mean, spread, lo, hi, lo_m, hi_m, n, below

    # the launch alone: the C entry on buffers made once (Engine.ensemble_stats adds the outputs' allocation and two small uploads)
    desc = torch.tensor([[e * M * L, M, L, e * L] for e in range(E)], dtype=torch.int32, device=dev)
    bufs = [torch.empty((E * L, 20), dtype=getattr(torch, dt), device=dev) for _, dt in _lib.ENS_ARRAYS]
    status = torch.zeros(E, dtype=torch.int32, device=dev)

    def stats_raw():
        rc = eng.lib.tmpnn_ensemble_stats(_ptr(table), 21, _ptr(b["S"]), _ptr(desc), E, T, E * L, L, -0.5, *[_ptr(t) for t in bufs], _ptr(status),
                                          _stream())
        assert rc == 0, rc

    legs = {"packed_forward": fwd, "forward_plus_ensemble_stats": lambda: (fwd(), stats()),
            "forward_plus_torch_reductions": lambda: (fwd(), torch_stats()), "ensemble_stats_launch_only": stats_raw,
            "ensemble_stats_engine_call": stats, "torch_reductions_only": torch_stats}
    ra = alternated(legs, a.rounds, lambda fn, warm: ms_per_call(fn, 2 if warm else 10))
    peak = {}
    for name in ("packed_forward", "forward_plus_ensemble_stats", "forward_plus_torch_reductions"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        legs[name]()
        torch.cuda.synchronize()
        peak[name] = {"peak_bytes_above_resident": int(torch.cuda.max_memory_allocated() - base), "resident_bytes": int(base)}
    # the two routes agree where no order decides: counts, extremes and their members exactly, mean and spread to rounding
    got, ref = stats(), torch_stats()
    agree = {"count": bool(torch.equal(got["count"], ref[6].reshape(-1, 20).int())), "lo": bool(torch.equal(got["lo"], ref[2].reshape(-1, 20))),
             "hi": bool(torch.equal(got["hi"], ref[3].reshape(-1, 20))),
             "lo_member": bool(torch.equal(got["lo_member"], ref[4].reshape(-1, 20).int())),
             "below": bool(torch.equal(got["below"], ref[7].reshape(-1, 20).int())),
             "max_abs_mean_difference": float((got["mean"] - ref[0].reshape(-1, 20)).abs().max()),
             "max_abs_spread_difference": float((got["spread"] - ref[1].reshape(-1, 20)).abs().max())}
    f = ra["packed_forward"]["median"]
    out["ensembles"] = dict(workload=f"{E} ensembles x {M} members x L = {L}: T = {T} rows, {T * 20} predictions -> {E * L * 20} entries x 8",
                            unit="ms per call (device events, 10 calls)", **ra, peak_memory=peak, torch_agreement=agree,
                            stats_over_forward=round(ra["ensemble_stats_engine_call"]["median"] / f, 5),
                            launch_over_forward=round(ra["ensemble_stats_launch_only"]["median"] / f, 5),
                            torch_reductions_over_forward=round(ra["torch_reductions_only"]["median"] / f, 5),
                            table_bytes_read_per_pass=T * 20 * 4)
    if a.parent_lib:
        P = 64
        hb = bench.build_batch(P, L, 0, dev)
        this_out = torch.empty((hb["T"], 21), dtype=torch.float32, device=dev)
        parent_out = torch.empty_like(this_out)
        this, parent = LibForward(_lib.LIB_PATH, eng, hb, this_out), LibForward(a.parent_lib, eng, hb, parent_out)
        rh = alternated({"headline_this_library": this, "headline_parent_library": parent}, a.rounds,
                        lambda fn, warm: ms_per_call(fn, 3 if warm else 30))
        this()
        parent()
        torch.cuda.synchronize()
        t_ms, p_ms = rh["headline_this_library"]["median"], rh["headline_parent_library"]["median"]
        out["headline"] = dict(workload=f"{P} proteins x L = {L}, ms per forward (device events, 30 calls)", **rh,
                               this_over_parent=round(t_ms / p_ms, 4),
                               same_bits=bool(torch.equal(this_out.view(torch.int32), parent_out.view(torch.int32))),
                               preds_per_s_this=round(P * L * 20 / t_ms * 1e3), preds_per_s_parent=round(P * L * 20 / p_ms * 1e3),
                               note="both legs call tmpnn_ssm_forward through ctypes with a handle, packed buffer and workspace of their own")
    out["not_measured"] = ["other E / M / L", "multi-GPU (the reduction is single rank)", "bf16x3 and fp32 forwards", "the command line end to end"] + \
                          ([] if a.parent_lib else ["the headline against the parent library"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
