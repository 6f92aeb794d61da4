#!/usr/bin/env python3
"""The C-alpha-only flavour beside the full-backbone one, on one GPU: 64 synthetic backbones of L = 256 and synthetic weights at
f16x2, medians of five alternated rounds in one process. Three legs, each with a CA handle and a full-backbone handle on the same
backbones (the CA handle reads only their C-alpha atoms):
  (a) the featurizer stage: ca_frames + the CA edge kernel (Engine.edge_featurize of a CA engine) against the full-backbone edge
      kernel, both on the k-NN graph computed once outside the timed region;
  (b) Engine.encode;
  (c) the fused forward with log_probs only (Engine.ssm_forward, check_status off).
Each timed call is ITERS launches back to back, the time divided by ITERS. Leg (a) is also split by launch: the library's per-kernel
event timers (tmpnn_profile_enable) around ca_frames, the CA edge kernel and the full-backbone edge kernel.
    python tools/ca_bench.py out.json [--rounds 5]
Recorded, not gated. One run on one box; the JSON keeps every round."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from thermompnn_amd.engine import Engine  # noqa: E402
from thermompnn_amd.synthetic import synthetic_backbone  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402

ITERS = 10


def timed(ways, rounds):
    """Alternated rounds of the callables -> (seconds per call and round, medians, spreads); one warm-up call each first."""
    for f in ways.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, f in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / ITERS)
    return {"seconds_per_call": times, "median_seconds": {k: statistics.median(v) for k, v in times.items()},
            "spread_seconds": {k: max(v) - min(v) for k, v in times.items()}}


def kernel_ms(lib, f, n=20):
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
    return {names[i].decode(): ms[i] / cnt[i] for i in range(k)}


def main():
    args = sys.argv[1:]
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    out_path = os.path.abspath(args[0])
    dev = torch.device("cuda:0")
    P, L = 64, 256
    full = Engine(synthetic_state_dict(0, "mpnn"), dev, 48, precision="f16x2", retry_precision=None)
    ca = Engine(synthetic_state_dict(0, "mpnn_ca"), dev, 48, precision="f16x2", retry_precision=None)
    X = torch.cat([torch.from_numpy(np.ascontiguousarray(synthetic_backbone(L, 100 + p)[0])).to(dev, torch.float32) for p in range(P)])
    T = P * L
    mask = torch.ones(T, device=dev)
    ridx = torch.arange(L, dtype=torch.int32, device=dev).repeat(P)
    cenc = torch.ones(T, dtype=torch.int32, device=dev)
    S = torch.zeros(T, dtype=torch.int32, device=dev)
    offsets = (torch.arange(P + 1, dtype=torch.int32) * L).to(dev)
    E_idx, D_nb = full.knn_topk(X, mask, offsets, max_len=L)
    legs = {
        "a_featurizer_stage": timed({"ca_frames_plus_ca_edge_kernel": lambda: ca.edge_featurize(X, ridx, cenc, E_idx, D_nb, offsets=offsets),
                                     "full_backbone_edge_kernel": lambda: full.edge_featurize(X, ridx, cenc, E_idx, D_nb)}, rounds),
        "b_encode": timed({"ca": lambda: ca.encode(X, mask, ridx, cenc, offsets, max_len=L),
                           "full_backbone": lambda: full.encode(X, mask, ridx, cenc, offsets, max_len=L)}, rounds),
        "c_forward_log_probs": timed({"ca": lambda: ca.ssm_forward(X, S, mask, ridx, cenc, offsets, max_len=L, want_ddg=False, want_log_probs=True,
                                                                   check_status=False),
                                      "full_backbone": lambda: full.ssm_forward(X, S, mask, ridx, cenc, offsets, max_len=L, want_ddg=False,
                                                                                want_log_probs=True, check_status=False)}, rounds),
    }
    legs["a_featurizer_stage"]["kernel_milliseconds_per_launch"] = {
        **kernel_ms(ca.lib, lambda: ca.edge_featurize(X, ridx, cenc, E_idx, D_nb, offsets=offsets)),
        **kernel_ms(full.lib, lambda: full.edge_featurize(X, ridx, cenc, E_idx, D_nb))}
    for leg in legs.values():
        m = leg["median_seconds"]
        a, b = list(m.values())[:2]
        leg["ca_over_full"] = a / b
        leg["difference_exceeds_the_spread"] = abs(a - b) > max(leg["spread_seconds"].values())
    res = {"workload": f"{P} synthetic backbones of L = {L} (T = {T}), synthetic weights, f16x2, K = 48", "device": torch.cuda.get_device_name(0),
           "rounds": rounds, "launches_per_timed_call": ITERS, **legs,
           "clock": "wall clock (time.perf_counter) around a synchronised device, one process, legs alternated; (a) and (b) allocate their "
                    "outputs inside the timed call, both flavours alike; (b) reads the status word back once per call"}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: {"median_seconds": v["median_seconds"], "ca_over_full": v["ca_over_full"]} for k, v in legs.items()}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
