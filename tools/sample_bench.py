#!/usr/bin/env python3
"""Autoregressive sampling two ways, on one GPU: synthetic backbones and weights at f16x2, the two legs alternated in one process
(five rounds), at L = 128 with N = 64 chains and at L = 256 with N = 256 chains, every position free, temperature 1:
  (a) ONE Engine.sample call: the chains run whole inside one launch (tmpnn_sample);
  (b) what a caller had before it: L calls of Engine.decode_ordered on the partly filled sequences, each followed by the softmax of
      the step's rows and the same inverse-CDF rule in torch on the device, with the same uniforms.
Both legs start from the same encoded backbone (the encode is outside the timed region). Reported: every round, medians, spread
(max - min), and how many letters of the two legs' sequences agree (torch.cumsum need not add in index order, and the two decoders
sum in different orders: a draw within rounding of a boundary may differ, and everything decoded after it then may too).
    python tools/sample_bench.py out.json [--rounds 5]
Recorded, not gated. One run on one box; the JSON keeps every round."""
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


def one_size(eng, L, N, rounds):
    dev = eng.device
    Xn, _ = synthetic_backbone(L, 3)
    X = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev, torch.float32)
    mask = torch.ones(L, device=dev)
    ridx, cenc = torch.arange(L, dtype=torch.int32, device=dev), torch.ones(L, dtype=torch.int32, device=dev)
    off = torch.tensor([0, L], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(L)
    order = torch.argsort(torch.rand((N, L), device=dev, generator=gen), dim=1).to(torch.int32)
    steps = torch.arange(L, dtype=torch.int32, device=dev).expand(N, L).contiguous()
    ranks = torch.empty_like(order).scatter_(1, order.long(), steps)
    u = torch.rand((N, L), device=dev, generator=gen)
    S_fixed = torch.zeros((N, L), dtype=torch.int32, device=dev)
    free = torch.ones((N, L), device=dev)
    enc = eng.encode(X, mask, ridx, cenc, off, max_len=L)
    rows = torch.arange(N, device=dev)
    out = {}

    def one_launch():
        out["a"] = eng.sample(enc, order, S_fixed, free, u, check_status=False)["S"]

    def step_by_step():
        S = S_fixed.clone()
        for s in range(L):
            t = order[:, s].long()
            lp = eng.decode_ordered(enc, S, ranks, check_status=False)["log_probs"][rows, t]
            p = torch.softmax(lp, dim=-1)
            c = torch.cumsum(p, dim=-1)
            above = c > (u[rows, t] * c[:, -1])[:, None]
            last = 20 - torch.argmax((p > 0).flip(-1).to(torch.int32), dim=-1)
            S[rows, t] = torch.where(above.any(-1), torch.argmax(above.to(torch.int32), dim=-1), last).to(torch.int32)
        out["b"] = S

    ways = {"a_one_sample_call": one_launch, "b_L_decode_ordered_calls": step_by_step}
    for f in ways.values():                                          # warm-up
        f()
    torch.cuda.synchronize()
    same = float((out["a"] == out["b"]).float().mean())
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, f in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    return {"L": L, "N": N, "seconds_per_round": times, "median_seconds": med, "spread_seconds": spread,
            "b_minus_a_median_seconds": med["b_L_decode_ordered_calls"] - med["a_one_sample_call"],
            "a_beats_b_by_more_than_the_spread": med["b_L_decode_ordered_calls"] - med["a_one_sample_call"] > max(spread.values()),
            "fraction_of_letters_equal": same, "chains_equal": int((out["a"] == out["b"]).all(1).sum())}


def main():
    args = sys.argv[1:]
    opt = lambda name, dflt: int(args[args.index(name) + 1]) if name in args else dflt
    rounds = opt("--rounds", 5)
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    out_path = os.path.abspath(args[0])
    eng = Engine(synthetic_state_dict(0), torch.device("cuda:0"), 48, precision="f16x2", retry_precision=None)
    res = {"workload": "synthetic backbones and weights, f16x2, every position free, temperature 1; the encode is outside the timed region",
           "device": torch.cuda.get_device_name(0), "rounds": rounds,
           "sizes": [one_size(eng, 128, 64, rounds), one_size(eng, 256, 256, rounds)],
           "clock": "wall clock (time.perf_counter) around a synchronised device, one process, legs alternated"}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps([{k: s[k] for k in ("L", "N", "median_seconds", "spread_seconds", "a_beats_b_by_more_than_the_spread",
                                         "fraction_of_letters_equal")} for s in res["sizes"]]))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
