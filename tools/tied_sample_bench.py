#!/usr/bin/env python3
"""Tied against untied sampling on one GPU: the two-chain fixture 2OCJ_AB (tests/golden/2OCJ_AB.npz, 2 x 194 residues), synthetic
weights at f16x2, N = 64 and N = 256 chains, every position free, temperature 1; the two legs alternated in one process (five
rounds, each timing REPEATS calls):
  (a) Engine.sample_tied with residue i of chain A tied to residue i of chain B ([i, 194 + i], weights 1/2): 388 steps, 194 draws;
  (b) Engine.sample on the same chains and the same 388-step orders, untied: 388 draws.
Both legs start from the same encoded backbone (the encode is outside the timed region). The tied form adds a 21-float accumulate per
step and one read-add-write of three table rows per non-closing member. Reported: every round, medians, the spread (max - min) and
the ratio of the medians; that every tied pair carries one letter is checked once, outside the timed region.
    python tools/tied_sample_bench.py out.json [--rounds 5] [--repeats 4]
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
from thermompnn_amd.design import tied_decoding_order  # noqa: E402
from thermompnn_amd.engine import Engine  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402


def one_size(eng, g, N, rounds, repeats):
    dev = eng.device
    L = len(g["S"])
    half = L // 2
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    enc = eng.encode(t(g["X"], torch.float32), t(g["mask"], torch.float32), t(g["residue_idx"], torch.int32), t(g["chain_enc"], torch.int32),
                     torch.tensor([0, L], dtype=torch.int32, device=dev), max_len=L)
    rng = np.random.default_rng(N)
    pairs = [[i, half + i] for i in range(half)]
    oc = [tied_decoding_order(rng.permutation(L), pairs) for _ in range(N)]
    order = torch.stack([o for o, _ in oc]).to(dev, torch.int32)
    close = torch.stack([c for _, c in oc]).to(dev)
    weight = torch.full((N, L), 0.5, device=dev)
    u = t(rng.random((N, L)).astype(np.float32), torch.float32)
    S_fixed = torch.zeros((N, L), dtype=torch.int32, device=dev)
    free = torch.ones((N, L), device=dev)
    out = {}

    def tied():
        out["a"] = eng.sample_tied(enc, order, close, S_fixed, free, u, weight=weight, check_status=False)["S"]

    def untied():
        out["b"] = eng.sample(enc, order, S_fixed, free, u, check_status=False)["S"]

    ways = {"a_sample_tied": tied, "b_sample_untied": untied}
    for f in ways.values():                                          # warm-up
        f()
    torch.cuda.synchronize()
    assert bool((out["a"][:, :half] == out["a"][:, half:]).all()), "a tied pair carries two letters"
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, f in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(repeats):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / repeats)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    return {"L": L, "N": N, "steps": L, "tied_draws_per_chain": half, "seconds_per_call_by_round": times, "median_seconds": med,
            "spread_seconds": spread, "tied_over_untied": med["a_sample_tied"] / med["b_sample_untied"],
            "difference_exceeds_the_spread": abs(med["a_sample_tied"] - med["b_sample_untied"]) > max(spread.values())}


def main():
    args = sys.argv[1:]
    opt = lambda name, dflt: int(args[args.index(name) + 1]) if name in args else dflt
    rounds, repeats = opt("--rounds", 5), opt("--repeats", 4)
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    out_path = os.path.abspath(args[0])
    with np.load(os.path.join(REPO, "tests", "golden", "2OCJ_AB.npz")) as z:
        g = {k: z[k] for k in ("X", "S", "mask", "residue_idx", "chain_enc")}
    eng = Engine(synthetic_state_dict(0), torch.device("cuda:0"), 48, precision="f16x2", retry_precision=None)
    res = {"workload": "2OCJ chains A + B (388 residues), synthetic weights, f16x2, every position free, temperature 1, pairs [i, 194 + i] "
                       "with weights 1/2; the encode is outside the timed region",
           "device": torch.cuda.get_device_name(0), "rounds": rounds, "calls_per_round": repeats,
           "sizes": [one_size(eng, g, 64, rounds, repeats), one_size(eng, g, 256, rounds, repeats)],
           "clock": "wall clock (time.perf_counter) around a synchronised device, one process, legs alternated"}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps([{k: s[k] for k in ("L", "N", "median_seconds", "spread_seconds", "tied_over_untied")} for s in res["sizes"]]))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
