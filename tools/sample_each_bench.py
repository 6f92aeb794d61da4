#!/usr/bin/env python3
"""Sampling for many backbones, on one GPU: synthetic backbones and weights at f16x2, every position free, temperature 1, medians of
five alternated rounds in one process. Three legs:
  (a) many backbones: P = 64 (and P = 256) different backbones of L = 128 with N = 8 chains each,
        leg 1: ONE Engine.encode of the packed batch + ONE Engine.sample_each;
        leg 2: P x (Engine.encode of the backbone alone + Engine.sample) — what a caller had before sample_each;
      both legs are fed the same orders and uniforms and the encodes are INSIDE the timed region; their letters must agree
      everywhere (asserted: the per-protein form promises the solo call's bits);
  (b) one backbone: P = 1, L = 128, N = 64, Engine.sample_each against Engine.sample on the same context and chains (the encode
      outside the timed region): what the per-protein form itself costs;
  (c) the untied kernel unchanged (only with --parent DIR, a checkout of the parent commit with its library built):
      tools/sample_bench.py of this tree and of DIR, three alternated runs each, every run a process of its own under a time limit;
      reported: the medians of Engine.sample (leg a of that tool) per tree and whether they differ by more than the runs' spread.
    python tools/sample_each_bench.py out.json [--rounds 5] [--parent DIR]
Recorded, not gated. One run on one box; the JSON keeps every round."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from thermompnn_amd.engine import Engine  # noqa: E402
from thermompnn_amd.synthetic import synthetic_backbone  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402


def timed(ways, rounds):
    """Alternated rounds of the callables -> (seconds per round, medians, spreads); one warm-up call each first."""
    for f in ways.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, f in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times, {k: statistics.median(v) for k, v in times.items()}, {k: max(v) - min(v) for k, v in times.items()}


def chains(P, L, N, dev, seed):
    """Per-protein random orders (local indices) and uniforms, zeros as fixed letters, every position free."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    order = torch.argsort(torch.rand((P, N, L), device=dev, generator=gen), dim=2).to(torch.int32)
    u = torch.rand((P, N, L), device=dev, generator=gen)
    return order, u


def many_backbones(eng, P, L, N, rounds):
    dev = eng.device
    X = [torch.from_numpy(np.ascontiguousarray(synthetic_backbone(L, 100 + p)[0])).to(dev, torch.float32) for p in range(P)]
    Xall = torch.cat(X)
    mask, ridx, cenc = torch.ones(L, device=dev), torch.arange(L, dtype=torch.int32, device=dev), torch.ones(L, dtype=torch.int32, device=dev)
    off1 = torch.tensor([0, L], dtype=torch.int32)
    offs = torch.arange(P + 1, dtype=torch.int32) * L
    order, u = chains(P, L, N, dev, 7)
    shift = (torch.arange(P, dtype=torch.int32, device=dev) * L)[:, None, None]
    pack = lambda t: t.permute(1, 0, 2).reshape(N, P * L).contiguous()
    O_all, U_all = pack(order + shift), pack(u)
    zeros, ones = torch.zeros((N, P * L), dtype=torch.int32, device=dev), torch.ones((N, P * L), device=dev)
    out = {}

    def one_launch():
        enc = eng.encode(Xall, mask.repeat(P), ridx.repeat(P), cenc.repeat(P), offs, max_len=L)
        out["each"] = eng.sample_each(enc, O_all, zeros, ones, U_all, check_status=False)["S"]

    def one_call_per_backbone():
        S = []
        for p in range(P):
            enc = eng.encode(X[p], mask, ridx, cenc, off1, max_len=L)
            S.append(eng.sample(enc, order[p], zeros[:, :L], ones[:, :L], u[p], check_status=False)["S"])
        out["loop"] = torch.cat(S, dim=1)

    times, med, spread = timed({"one_encode_one_sample_each": one_launch, "P_encodes_P_sample_calls": one_call_per_backbone}, rounds)
    same = bool(torch.equal(out["each"], out["loop"]))
    assert same, "sample_each and the per-backbone loop disagree on a letter"
    a, b = med["one_encode_one_sample_each"], med["P_encodes_P_sample_calls"]
    return {"P": P, "L": L, "N": N, "seconds_per_round": times, "median_seconds": med, "spread_seconds": spread, "letters_all_equal": same,
            "loop_over_each": b / a, "each_beats_the_loop_by_more_than_the_spread": b - a > max(spread.values())}


def one_backbone(eng, L, N, rounds):
    dev = eng.device
    X = torch.from_numpy(np.ascontiguousarray(synthetic_backbone(L, 3)[0])).to(dev, torch.float32)
    mask, ridx, cenc = torch.ones(L, device=dev), torch.arange(L, dtype=torch.int32, device=dev), torch.ones(L, dtype=torch.int32, device=dev)
    enc = eng.encode(X, mask, ridx, cenc, torch.tensor([0, L], dtype=torch.int32), max_len=L)
    order, u = chains(1, L, N, dev, 9)
    zeros, ones = torch.zeros((N, L), dtype=torch.int32, device=dev), torch.ones((N, L), device=dev)
    out = {}

    def each():
        out["each"] = eng.sample_each(enc, order[0], zeros, ones, u[0], check_status=False)

    def whole_axis():
        out["sample"] = eng.sample(enc, order[0], zeros, ones, u[0], check_status=False)

    times, med, spread = timed({"sample_each": each, "sample": whole_axis}, rounds)
    same = bool(torch.equal(out["each"]["S"], out["sample"]["S"]) and torch.equal(out["each"]["probs"], out["sample"]["probs"]))
    assert same, "sample_each on one backbone is not Engine.sample bit for bit"
    return {"P": 1, "L": L, "N": N, "seconds_per_round": times, "median_seconds": med, "spread_seconds": spread, "bits_equal": same,
            "each_over_sample": med["sample_each"] / med["sample"],
            "difference_exceeds_the_spread": abs(med["sample_each"] - med["sample"]) > max(spread.values())}


def untied_kernel_unchanged(parent, runs=3, limit=300):
    """tools/sample_bench.py of this tree and of ``parent``, alternated; every run its own process under a time limit."""
    trees = {"this_commit": REPO, "parent_commit": os.path.abspath(parent)}
    med = {k: {} for k in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(runs):
            for name, tree in trees.items():
                path = os.path.join(tmp, f"{name}_{r}.json")
                subprocess.run([sys.executable, os.path.join(tree, "tools", "sample_bench.py"), path], check=True, timeout=limit,
                               cwd=tree, stdout=subprocess.DEVNULL)
                print(f"(c) run {r + 1} of {runs}, {name}: done", file=sys.stderr, flush=True)
                for s in json.load(open(path))["sizes"]:
                    med[name].setdefault(f"L{s['L']}_N{s['N']}", []).append(s["median_seconds"]["a_one_sample_call"])
    res = {"runs_per_tree": runs, "engine_sample_median_seconds_per_run": med, "sizes": {}}
    for size in med["this_commit"]:
        a, b = med["this_commit"][size], med["parent_commit"][size]
        spread = max(max(a) - min(a), max(b) - min(b))
        diff = statistics.median(a) - statistics.median(b)
        res["sizes"][size] = {"this_median_seconds": statistics.median(a), "parent_median_seconds": statistics.median(b),
                              "this_minus_parent_seconds": diff, "largest_spread_of_a_tree_seconds": spread,
                              "differs_by_more_than_the_spread": abs(diff) > spread}
    return res


def main():
    args = sys.argv[1:]
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    out_path = os.path.abspath(args[0])
    eng = Engine(synthetic_state_dict(0), torch.device("cuda:0"), 48, precision="f16x2", retry_precision=None)
    res = {"workload": "synthetic backbones and weights, f16x2, every position free, temperature 1",
           "device": torch.cuda.get_device_name(0), "rounds": rounds,
           "a_many_backbones": [many_backbones(eng, 64, 128, 8, rounds), many_backbones(eng, 256, 128, 8, rounds)],
           "b_one_backbone": one_backbone(eng, 128, 64, rounds),
           "clock": "wall clock (time.perf_counter) around a synchronised device, one process, legs alternated; (a) includes the encodes"}
    del eng
    torch.cuda.empty_cache()
    res["c_untied_kernel_unchanged"] = untied_kernel_unchanged(parent) if parent else "not run (--parent DIR)"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    brief = [{k: s[k] for k in ("P", "N", "median_seconds", "spread_seconds")} for s in res["a_many_backbones"] + [res["b_one_backbone"]]]
    print(json.dumps({"a_b": brief, "c": res["c_untied_kernel_unchanged"] if not parent else res["c_untied_kernel_unchanged"]["sizes"]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
