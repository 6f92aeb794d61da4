#!/usr/bin/env python3
"""What the order mask costs, on one GPU: the bench protein (synthetic L = 256, tests/golden/syn_L256.npz) at f16x2, three legs
alternated five times in one process, each to a [256, 256, 21] log-probability output:
  (a) ProteinMPNN.conditional_probs' work: Engine.encode + ONE decode_ordered of 256 variants (one per position, that position last);
  (b) Engine.encode + decode_variants on the same 256 x 256 rows (the unmasked kernel: every neighbour visible);
  (c) Engine.encode + 256 separate decode_ordered calls of V = 1 (a caller without the batched form).
    python tools/ordered_bench.py out.json [--rounds 5]
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
from thermompnn_amd.protein_mpnn_utils import decoding_ranks  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402


def main():
    args = sys.argv[1:]
    opt = lambda name, dflt: int(args[args.index(name) + 1]) if name in args else dflt
    rounds = opt("--rounds", 5)
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    out_path = os.path.abspath(args[0])
    dev = torch.device("cuda:0")
    eng = Engine(synthetic_state_dict(0), dev, 48, precision="f16x2", retry_precision=None)
    with np.load(os.path.join(REPO, "tests", "golden", "syn_L256.npz")) as z:
        g = {k: z[k] for k in ("X", "S", "mask", "residue_idx", "chain_enc")}
    L = len(g["S"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    X, mask = t(g["X"], torch.float32), t(g["mask"], torch.float32)
    ridx, cenc = t(g["residue_idx"], torch.int32), t(g["chain_enc"], torch.int32)
    off = torch.tensor([0, L], dtype=torch.int32, device=dev)
    Sd = t(g["S"], torch.int32)[None].expand(L, L).contiguous()
    randn = torch.randn(1, L, generator=torch.Generator().manual_seed(0)).to(dev)
    ranks = decoding_ranks(torch.eye(L, device=dev), randn).contiguous()
    out = torch.empty((L, L, 21), device=dev)
    want = dict(want_ddg=False, want_log_probs=True)

    def ordered():
        enc = eng.encode(X, mask, ridx, cenc, off, max_len=L)
        out.copy_(eng.decode_ordered(enc, Sd, ranks, **want)["log_probs"])

    def unmasked():
        enc = eng.encode(X, mask, ridx, cenc, off, max_len=L)
        out.copy_(eng.decode_variants(enc, Sd, **want)["log_probs"])

    def one_by_one():
        enc = eng.encode(X, mask, ridx, cenc, off, max_len=L)
        for v in range(L):
            out[v] = eng.decode_ordered(enc, Sd[v:v + 1], ranks[v:v + 1], check_status=False, **want)["log_probs"][0]

    ways = {"a_ordered_256_variants": ordered, "b_unmasked_256_variants": unmasked, "c_ordered_256_calls": one_by_one}
    sample = {}
    for name, f in ways.items():                                     # warm-up; (a) and (c) must agree bit for bit
        f()
        torch.cuda.synchronize()
        sample[name] = out.clone()
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
    res = {"workload": f"syn_L256 (L={L}), 256 variants x 256 rows, log-probabilities, f16x2; every leg includes one encode",
           "device": torch.cuda.get_device_name(0), "rounds": rounds, "seconds_per_round": times, "median_seconds": med,
           "spread_seconds": spread, "ratio_a_over_b_median": med["a_ordered_256_variants"] / med["b_unmasked_256_variants"],
           "ratio_c_over_a_median": med["c_ordered_256_calls"] / med["a_ordered_256_variants"],
           "a_minus_b_median_seconds": med["a_ordered_256_variants"] - med["b_unmasked_256_variants"],
           "a_equals_c_bit_for_bit": bool(torch.equal(sample["a_ordered_256_variants"], sample["c_ordered_256_calls"])),
           "max_abs_a_minus_b": float((sample["a_ordered_256_variants"] - sample["b_unmasked_256_variants"]).abs().max()),
           "clock": "wall clock (time.perf_counter) around a synchronised device, one process"}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("median_seconds", "spread_seconds", "ratio_a_over_b_median", "ratio_c_over_a_median",
                                          "a_equals_c_bit_for_bit")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
