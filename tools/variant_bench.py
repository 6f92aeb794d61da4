#!/usr/bin/env python3
"""Three ways to the same [V, L, 21] output on one GPU: the bench protein (synthetic L = 256) under all 19 L = 4 864
single-substitution backgrounds (24.9 M predictions), alternated five times in one process:
  (a) ssm_forward on replicated copies in batches of 64 (the fused path, encoder and all, once per copy);
  (b) the stage-wise loop: k-NN, featurizer and encoder once, then dec_layer x 3 + ddg_head per variant;
  (c) Engine.encode + Engine.decode_variants.
    python tools/variant_bench.py out.json [--rounds 5] [--variants N]
Acceptance: (c) is faster than (a) and than (b) in every round. One run on one box; the JSON keeps every round."""
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
from thermompnn_amd.variant_scan import sequence_indices, single_backgrounds  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402


def main():
    args = sys.argv[1:]
    opt = lambda name, dflt: int(args[args.index(name) + 1]) if name in args else dflt
    rounds, n_var = opt("--rounds", 5), opt("--variants", 0)
    if not args or args[0].startswith("--"):
        raise SystemExit(__doc__)
    out_path = os.path.abspath(args[0])
    dev = torch.device("cuda:0")
    eng = Engine(synthetic_state_dict(0), dev, 48, retry_precision=None)
    L = 256
    Xn, seq = synthetic_backbone(L, 0)
    base = sequence_indices(seq)
    S = single_backgrounds(seq)[1].reshape(-1, L)
    S = S[(S != base[None]).any(1)]
    if n_var:
        S = S[:n_var]
    V = len(S)
    X = torch.tensor(Xn, dtype=torch.float32, device=dev)
    Sd = torch.from_numpy(S).to(dev, torch.int32)
    mask, ridx, cenc = torch.ones(L, device=dev), torch.arange(L, dtype=torch.int32, device=dev), torch.ones(L, dtype=torch.int32, device=dev)
    off1 = torch.tensor([0, L], dtype=torch.int32, device=dev)
    B = 64
    rep = lambda t: t.repeat(B, *([1] * (t.dim() - 1)))
    Xb, mb, rb, cb = rep(X), rep(mask), rep(ridx), rep(cenc)
    offb = (torch.arange(B + 1, dtype=torch.int32) * L).to(dev)
    out = torch.empty((V, L, 21), device=dev)

    def fused():
        for v0 in range(0, V, B):
            n = min(B, V - v0)
            r = eng.ssm_forward(Xb[:n * L], Sd[v0:v0 + n].reshape(-1), mb[:n * L], rb[:n * L], cb[:n * L], offb[:n + 1], max_len=L,
                                check_status=False)
            out[v0:v0 + n] = r["ddg"].view(n, L, 21)
        eng.check_last_status()

    def stagewise():
        E_idx, D_nb = eng.knn_topk(X, mask, off1, max_len=L)
        hE = eng.edge_featurize(X, ridx, cenc, E_idx, D_nb)
        hV = torch.zeros((L, 128), device=dev)
        for l in range(3):
            eng.enc_layer(l, hV, hE, E_idx, mask)
        for v in range(V):
            h = [hV]
            for l in range(3):
                h.append(eng.dec_layer(l, h[-1], hE, E_idx, Sd[v], mask))
            out[v] = eng.ddg_head(h[3], h[2], Sd[v])

    def variants():
        enc = eng.encode(X, mask, ridx, cenc, off1, max_len=L)
        out.copy_(eng.decode_variants(enc, Sd)["ddg"])

    ways = {"a_fused_replicated": fused, "b_stagewise_loop": stagewise, "c_encode_decode_variants": variants}
    sample = {}
    for name, f in ways.items():                                     # warm-up + the three outputs agree
        f()
        torch.cuda.synchronize()
        sample[name] = out.clone()
    agree = {k: float((sample[k] - sample["a_fused_replicated"]).abs().max()) for k in sample}
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for name, f in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    c = times["c_encode_decode_variants"]
    res = {"workload": f"synthetic L={L}, V={V} single-substitution backgrounds, {V * L * 20} predictions, f16x2",
           "device": torch.cuda.get_device_name(0), "rounds": rounds, "seconds_per_round": times, "median_seconds": med,
           "ratio_a_over_c_per_round": [a / x for a, x in zip(times["a_fused_replicated"], c)],
           "ratio_b_over_c_per_round": [b / x for b, x in zip(times["b_stagewise_loop"], c)],
           "ratio_a_over_c_median": med["a_fused_replicated"] / med["c_encode_decode_variants"],
           "ratio_b_over_c_median": med["b_stagewise_loop"] / med["c_encode_decode_variants"],
           "c_faster_in_every_round": all(x < a and x < b for a, b, x in zip(times["a_fused_replicated"], times["b_stagewise_loop"], c)),
           "max_abs_ddg_difference_vs_a": agree, "clock": "wall clock (time.perf_counter) around a synchronised device, one process"}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("median_seconds", "ratio_a_over_c_per_round", "ratio_b_over_c_per_round", "c_faster_in_every_round",
                                          "max_abs_ddg_difference_vs_a")}))
    return 0 if res["c_faster_in_every_round"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
