"""Packed against per-protein training of the sequence model: thermompnn_amd.model_utils.ProteinMPNN with packed = False (one
tmpnn_seqloss_forward / _backward pair per batch member) and packed = True (one tmpnn_seqloss_batch_forward / _backward pair per
batch), alternated inside one process. Workloads: tools/seqloss_bench.py's synthetic set (L in [40, 72]) as featurize-padded batches
of B = 8 and B = 64 proteins, and one padded [8, 256] batch. A step is forward + loss_smoothed + backward in training mode (dropout
on, a fresh decoding order per forward). Per workload and leg: the median over --rounds rounds of the ms per step, the rounds'
spread (min, max), saved / scratch bytes per step; and, in eval mode under one fixed order, that the two legs' losses agree.
Writes ONE JSON document to --out (default profiles/seqbatch_bench.json) and prints it.

    python tools/seqbatch_bench.py [--rounds 5] [--out profiles/seqbatch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from finetune_bench import items_for, timed  # noqa: E402


def batch_inputs(pdbs, device):
    from thermompnn_amd.pdb_io import tied_featurize
    f = tied_featurize(pdbs, device, None, None, None, None, None, None, ca_only=False)
    return f[0], f[1], f[2], f[4], f[12], f[5]                 # X, S, mask, chain_M, residue_idx, chain_encoding_all


def step(model, inp, randn=None):
    from thermompnn_amd.model_utils import loss_smoothed
    X, S, mask, chain_M, ridx, cenc = inp
    model.zero_grad(set_to_none=True)
    loss = loss_smoothed(S, model(X, S, mask, chain_M, ridx, cenc, randn=randn), mask * chain_M)[1]
    loss.backward()
    return loss.detach()


def bytes_per_step(lib, B, L, packed):
    K = min(48, L)
    if packed:
        return int(lib.tmpnn_seqloss_batch_saved_bytes(B * L, B, K)), int(lib.tmpnn_seqloss_batch_scratch_bytes(B * L, B, K))
    return B * int(lib.tmpnn_seqloss_saved_bytes(L)), int(lib.tmpnn_seqloss_scratch_bytes(L))      # B saved buffers live, one scratch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seqbatch_bench.json"))
    a = ap.parse_args(argv)
    from thermompnn_amd import _lib
    from thermompnn_amd import model_utils as mu
    from thermompnn_amd.weights import synthetic_state_dict
    lib = _lib.load()
    model = mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0, dropout=0.1)
    model.load_state_dict(synthetic_state_dict(0, "mpnn"))
    model = model.cuda()
    rng = np.random.default_rng(0)
    short = [p[0] for p, _ in items_for(rng.integers(40, 73, 128), 1, 1000)]
    workloads = {"B8_L40-72": [short[i:i + 8] for i in range(0, 64, 8)], "B64_L40-72": [short[:64], short[64:]],
                 "B8_L256": [[p[0] for p, _ in items_for([256] * 8, 1, 5256)]]}
    res = {"metric": "seqbatch_step", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "provenance": "one MI355X box, one run of tools/seqbatch_bench.py; legs alternated inside the process",
           "step": "forward + loss_smoothed + backward, training mode (dropout 0.1), k_neighbors 48"}
    for name, batches in workloads.items():
        inps = [batch_inputs(b, "cuda") for b in batches]
        B, L = int(inps[0][1].shape[0]), max(int(i[1].shape[1]) for i in inps)
        ms = {False: [], True: []}
        model.train()
        for packed in (False, True):                                       # warm-up: buffers, code objects
            model.packed = packed
            step(model, inps[0])
        for _ in range(a.rounds):
            for packed in (False, True):
                model.packed = packed
                ms[packed].append(1e3 * timed(lambda: [step(model, i) for i in inps], 1) / len(inps))
        model.eval()                                                       # no dropout, one order: the legs compute the same loss
        randn = torch.randn(inps[0][3].shape, generator=torch.Generator().manual_seed(1)).cuda()
        losses = {}
        for packed in (False, True):
            model.packed = packed
            losses[packed] = float(step(model, inps[0], randn))
        rel = abs(losses[True] - losses[False]) / abs(losses[False])
        entry = {"proteins_per_step": B, "L_padded": L, "rows_per_step": B * L, "steps_per_round": len(inps),
                 "eval_loss_loop": losses[False], "eval_loss_packed": losses[True], "eval_loss_rel_diff": rel, "losses_agree": rel <= 1e-6}
        for packed, leg in ((False, "loop"), (True, "packed")):
            sv, sc = bytes_per_step(lib, B, L, packed)
            entry[leg] = {"ms_per_step_median": round(statistics.median(ms[packed]), 3), "ms_per_step_min": round(min(ms[packed]), 3),
                          "ms_per_step_max": round(max(ms[packed]), 3), "ms_per_step_rounds": [round(v, 3) for v in ms[packed]],
                          "saved_bytes_per_step": sv, "scratch_bytes": sc}
        spread = max(entry[l]["ms_per_step_max"] - entry[l]["ms_per_step_min"] for l in ("loop", "packed"))
        gain = entry["loop"]["ms_per_step_median"] - entry["packed"]["ms_per_step_median"]
        entry["loop_over_packed"] = round(entry["loop"]["ms_per_step_median"] / entry["packed"]["ms_per_step_median"], 3)
        entry["packed_beats_loop_by_more_than_the_spread"] = bool(gain > spread)
        res[name] = entry
    model.packed = False
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
