"""Sequence-loss throughput (tmpnn_seqloss_forward + _backward through thermompnn_amd.model_utils.ProteinMPNN, loss_smoothed,
loss.backward()) next to the ddG fine-tune pair (tmpnn_finetune_forward + _backward through TransferModel's differentiable path,
40 mutants per protein) at the same sizes: ~240 synthetic proteins with L in [40, 72], one L = 256 and one L = 1024 protein.
Synthetic weights, dropout on (training mode), a fresh decoding order per forward. Prints ONE JSON line: ms per protein for
forward + backward and for the forward alone (under torch.no_grad), best of --reps passes.

    python tools/seqloss_bench.py [--proteins 240] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from finetune_bench import items_for, model_for, timed  # noqa: E402


def seq_inputs(pdb, device):
    from thermompnn_amd.pdb_io import tied_featurize
    f = tied_featurize([pdb], device, None, None, None, None, None, None, ca_only=False)
    return f[0], f[1], f[2], f[4], f[12], f[5]                 # X, S, mask, chain_M, residue_idx, chain_encoding_all


def seq_step(model, inp):
    from thermompnn_amd.model_utils import loss_smoothed
    X, S, mask, chain_M, ridx, cenc = inp
    model.zero_grad(set_to_none=True)
    loss_smoothed(S, model(X, S, mask, chain_M, ridx, cenc), mask * chain_M)[1].backward()


def seq_forward(model, inp):
    X, S, mask, chain_M, ridx, cenc = inp
    with torch.no_grad():
        model(X, S, mask, chain_M, ridx, cenc)


def ddg_step(model, item):
    pdb, muts = item
    model.zero_grad(set_to_none=True)
    pred, _ = model(pdb, muts)
    torch.stack([F.mse_loss(p["ddG"], m.ddG.cuda()) for p, m in zip(pred, muts)]).mean().backward()


def best(fn, things, reps):
    return round(min(1e3 * timed(lambda: [fn(t) for t in things], 1) / len(things) for _ in range(reps)), 3)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    from thermompnn_amd import _lib
    from thermompnn_amd import model_utils as mu
    from thermompnn_amd.weights import synthetic_state_dict
    lib = _lib.load()
    rng = np.random.default_rng(0)
    seq = mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0, dropout=0.1)
    seq.load_state_dict(synthetic_state_dict(0, "mpnn"))
    seq = seq.cuda().train()
    with tempfile.TemporaryDirectory() as tmp:
        ddg = model_for(tmp)
    ddg.differentiable = True
    ddg.train()
    res = {"metric": "seqloss_step", "device": torch.cuda.get_device_name(0), "slab_numel": int(lib.tmpnn_seqloss_slab_numel())}
    sets = {"megascale": items_for(rng.integers(40, 73, a.proteins), 40, 1000), "L256": items_for([256], 40, 5256),
            "L1024": items_for([1024], 40, 6024)}
    for name, items in sets.items():
        inps = [seq_inputs(pdb[0], "cuda") for pdb, _ in items]
        seq_step(seq, inps[0])                                             # warm-up: buffers, code objects
        ddg_step(ddg, items[0])
        Lmax = max(int(i[1].shape[1]) for i in inps)
        res[name] = {"proteins": len(items), "L_max": Lmax,
                     "seqloss_ms_forward_backward": best(lambda i: seq_step(seq, i), inps, a.reps),
                     "seqloss_ms_forward": best(lambda i: seq_forward(seq, i), inps, a.reps),
                     "finetune_ms_forward_backward": best(lambda it: ddg_step(ddg, it), items, a.reps),
                     "seqloss_saved_bytes": int(lib.tmpnn_seqloss_saved_bytes(Lmax)),
                     "seqloss_scratch_bytes": int(lib.tmpnn_seqloss_scratch_bytes(Lmax))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
