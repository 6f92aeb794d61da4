"""Fine-tuning throughput (ProteinMPNN + head, thermompnn_amd.finetune.MPNNTrainer) on a synthetic Mega-scale-shaped set: ~240
proteins with L in [40, 72], 40 labelled single mutants each (synthetic weights, random targets), plus one L = 256 and one L = 1024
protein. A step's forward alone is timed through the eval entry (the same training forward without dropout); backward = step -
forward. Prints ONE JSON line: ms per step / forward / backward per set, AdamW ms, workspace bytes.

    python tools/finetune_bench.py [--proteins 240] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AA20 = "ACDEFGHIKLMNPQRSTVWY"


def model_for(tmp):
    from thermompnn_amd import weights
    from thermompnn_amd.train import Config
    from thermompnn_amd.transfer_model import TransferModel
    sd = weights.synthetic_state_dict(0)
    os.makedirs(os.path.join(tmp, "vanilla_model_weights"), exist_ok=True)
    weights.save_vanilla_checkpoint(os.path.join(tmp, "vanilla_model_weights", "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    cfg = Config.wrap(dict(model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=False, load_pretrained=True,
                                      lightattn=True), platform=dict(thermompnn_dir=tmp)))
    m = TransferModel(cfg)
    m.load_state_dict(sd)
    return m.cuda()


def items_for(lengths, n_mut, seed0):
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.synthetic import synthetic_pdb_dict
    rng = np.random.default_rng(seed0)
    out = []
    for i, L in enumerate(lengths):
        p = synthetic_pdb_dict(int(L), seed=seed0 + i)
        seq = p["seq"]
        muts = []
        for _ in range(n_mut):
            j = int(rng.integers(0, len(seq)))
            muts.append(Mutation(j, seq[j], AA20[int(rng.integers(0, 20))], torch.tensor([float(rng.normal())]), "syn"))
        out.append(([p], muts))
    return out


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def measure(tr, prots, reps):
    """-> (ms per step, ms per forward) averaged over the set, best of reps passes."""
    step_ms, fwd_ms = [], []
    for _ in range(reps):
        step_ms.append(1e3 * timed(lambda: [tr.forward_backward(p) for p in prots], 1) / len(prots))
        fwd_ms.append(1e3 * timed(lambda: [tr.predict_one(p) for p in prots], 1) / len(prots))
    return min(step_ms), min(fwd_ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    from thermompnn_amd.finetune import MPNNTrainer
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = model_for(tmp)
    tr = MPNNTrainer(model, seed=0)
    mega = tr.prepare(items_for(rng.integers(40, 73, a.proteins), 40, 1000))
    res = {"metric": "finetune_step", "device": torch.cuda.get_device_name(0)}
    tr.forward_backward(mega[0])                                         # warm-up: workspace, code objects
    s, f = measure(tr, mega, a.reps)
    res["megascale"] = {"proteins": len(mega), "L": [40, 72], "ms_per_step": round(s, 3), "ms_forward": round(f, 3),
                        "ms_backward": round(s - f, 3), "workspace_bytes_L72": tr.workspace_bytes(72, 40)}
    for L in (256, 1024):
        p = tr.prepare(items_for([L], 40, 5000 + L))
        tr.forward_backward(p[0])
        s, f = measure(tr, p, a.reps)
        res[f"L{L}"] = {"ms_per_step": round(s, 3), "ms_forward": round(f, 3), "ms_backward": round(s - f, 3),
                        "workspace_bytes": tr.workspace_bytes(L, 40)}
    res["adamw_ms"] = round(1e3 * timed(tr.adamw, 20), 4)
    res["slab_numel"] = tr.numel
    print(json.dumps(res))


if __name__ == "__main__":
    main()
