"""Head-training throughput on a synthetic Mega-scale-shaped set: ~240 proteins with L in [40, 72], all 19 L single mutants
labelled, targets from a teacher head (synthetic weights seed 1) through TransferModel.ssm_table; the student (seed 0) trains
with thermompnn_amd.train.HeadTrainer. Prints ONE JSON line: feature-cache build s, ms per step, epoch s, validation s.

    python tools/train_bench.py [--proteins 240] [--epochs 2]
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


def model_for(tmp, head_seed):
    from thermompnn_amd import weights
    from thermompnn_amd.train import Config
    from thermompnn_amd.transfer_model import TransferModel
    sd = weights.synthetic_state_dict(0)
    sd.update({k: v for k, v in weights.synthetic_state_dict(head_seed).items() if not k.startswith("prot_mpnn.")})
    os.makedirs(os.path.join(tmp, "vanilla_model_weights"), exist_ok=True)
    weights.save_vanilla_checkpoint(os.path.join(tmp, "vanilla_model_weights", "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    cfg = Config.wrap(dict(model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=True, load_pretrained=True,
                                      lightattn=True), platform=dict(thermompnn_dir=tmp)))
    m = TransferModel(cfg)
    m.load_state_dict(sd)
    return m.cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=240)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--val-fraction", type=float, default=0.1)
    a = ap.parse_args(argv)
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.synthetic import synthetic_pdb_dict
    from thermompnn_amd.train import HeadTrainer
    rng = np.random.default_rng(0)
    prots = [synthetic_pdb_dict(int(L), seed=1000 + i) for i, L in enumerate(rng.integers(40, 73, a.proteins))]
    with tempfile.TemporaryDirectory() as tmp:
        teacher = model_for(os.path.join(tmp, "t"), 1)
        items = []
        for p in prots:
            table = teacher.ssm_table([p]).cpu().numpy()
            seq = p["seq"]
            items.append(([p], [Mutation(i, seq[i], c, torch.tensor([float(table[i, AA20.index(c)])]), "syn")
                                for i in range(len(seq)) for c in AA20 if c != seq[i]]))
        student = model_for(os.path.join(tmp, "s"), 0)
    n_val = max(1, int(round(a.val_fraction * len(items))))
    tr = HeadTrainer(student, seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_split, val_split = tr.build_cache(items[n_val:]), tr.build_cache(items[:n_val])
    torch.cuda.synchronize()
    cache_s = time.perf_counter() - t0
    order_rng = np.random.default_rng(1)
    epoch_s, val_s, mse = [], [], []
    for _ in range(a.epochs):
        tr.begin_epoch(len(train_split))
        t0 = time.perf_counter()
        for i in order_rng.permutation(len(train_split)):
            tr.step(train_split, int(i))
        losses = tr.epoch_losses()                                   # the epoch's one device-to-host read
        epoch_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        mse.append(tr.evaluate(val_split)["mse"])
        val_s.append(time.perf_counter() - t0)
    steps = len(train_split)
    print(json.dumps({"metric": "head_train", "proteins": len(items), "train_proteins": steps, "val_proteins": n_val,
                      "train_mutants": int(train_split.rows.numel()), "cache_build_s": round(cache_s, 3),
                      "ms_per_step": round(1e3 * min(epoch_s) / steps, 4), "epoch_s": round(min(epoch_s), 4),
                      "val_s": round(min(val_s), 4), "train_loss_last_epoch": float(np.mean(losses)),
                      "val_mse": [round(float(x), 5) for x in mse], "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
