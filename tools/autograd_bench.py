"""The torch-autograd path of TransferModel (thermompnn_amd/autograd.py) against the fused fine-tune step (MPNNTrainer.forward_backward)
on the synthetic set of tools/finetune_bench.py: ~240 proteins with L in [40, 72], 40 labelled mutants each, plus one L = 256 and one
L = 1024 protein. Per protein and step: model(pdb, mutations) + the per-mutant F.mse_loss mean + loss.backward(), with ProteinMPNN
unfrozen and frozen (requires_grad False: head-only backward), eval mode (no dropout); the fused step includes ProteinMPNN's backward.
Also times packing the parameters into the fp32 slab alone and reports the saved bytes a live graph holds per protein. Prints ONE
JSON line.

    python tools/autograd_bench.py [--proteins 240] [--reps 3]
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


def autograd_ms(model, items, reps):
    def one(item):
        pdb, muts = item
        pred, _ = model(pdb, muts)
        loss = torch.stack([F.mse_loss(p["ddG"], m.ddG.cuda()) for p, m in zip(pred, muts) if m.ddG is not None]).mean()
        loss.backward()

    one(items[0])                                                          # warm-up: slab, scratch, code objects
    return min(1e3 * timed(lambda: [one(it) for it in items], 1) / len(items) for _ in range(reps))


def fused_ms(tr, prots, reps):
    tr.forward_backward(prots[0])
    return min(1e3 * timed(lambda: [tr.forward_backward(p) for p in prots], 1) / len(prots) for _ in range(reps))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    from thermompnn_amd.autograd import plan_for
    from thermompnn_amd.finetune import MPNNTrainer
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = model_for(tmp)
    model.differentiable = True
    model.eval()
    tr = MPNNTrainer(model, seed=0, p_mpnn=0.0, p_head=0.0)
    sets = {"megascale": items_for(rng.integers(40, 73, a.proteins), 40, 1000), "L256": items_for([256], 40, 5256),
            "L1024": items_for([1024], 40, 6024)}
    plan = plan_for(model)
    params = [dict(model.named_parameters())[k] for k in plan.names]
    res = {"metric": "autograd_step", "device": torch.cuda.get_device_name(0), "slab_numel": plan.numel}

    def repack():
        plan._slab_key = None
        plan.pack(params)

    res["pack_slab_ms"] = round(1e3 * timed(repack, 50), 4)
    for name, items in sets.items():
        prots = tr.prepare(items)
        L = prots[0].L if name != "megascale" else 72
        row = {"ms_fused_step": round(fused_ms(tr, prots, a.reps), 3)}
        for p in model.prot_mpnn.parameters():
            p.requires_grad_(True)
        row["ms_autograd_unfrozen"] = round(autograd_ms(model, items, a.reps), 3)
        for p in model.prot_mpnn.parameters():
            p.requires_grad_(False)
        row["ms_autograd_frozen"] = round(autograd_ms(model, items, a.reps), 3)
        for p in model.prot_mpnn.parameters():
            p.requires_grad_(True)
        model.zero_grad(set_to_none=True)
        row["saved_bytes_per_protein"] = plan.saved_bytes(L, 40)
        row["scratch_bytes"] = int(plan.lib.tmpnn_finetune_scratch_bytes(L, 40, plan.n_final, int(plan.lightattn), plan.n_layers,
                                                                         plan.cdims))
        row["fused_workspace_bytes"] = tr.workspace_bytes(L, 40)
        if name == "megascale":
            row.update(proteins=len(items), L=[40, 72], bytes_at_L=72)
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
