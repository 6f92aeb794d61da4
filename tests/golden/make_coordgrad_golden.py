"""Golden gradients with respect to the backbone coordinates, by IMPORTING THE REFERENCE (runs only in the build container).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coordgrad_golden.py [seqloss | finetune] [case]

The recipes of make_seqloss_golden.py and make_finetune_golden.py (float64, synthetic weights, injected dropout masks, the recorded
decoding order, the mutant list, targets and seed of finetune_2OCJ_A.npz), with X a leaf that requires grad: the reference's
featurizer is plain torch, so X.grad is dL / dX. For the ddG loss the leaf is put in place of the coordinates that tied_featurize
returns inside the reference's TransferModel.forward.

Stored per file: E_idx, and per tag ("ones" / "drawn") ``{tag}_dX`` [L,4,3] float64 and the loss; on the heavy draw also
``{tag}_dX_d32``, the max distance of the SAME reference run in float32 from it. Tensors only, a few KB each.

Every case has more than K = 48 valid residues (asserted), so no masked residue sits in a valid row's neighbour list and the reference's
gradient coincides with the contract of the _x backwards (D_max of _dist a constant) exactly.
"""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                          # noqa: E402  (imports the reference, puts the repo on sys.path)
import model_utils as ref_mu                      # noqa: E402  (the reference)
import make_finetune_golden as mf                 # noqa: E402
import make_seqloss_golden as ms                  # noqa: E402

from thermompnn_amd.datasets import Mutation      # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402

SCALE = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)
SEQ_CASES = ("2OCJ_A", "2OCJ_A_gap", "2OCJ_A_fixed", "2OCJ_A_hot")
FT_CASES = ("2OCJ_A", "2OCJ_A_hot")


def inject(mpnn, tag, L, K):
    for l, layer in enumerate(mpnn.encoder_layers):
        for j, name in enumerate(("dropout1", "dropout2", "dropout3")):
            rows = L * K if j == 2 else L
            m = np.ones((rows, 128)) if tag == "ones" else mf.site_mask(3 * l + j, rows) * SCALE
            setattr(layer, name, mf.InjectedDropout(torch.from_numpy(m)))
    for l, layer in enumerate(mpnn.decoder_layers):
        for j, name in enumerate(("dropout1", "dropout2")):
            m = np.ones((L, 128)) if tag == "ones" else mf.site_mask(9 + 2 * l + j, L) * SCALE
            setattr(layer, name, mf.InjectedDropout(torch.from_numpy(m)))


def spy_graph(mpnn, captured):
    fwd = mpnn.features.forward

    def spy(*a, **k):
        E, E_idx = fwd(*a, **k)
        captured["E_idx"] = E_idx
        return E, E_idx
    mpnn.features.forward = spy
    return fwd


def more_than_k_valid(mask, K):
    assert int((mask > 0).sum()) > K, "a protein with at most K valid residues: the reference's D_max leak is live, not a contract case"


def seqloss(case):
    entry = mg.ref_utils.alt_parse_PDB(ms.CASES[case], "A")[0]
    feats = mg.ref_utils.tied_featurize([entry], "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask, chain_M, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[4], feats[5], feats[12]
    L = int(S.shape[1])
    K = min(48, L)
    more_than_k_valid(mask[0], K)
    if case == "2OCJ_A_fixed":
        chain_M = chain_M.clone()
        chain_M[0, ::3] = 0.0
    weight_seed, style = ms.WEIGHTS.get(case, (mg.WEIGHT_SEED, "xavier"))
    out = dict(weight_seed=np.int64(weight_seed), seed=np.int64(mf.SEED), step=np.int64(mf.STEP))

    def run(tag, dtype):
        model = ref_mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0, dropout=0.1)
        model.load_state_dict(synthetic_state_dict(weight_seed, "mpnn", style), strict=True)
        model = model.to(dtype).train()
        model.features.embeddings.linear.register_forward_pre_hook(lambda mod, args: tuple(x.to(dtype) for x in args))
        inject(model, tag, L, K)
        captured = {}
        fwd = spy_graph(model, captured)
        Xl = X.to(dtype).clone().requires_grad_(True)
        try:
            torch.manual_seed(ms.ORDER_SEED)
            log_probs = model(Xl, S, mask, chain_M, residue_idx, chain_enc)
        finally:
            model.features.forward = fwd
        _, loss = ref_mu.loss_smoothed(S, log_probs.double(), mask * chain_M)
        loss.backward()
        return Xl.grad[0].double().numpy(), loss.item(), captured["E_idx"][0].numpy().astype(np.int32)

    for tag in ms.TAGS.get(case, ("ones", "drawn")):
        dX, loss, E_idx = run(tag, torch.float64)
        out["E_idx"], out[f"{tag}_dX"], out[f"{tag}_loss"] = E_idx, dX, np.float64(loss)
        line = f"seqloss {case} {tag}: loss {loss:.8f}, max|dX| {np.abs(dX).max():.4g} per slot {np.abs(dX).max((0, 2))}"
        if case in ms.WEIGHTS:
            d32 = run(tag, torch.float32)[0]
            out[f"{tag}_dX_d32"] = np.float64(np.abs(d32 - dX).max())
            line += f", float32 reference d32 / max|dX| {out[f'{tag}_dX_d32'] / np.abs(dX).max():.3g}"
        print(line)
    path = os.path.join(HERE, f"coordgrad_seqloss_{case}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


def finetune(case):
    g = np.load(os.path.join(HERE, "finetune_2OCJ_A.npz"))           # the mutant list, the targets and the seed
    pdb = mg.ref_utils.alt_parse_PDB(mf.CASES[case], "A")
    seq = pdb[0]["seq"]
    L = len(seq)
    K = min(48, L)
    muts = [Mutation(int(p), mf.AA20[w], mf.AA20[m], None, "2OCJ") for p, w, m in zip(g["positions"], g["wildtype"], g["mutation"])]
    assert all(seq[m.position] == m.wildtype for m in muts) and int(g["seed"]) == mf.SEED and int(g["step"]) == mf.STEP
    targets = g["targets"]
    weight_seed, style = mf.WEIGHTS.get(case, (mg.WEIGHT_SEED, "xavier"))
    out = dict(weight_seed=np.int64(weight_seed), seed=np.int64(mf.SEED), step=np.int64(mf.STEP))
    tf = mg.ref_tm.tied_featurize

    def run(tag, dtype):
        with tempfile.TemporaryDirectory() as tmp:
            model = mg.build_reference_model(tmp, weight_seed, style).to(dtype)
        for m, t in zip(muts, targets):
            m.ddG = None if np.isnan(t) else torch.tensor([float(t)], dtype=dtype)
        captured = {}

        def spy_featurize(*a, **k):
            feats = [t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t for t in tf(*a, **k)]
            more_than_k_valid(feats[2][0], K)
            feats[0] = captured["X"] = feats[0].detach().clone().requires_grad_(True)
            return tuple(feats)
        mg.ref_tm.tied_featurize = spy_featurize
        model.prot_mpnn.features.embeddings.linear.register_forward_pre_hook(lambda mod, args: tuple(x.to(dtype) for x in args))
        for prm in model.parameters():
            prm.requires_grad_(True)
        model.light_attention.dropout = nn.Identity()
        inject(model.prot_mpnn, tag, L, K)
        fwd = spy_graph(model.prot_mpnn, captured)
        model.train()
        try:
            pred, _ = model([pdb[0]], muts)
        finally:
            model.prot_mpnn.features.forward = fwd
            mg.ref_tm.tied_featurize = tf
        loss = torch.stack([F.mse_loss(o["ddG"], m.ddG) for m, o in zip(muts, pred) if m.ddG is not None]).mean()
        loss.backward()
        return captured["X"].grad[0].double().numpy(), loss.item(), captured["E_idx"][0].numpy().astype(np.int32)

    for tag in mf.TAGS.get(case, ("ones", "drawn")):
        dX, loss, E_idx = run(tag, torch.float64)
        out["E_idx"], out[f"{tag}_dX"], out[f"{tag}_loss"] = E_idx, dX, np.float64(loss)
        line = f"finetune {case} {tag}: loss {loss:.8f}, max|dX| {np.abs(dX).max():.4g} per slot {np.abs(dX).max((0, 2))}"
        if case in mf.WEIGHTS:
            d32 = run(tag, torch.float32)[0]
            out[f"{tag}_dX_d32"] = np.float64(np.abs(d32 - dX).max())
            line += f", float32 reference d32 / max|dX| {out[f'{tag}_dX_d32'] / np.abs(dX).max():.3g}"
        print(line)
    path = os.path.join(HERE, f"coordgrad_finetune_{case}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    kinds = {"seqloss": (seqloss, SEQ_CASES), "finetune": (finetune, FT_CASES)}
    for kind in (sys.argv[1:2] or list(kinds)):
        fn, cases = kinds[kind]
        for case in (sys.argv[2:3] or cases):
            fn(case)
