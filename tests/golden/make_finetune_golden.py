"""Golden gradients of one fine-tuning step (ProteinMPNN unfrozen), by IMPORTING THE REFERENCE (runs only in the build container).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_finetune_golden.py [2OCJ_A | 2OCJ_A_gap | 2OCJ_A_hot]

The reference TransferModel (make_golden.build_reference_model: synthetic weights, seed 0, released head) runs in float64 and in
train mode with every parameter trainable, over ~96 mutants of 2OCJ chain A (several sharing a position, a few with ddG None). Each
of the 15 nn.Dropout modules of its EncLayers / DecLayers is replaced by a module that multiplies by an injected mask: all ones, or
the masks of the documented generator of csrc/tmpnn_finetune.hip (restated in numpy below; seed 7, step 3) times 1 / (1 - thr / 2^24).
The head's conv dropout is the identity in both cases. Loss = mean over labelled mutants of F.mse_loss (train_thermompnn.py:52-62).

Stored: the E_idx the reference used, the loss per case, and per trainable tensor either the full gradient (<= 4096 entries) or a
fixed sample of 2048 entries (seeded by the tensor's name and size, sample_index) with the float64 sum of squares, the dot with a
seeded +-1 vector and max|g|. Full gradients up to 16 k entries and 4096-entry samples would make the file about 2.5 MB; these
limits keep it under 1 MB. W_out has no gradient and is not stored. Only tensors are stored, nothing of the reference's source.

2OCJ_A_gap runs the same recipe on tests/golden/2OCJ_gap_chainA.pdb (residue 120 without its N line: position 24 has mask 0 and keeps
its letter; residues 150-152 removed: positions 54-56 are '-', token 20, mask 0). Its mutant positions are drawn from the residues
that have a letter, position 24 always among them. The E_idx of a masked row is arbitrary (every candidate sits at the same adjusted
distance) and does not reach the loss.

2OCJ_A_hot runs 2OCJ_A's mutants from the heavy weight draw "hot", seed 2 (matrices x 3, biases x 5, LayerNorm gamma in [-2, 2]), the
drawn-mask run only, and stores beside every float64 result its distance "d32" from the same reference run in float32.
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

from thermompnn_amd.datasets import ALPHABET, Mutation  # noqa: E402

AA20 = ALPHABET[:20]
FULL_MAX, SAMPLE = 4096, 2048
SEED, STEP = 7, 3


def _mix(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def site_mask(site, rows, p=0.1):
    with np.errstate(over="ignore"):
        k2 = _mix(_mix(np.uint64(SEED) ^ np.uint64(0x9E3779B97F4A7C15)) + np.uint64(STEP))
        ks = _mix(k2 ^ (np.uint64(0xD6E8FEB86659FD93) * np.uint64(site + 1)))
    h = _mix(ks ^ ((np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(128, dtype=np.uint64)[None, :]))
    return ((h >> np.uint64(40)) >= np.uint64(round(p * 2 ** 24))).astype(np.float64)


class InjectedDropout(nn.Module):
    def __init__(self, mult):
        super().__init__()
        self.mult = mult

    def forward(self, x):
        return x * self.mult.view(x.shape).to(x.dtype)


def sample_index(name, n):
    """The entries of a sampled tensor and its +-1 vector, reproducible from its name and size (the test draws them again)."""
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + n)
    return np.sort(rng.choice(n, SAMPLE, replace=False)), rng.choice([-1.0, 1.0], n)


CASES = {"2OCJ_A": os.path.join(mg.REF, "examples", "2OCJ.pdb"), "2OCJ_A_gap": os.path.join(HERE, "2OCJ_gap_chainA.pdb")}
GAP_MASKED = 24                                   # residue 120 without its N line
# a case on another weight draw than make_golden's seed 0: (seed, style), and the tags it stores. 2OCJ_A_hot is 2OCJ_A (same mutants
# and targets) from the heavy draw of the 2OCJ_A_hot inference fixture; it stores the drawn-mask run only (half the size of the
# others) and, beside each float64 result, the distance "d32" of the SAME reference evaluated in float32 from it.
WEIGHTS = {"2OCJ_A_hot": (2, "hot")}
TAGS = {"2OCJ_A_hot": ("drawn",)}
CASES["2OCJ_A_hot"] = CASES["2OCJ_A"]


def main(case="2OCJ_A"):
    rng = np.random.default_rng(7)
    pdb = mg.ref_utils.alt_parse_PDB(CASES[case], "A")
    seq = pdb[0]["seq"]
    L = len(seq)
    K = min(48, L)
    if case in ("2OCJ_A", "2OCJ_A_hot"):
        positions = np.sort(rng.choice([i for i in range(L) if seq[i] in AA20], 32, replace=False))
    else:
        assert seq[GAP_MASKED] in AA20 and seq[54:57] == "---"
        positions = np.sort(np.append(rng.choice([i for i in range(L) if seq[i] in AA20 and i != GAP_MASKED], 31, replace=False),
                                      GAP_MASKED))
    muts = []
    for p in positions:
        for a in rng.choice([c for c in AA20 if c != seq[p]], 3, replace=False):
            muts.append(Mutation(int(p), seq[p], str(a), None, "2OCJ"))
    targets = rng.normal(0.0, 1.5, len(muts)).astype(np.float32)
    targets[rng.choice(len(muts), 6, replace=False)] = np.nan
    weight_seed, style = WEIGHTS.get(case, (mg.WEIGHT_SEED, "xavier"))
    out = dict(positions=np.array([m.position for m in muts], np.int32), wildtype=np.array([AA20.index(m.wildtype) for m in muts], np.int32),
               mutation=np.array([AA20.index(m.mutation) for m in muts], np.int32), targets=targets, seed=np.int64(SEED),
               step=np.int64(STEP), weight_seed=np.int64(weight_seed))
    if case in WEIGHTS:
        out["weight_style"] = np.array(style)
    scale = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)
    tf = mg.ref_tm.tied_featurize

    def run(tag, dtype):
        """The reference in ``dtype`` under the masks of ``tag`` -> (loss, {name: flat gradient or None}, E_idx)."""
        with tempfile.TemporaryDirectory() as tmp:
            model = mg.build_reference_model(tmp, weight_seed, style).to(dtype)
        for m, t in zip(muts, targets):
            m.ddG = None if np.isnan(t) else torch.tensor([float(t)], dtype=dtype)
        # ``dtype`` end to end: the featurized inputs are cast, and the one-hot the reference builds with .float() is cast back
        mg.ref_tm.tied_featurize = lambda *a, **k: tuple(t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t for t in tf(*a, **k))
        model.prot_mpnn.features.embeddings.linear.register_forward_pre_hook(lambda mod, args: tuple(x.to(dtype) for x in args))
        for prm in model.parameters():
            prm.requires_grad_(True)
        model.light_attention.dropout = nn.Identity()
        captured = {}
        mpnn = model.prot_mpnn
        for l, layer in enumerate(mpnn.encoder_layers):
            for j, name in enumerate(("dropout1", "dropout2", "dropout3")):
                rows = L * K if j == 2 else L
                m = np.ones((rows, 128)) if tag == "ones" else site_mask(3 * l + j, rows) * scale
                setattr(layer, name, InjectedDropout(torch.from_numpy(m)))
        for l, layer in enumerate(mpnn.decoder_layers):
            for j, name in enumerate(("dropout1", "dropout2")):
                m = np.ones((L, 128)) if tag == "ones" else site_mask(9 + 2 * l + j, L) * scale
                setattr(layer, name, InjectedDropout(torch.from_numpy(m)))
        feat_fwd = mpnn.features.forward

        def spy(*a, **k):
            E, E_idx = feat_fwd(*a, **k)
            captured["E_idx"] = E_idx
            return E, E_idx
        mpnn.features.forward = spy
        model.zero_grad()
        model.train()
        try:
            pred, _ = model([pdb[0]], muts)
        finally:
            mpnn.features.forward = feat_fwd
            mg.ref_tm.tied_featurize = tf
        loss = torch.stack([F.mse_loss(o["ddG"], m.ddG) for m, o in zip(muts, pred) if m.ddG is not None]).mean()
        loss.backward()
        assert loss.dtype == dtype
        grads = {}
        for name, prm in model.named_parameters():
            if name.startswith("prot_mpnn.W_out"):
                assert prm.grad is None
                continue
            grads[name] = (prm.grad if prm.grad is not None else torch.zeros_like(prm)).reshape(-1).double().numpy()
        return loss.item(), grads, captured["E_idx"][0].numpy().astype(np.int32)

    for tag in TAGS.get(case, ("ones", "drawn")):
        loss, grads, E_idx = run(tag, torch.float64)
        out[f"{tag}_loss"] = np.float64(loss)
        out["E_idx"] = E_idx
        for name, g in grads.items():
            if g.size <= FULL_MAX:
                out[f"{tag}|{name}|full"] = g.astype(np.float32)
            else:
                idx, sign = sample_index(name, g.size)
                out[f"{tag}|{name}|val"] = g[idx].astype(np.float32)
                out[f"{tag}|{name}|sumsq"] = np.float64((g * g).sum())
                out[f"{tag}|{name}|dot"] = np.float64((g * sign).sum())
                out[f"{tag}|{name}|absmax"] = np.float64(np.abs(g).max())
        print(f"{tag}: loss {loss:.8f}")
        if case in WEIGHTS:
            loss32, g32, E32 = run(tag, torch.float32)
            assert np.array_equal(E32, E_idx)
            out[f"{tag}_loss_d32"] = np.float64(abs(loss32 - loss) / abs(loss))
            worst = 0.0
            for name, g in grads.items():
                out[f"{tag}|{name}|d32"] = np.float64(np.abs(g32[name] - g).max())
                if np.abs(g).max() > 1e-12:
                    worst = max(worst, float(out[f"{tag}|{name}|d32"]) / float(np.abs(g).max()))
            print(f"{case} {tag}: float32 reference: loss rel. d32 {out[f'{tag}_loss_d32']:.3g}, worst gradient d32 / max|g| {worst:.3g}")
    path = os.path.join(HERE, f"finetune_{case}.npz")
    np.savez_compressed(path, **out)
    print(f"finetune_{case}: {len(muts)} mutants -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main(*sys.argv[1:2])
