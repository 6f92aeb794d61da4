"""Golden log-probabilities and gradients of a PADDED BATCH OF TWO under ProteinMPNN's training objective, by IMPORTING THE
REFERENCE's training flavour (model_utils.ProteinMPNN; runs only in the build container).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_seqbatch_golden.py

The batch: tests/masked_backbones.py's msk_L40 and msk_L56_2ch padded to 56 rows as featurize pads (zeros, mask 0, chain_M 0 beyond a
member's length). The recipe of make_seqloss_golden.py: float64, the synthetic ProteinMPNN weights of make_golden (seed 0),
k_neighbors = 48, augment_eps = 0, no dropout (eval mode: the 15 nn.Dropout modules are the identity), the same spies on the
featurizer, torch.randn and torch.argsort; the reference draws its decoding order itself (torch.manual_seed(11)) and the draw is
recorded. One more stand-in, for torch.topk inside the featurizer: a padded member has more masked residues than free neighbour slots,
all of them at exactly the row's D_max, and which of them torch.topk lists is its implementation's choice (it is not the same choice
from one torch build to the next). The stand-in is a top-k by a STABLE sort, so the lowest index wins every exact tie: a valid
top-k of the same values, and the rule the device's k-NN documents (DESIGN.md "Ties"). Without it the two graphs differ in which
masked residues they list, and nothing downstream can be compared.
Loss = loss_smoothed(S, log_probs, mask * chain_M)[1], the sum over both members / 2000.

Stored: E_idx [2,56,48], randn, decoding_order, log_probs [2,56,21], the loss, per tensor the gradient in make_seqloss_golden.py's
summary form (tag "eval"), and beside every float64 result the distance "d32" of the SAME reference run in float32 from it. Only
tensors are stored, nothing of the reference's source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                          # noqa: E402  (imports the reference, puts the repo on sys.path)
import model_utils as ref_mu                      # noqa: E402  (the reference)
from make_finetune_golden import FULL_MAX, sample_index  # noqa: E402

from masked_backbones import layout_arrays        # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402

ORDER_SEED = 11
MEMBERS = ("msk_L40", "msk_L56_2ch")
TAG = "eval"


def padded_batch():
    arrs = [layout_arrays(n) for n in MEMBERS]
    Lm = max(len(a[1]) for a in arrs)
    pad = lambda x, dt: torch.stack([torch.cat([torch.as_tensor(v).to(dt), torch.zeros((Lm - len(v),) + v.shape[1:], dtype=dt)]) for v in x])
    X, S, mask = pad([a[0] for a in arrs], torch.float32), pad([a[1] for a in arrs], torch.long), pad([a[2] for a in arrs], torch.float32)
    return X, S, mask, mask.clone(), pad([a[3] for a in arrs], torch.long), pad([a[4] for a in arrs], torch.long)


def run(dtype, batch):
    X, S, mask, chain_M, residue_idx, chain_enc = batch
    model = ref_mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0, dropout=0.1)
    missing = model.load_state_dict(synthetic_state_dict(mg.WEIGHT_SEED, "mpnn"), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model = model.to(dtype).eval()
    model.features.embeddings.linear.register_forward_pre_hook(lambda mod, args: tuple(x.to(dtype) for x in args))
    captured = {}
    feat_fwd, randn, argsort, topk = model.features.forward, torch.randn, torch.argsort, torch.topk

    def stable_topk(x, k, dim=-1, largest=True, sorted=True):
        assert not largest
        idx = torch.sort(x, dim=dim, stable=True).indices.narrow(dim, 0, int(k)).contiguous()
        captured["topk_calls"] = captured.get("topk_calls", 0) + 1
        return torch.gather(x, dim, idx), idx

    def spy_features(*a, **k):
        E, E_idx = feat_fwd(*a, **k)
        captured["E_idx"] = E_idx
        return E, E_idx

    def spy_randn(*a, **k):
        captured["randn"] = randn(*a, **k)
        return captured["randn"]

    def spy_argsort(*a, **k):
        captured["order"] = argsort(*a, **k)
        return captured["order"]
    model.features.forward, torch.randn, torch.argsort, torch.topk = spy_features, spy_randn, spy_argsort, stable_topk
    try:
        model.zero_grad()
        torch.manual_seed(ORDER_SEED)
        log_probs = model(X.to(dtype), S, mask, chain_M, residue_idx, chain_enc)
    finally:
        model.features.forward, torch.randn, torch.argsort, torch.topk = feat_fwd, randn, argsort, topk
    _, loss = ref_mu.loss_smoothed(S, log_probs.double(), mask * chain_M)
    loss.backward()
    assert log_probs.dtype == dtype and captured["randn"].shape == chain_M.shape and captured["topk_calls"] == 1
    grads = {name: (prm.grad if prm.grad is not None else torch.zeros_like(prm)).reshape(-1).double().numpy()
             for name, prm in model.named_parameters()}
    return log_probs.detach().double().numpy(), loss.item(), grads, captured


def main():
    batch = padded_batch()
    mask = batch[2]
    log_probs, loss, grads, captured = run(torch.float64, batch)
    out = dict(weight_seed=np.int64(mg.WEIGHT_SEED), members=np.array(MEMBERS), E_idx=captured["E_idx"].numpy().astype(np.int32),
               randn=captured["randn"].numpy().astype(np.float32), decoding_order=captured["order"].numpy().astype(np.int32))
    out[f"{TAG}_log_probs"] = log_probs.astype(np.float32)
    out[f"{TAG}_loss"] = np.float64(loss)
    for name, g in grads.items():
        if g.size <= FULL_MAX:
            out[f"{TAG}|{name}|full"] = g.astype(np.float32)
        else:
            idx, sign = sample_index(name, g.size)
            out[f"{TAG}|{name}|val"] = g[idx].astype(np.float32)
            out[f"{TAG}|{name}|sumsq"] = np.float64((g * g).sum())
            out[f"{TAG}|{name}|dot"] = np.float64((g * sign).sum())
            out[f"{TAG}|{name}|absmax"] = np.float64(np.abs(g).max())
    lp32, loss32, g32, cap32 = run(torch.float32, batch)
    assert np.array_equal(cap32["order"].numpy(), captured["order"].numpy())
    live = mask.numpy() > 0
    assert np.array_equal(cap32["E_idx"].numpy()[live], captured["E_idx"].numpy()[live])
    out[f"{TAG}_log_probs_d32"] = np.float64(np.abs(lp32 - log_probs).max())
    out[f"{TAG}_loss_d32"] = np.float64(abs(loss32 - loss) / abs(loss))
    worst = 0.0
    for name, g in grads.items():
        out[f"{TAG}|{name}|d32"] = np.float64(np.abs(g32[name] - g).max())
        worst = max(worst, float(out[f"{TAG}|{name}|d32"]) / float(np.abs(g).max()))
    print(f"seqbatch: loss {loss:.8f}, max|log_probs| {np.abs(log_probs).max():.1f}, float32 reference: log_probs d32 "
          f"{out[f'{TAG}_log_probs_d32']:.3g}, loss rel. d32 {out[f'{TAG}_loss_d32']:.3g}, worst gradient d32 / max|g| {worst:.3g}")
    path = os.path.join(HERE, "seqbatch_L40_L56.npz")
    np.savez_compressed(path, **out)
    print(f"seqbatch_L40_L56 -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
