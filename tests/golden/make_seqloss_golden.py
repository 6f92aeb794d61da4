"""Golden log-probabilities, loss and gradients of ProteinMPNN's own training objective, by IMPORTING THE REFERENCE's training
flavour (model_utils.ProteinMPNN; runs only in the build container).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_seqloss_golden.py [2OCJ_A | 2OCJ_A_gap | 2OCJ_A_fixed | 2OCJ_A_hot | losses]

The recipe of make_finetune_golden.py: float64, the synthetic ProteinMPNN weights of make_golden (seed 0), K = 48, augment_eps = 0,
train mode, each of the 15 nn.Dropout modules replaced by a module that multiplies by an injected mask: all ones ("ones"), or the
masks of the documented generator of csrc/tmpnn_finetune.hip at seed 7, step 3, times 1 / (1 - thr / 2^24) ("drawn"). The reference
draws its decoding order itself (torch.randn under torch.manual_seed(11), from chain_M and mask in float32 as tied_featurize gives them);
the draw and the order are recorded. Loss = loss_smoothed(S, log_probs, mask * chain_M)[1].

Cases: 2OCJ_A (every residue designable), 2OCJ_A_gap (tests/golden/2OCJ_gap_chainA.pdb: position 24 has mask 0 and keeps its letter,
positions 54-56 are '-', token 20, mask 0), 2OCJ_A_fixed (chain_M = 0 on every third residue: they decode first and are excluded from
the loss), 2OCJ_A_hot (2OCJ_A from the heavy weight draw "hot", seed 2: matrices x 3, biases x 5, LayerNorm gamma in [-2, 2]; the
drawn-mask run only, and beside every float64 result the distance "d32" of the same reference run in float32 from it).

Stored per case: E_idx, randn, decoding_order, chain_M, and per tag log_probs, the loss and per tensor either the full gradient
(<= 4096 entries) or the sample_index sample with the float64 sum of squares, the dot with the seeded +-1 vector and max|g|. Only
tensors are stored, nothing of the reference's source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                          # noqa: E402  (imports the reference, puts the repo on sys.path)
import model_utils as ref_mu                      # noqa: E402  (the reference)
from make_finetune_golden import FULL_MAX, SEED, STEP, InjectedDropout, sample_index, site_mask  # noqa: E402

from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402

ORDER_SEED = 11
CASES = {"2OCJ_A": os.path.join(mg.REF, "examples", "2OCJ.pdb"), "2OCJ_A_gap": os.path.join(HERE, "2OCJ_gap_chainA.pdb"),
         "2OCJ_A_fixed": os.path.join(mg.REF, "examples", "2OCJ.pdb")}


# cases on another weight draw than make_golden's seed 0: (seed, style), and the tags they store. 2OCJ_A_hot is the heavy draw of the
# 2OCJ_A_hot inference fixture; it stores the drawn-mask run only (the file stays at half the size of the others) and, beside each
# float64 result, the distance of the SAME reference evaluated in float32 from it ("d32"): the tests' lines on this draw are set
# against that distance, never against a device's result.
WEIGHTS = {"2OCJ_A_hot": (2, "hot")}
TAGS = {"2OCJ_A_hot": ("drawn",)}
CASES["2OCJ_A_hot"] = CASES["2OCJ_A"]


def main(case="2OCJ_A"):
    entry = mg.ref_utils.alt_parse_PDB(CASES[case], "A")[0]
    # the reference's tied_featurize, as in make_finetune_golden.py (model_utils.featurize has no token for the '-' of a numbering gap)
    feats = mg.ref_utils.tied_featurize([entry], "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask, chain_M, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[4], feats[5], feats[12]
    assert float(chain_M.min()) == 1.0 and chain_M.dtype == mask.dtype == torch.float32
    L = int(S.shape[1])
    K = min(48, L)
    if case == "2OCJ_A_fixed":
        chain_M = chain_M.clone()
        chain_M[0, ::3] = 0.0
    if case == "2OCJ_A_gap":
        assert float(mask[0, 24]) == 0.0 and entry["seq"][54:57] == "---"
    weight_seed, style = WEIGHTS.get(case, (mg.WEIGHT_SEED, "xavier"))
    scale = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)
    out = dict(seed=np.int64(SEED), step=np.int64(STEP), weight_seed=np.int64(weight_seed), chain_M=chain_M[0].numpy())
    if case in WEIGHTS:
        out["weight_style"] = np.array(style)

    def run(tag, dtype):
        """The reference in ``dtype`` under the masks of ``tag`` -> (log_probs, loss, {name: flat gradient}, what the spies saw)."""
        model = ref_mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0, dropout=0.1)
        missing = model.load_state_dict(synthetic_state_dict(weight_seed, "mpnn", style), strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        model = model.to(dtype).train()
        model.features.embeddings.linear.register_forward_pre_hook(lambda mod, args: tuple(x.to(dtype) for x in args))
        captured = {}
        for l, layer in enumerate(model.encoder_layers):
            for j, name in enumerate(("dropout1", "dropout2", "dropout3")):
                rows = L * K if j == 2 else L
                m = np.ones((rows, 128)) if tag == "ones" else site_mask(3 * l + j, rows) * scale
                setattr(layer, name, InjectedDropout(torch.from_numpy(m)))
        for l, layer in enumerate(model.decoder_layers):
            for j, name in enumerate(("dropout1", "dropout2")):
                m = np.ones((L, 128)) if tag == "ones" else site_mask(9 + 2 * l + j, L) * scale
                setattr(layer, name, InjectedDropout(torch.from_numpy(m)))
        feat_fwd, randn, argsort = model.features.forward, torch.randn, torch.argsort

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
        model.features.forward, torch.randn, torch.argsort = spy_features, spy_randn, spy_argsort
        try:
            model.zero_grad()
            torch.manual_seed(ORDER_SEED)
            log_probs = model(X.to(dtype), S, mask, chain_M, residue_idx, chain_enc)
        finally:
            model.features.forward, torch.randn, torch.argsort = feat_fwd, randn, argsort
        _, loss = ref_mu.loss_smoothed(S, log_probs.double(), mask * chain_M)
        loss.backward()
        assert log_probs.dtype == dtype and captured["randn"].shape == chain_M.shape
        grads = {name: (prm.grad if prm.grad is not None else torch.zeros_like(prm)).reshape(-1).double().numpy()
                 for name, prm in model.named_parameters()}
        return log_probs[0].detach().double().numpy(), loss.item(), grads, captured

    for tag in TAGS.get(case, ("ones", "drawn")):
        log_probs, loss, grads, captured = run(tag, torch.float64)
        out["E_idx"] = captured["E_idx"][0].numpy().astype(np.int32)
        out["randn"] = captured["randn"][0].numpy().astype(np.float32)
        out["decoding_order"] = captured["order"][0].numpy().astype(np.int32)
        out[f"{tag}_log_probs"] = log_probs.astype(np.float32)
        out[f"{tag}_loss"] = np.float64(loss)
        for name, g in grads.items():
            if g.size <= FULL_MAX:
                out[f"{tag}|{name}|full"] = g.astype(np.float32)
            else:
                idx, sign = sample_index(name, g.size)
                out[f"{tag}|{name}|val"] = g[idx].astype(np.float32)
                out[f"{tag}|{name}|sumsq"] = np.float64((g * g).sum())
                out[f"{tag}|{name}|dot"] = np.float64((g * sign).sum())
                out[f"{tag}|{name}|absmax"] = np.float64(np.abs(g).max())
        print(f"{case} {tag}: loss {loss:.8f}")
        if case in WEIGHTS:
            lp32, loss32, g32, cap32 = run(tag, torch.float32)
            assert np.array_equal(cap32["order"][0].numpy(), captured["order"][0].numpy())
            live = mask[0].numpy() > 0
            assert np.array_equal(cap32["E_idx"][0].numpy()[live], captured["E_idx"][0].numpy()[live])
            out[f"{tag}_log_probs_d32"] = np.float64(np.abs(lp32 - log_probs).max())
            out[f"{tag}_loss_d32"] = np.float64(abs(loss32 - loss) / abs(loss))
            worst = 0.0
            for name, g in grads.items():
                out[f"{tag}|{name}|d32"] = np.float64(np.abs(g32[name] - g).max())
                worst = max(worst, float(out[f"{tag}|{name}|d32"]) / float(np.abs(g).max()))
            print(f"{case} {tag}: max|log_probs| {np.abs(log_probs).max():.1f}, float32 reference: log_probs d32 {out[f'{tag}_log_probs_d32']:.3g}, "
                  f"loss rel. d32 {out[f'{tag}_loss_d32']:.3g}, worst gradient d32 / max|g| {worst:.3g}")
    path = os.path.join(HERE, f"seqloss_{case}.npz")
    np.savez_compressed(path, **out)
    print(f"seqloss_{case}: L {L} -> {os.path.getsize(path) / 1024:.0f} KiB")


def losses():
    """loss_nll, loss_smoothed and NoamOpt.rate of the reference on seeded random inputs -> seqloss_losses.npz (the host test feeds
    the same inputs to thermompnn_amd.model_utils; the suite itself never imports the reference)."""
    g = torch.Generator().manual_seed(5)
    S = torch.randint(0, 21, (3, 37), generator=g)
    log_probs = torch.log_softmax(torch.randn(3, 37, 21, generator=g), -1)
    mask = (torch.rand(3, 37, generator=g) > 0.2).float()
    nll, nll_av, hits = ref_mu.loss_nll(S, log_probs, mask)
    sm, sm_av = ref_mu.loss_smoothed(S, log_probs, mask)
    _, sm_av3 = ref_mu.loss_smoothed(S, log_probs, mask, weight=0.3)
    steps = np.array([1, 2, 10, 100, 3999, 4000, 4001, 50000], np.int64)
    opt = ref_mu.get_std_opt([torch.nn.Parameter(torch.zeros(1))], 128, 0)
    rates = np.array([opt.rate(int(t)) for t in steps], np.float64)
    adam = opt.optimizer.defaults
    path = os.path.join(HERE, "seqloss_losses.npz")
    np.savez_compressed(path, S=S.numpy(), log_probs=log_probs.numpy(), mask=mask.numpy(), nll=nll.numpy(), nll_av=nll_av.numpy(),
                        hits=hits.numpy(), smoothed=sm.numpy(), smoothed_av=sm_av.numpy(), smoothed_av_w03=sm_av3.numpy(), steps=steps,
                        rates=rates, adam=np.array([adam["lr"], *adam["betas"], adam["eps"]], np.float64))
    print(f"seqloss_losses -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    losses() if sys.argv[1:2] == ["losses"] else main(*sys.argv[1:2])
