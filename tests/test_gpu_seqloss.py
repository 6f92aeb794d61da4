"""ProteinMPNN's sequence loss on the MI355X (tmpnn_seqloss_forward / _backward, thermompnn_amd.model_utils): the reference's
goldens, a float64 restatement on the layouts where the order predicate can go wrong, consistency with the inference decoder,
determinism and isolation from the ddG path, the autograd surface, and twenty optimiser steps."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from masked_backbones import layout_arrays
from seqloss_restatement import grads_f64, log_probs_f64, split_masks
from test_gpu_finetune import _golden_sample_index, numpy_site_mask
from train_weight_cases import HOT_F64_FACTOR, SEQLOSS_WEIGHT_CASES, mpnn_weights, seq_id

pytestmark = pytest.mark.gpu

# Largest |device - float64 restatement| / max|g| of any tensor over RESTATE_CASES on the first passing run (MI355X; msk_L40 under
# ranks 0..L-1, features.norm_edges.weight): see test_every_gradient_matches_the_float64_restatement. Its bound is twice that, and
# never looser than the 1e-4 x max|g| the fine-tune tests hold the same kernels to (FINETUNE_TOL).
MEASURED_WORST = 2.39e-6
FINETUNE_TOL = 1e-4
GRAD_TOL = min(2 * MEASURED_WORST, FINETUNE_TOL)
SCALE = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)


def _sd(seed=0):
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(seed, "mpnn")


def _shapes():
    from thermompnn_amd.weights import mpnn_param_shapes
    return mpnn_param_shapes()


def _split(flat):
    out, o = {}, 0
    for k, s in _shapes().items():
        n = int(np.prod(s))
        out[k] = flat[o:o + n].view(s)
        o += n
    assert o == flat.numel()
    return out


class Call:
    """tmpnn_seqloss_forward / _backward called directly on one protein (arrays as layout_arrays / tied_featurize give them)."""

    def __init__(self, X, S, mask, ridx, cenc, ranks, K=48, sd=None):
        from thermompnn_amd import _lib
        self.lib = _lib.load()
        dev = "cuda"
        t = lambda a, dt: torch.as_tensor(np.asarray(a)).to(dev, dt).contiguous()
        self.X, self.mask = t(X, torch.float32), t(mask, torch.float32)
        self.S, self.ridx, self.cenc = t(S, torch.int32), t(ridx, torch.int32), t(cenc, torch.int32)
        self.ranks = None if ranks is None else t(ranks, torch.int32)
        self.L, self.K = int(self.S.numel()), K
        self.Keff = min(K, self.L)
        self.slab = torch.cat([v.reshape(-1).float() for v in (sd or _sd()).values()]).cuda()
        self.numel = int(self.lib.tmpnn_seqloss_slab_numel())
        assert self.slab.numel() == self.numel
        self.saved = torch.empty(self.lib.tmpnn_seqloss_saved_bytes(self.L), dtype=torch.uint8, device=dev)
        self.scratch = torch.empty(self.lib.tmpnn_seqloss_scratch_bytes(self.L), dtype=torch.uint8, device=dev)
        self.E_idx = torch.full((self.L, self.Keff), -1, dtype=torch.int32, device=dev)

    def _head(self):
        from thermompnn_amd.train import _ptr
        return (_ptr(self.X), _ptr(self.S), _ptr(self.mask), _ptr(self.ridx), _ptr(self.cenc), self.L, self.K, _ptr(self.ranks),
                _ptr(self.slab), self.numel)

    def forward(self, p=0.0, seed=0, step=0, keep_in=None, keep_out=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        lp = torch.empty((self.L, 21), dtype=torch.float32, device="cuda")
        check(self.lib.tmpnn_seqloss_forward(*self._head(), p, _ptr(keep_in), _ptr(keep_out), seed, step, _ptr(lp), _ptr(self.E_idx),
                                             _ptr(self.saved), self.saved.numel(), _stream()), "tmpnn_seqloss_forward")
        return lp

    def backward(self, dlp, p=0.0, seed=0, step=0, keep_in=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        dlp = torch.as_tensor(dlp).to("cuda", torch.float32).contiguous()
        grads = torch.zeros(self.numel, dtype=torch.float32, device="cuda")
        check(self.lib.tmpnn_seqloss_backward(*self._head(), p, _ptr(keep_in), seed, step, _ptr(dlp), _ptr(grads), _ptr(self.saved),
                                              self.saved.numel(), _ptr(self.scratch), self.scratch.numel(), _stream()),
              "tmpnn_seqloss_backward")
        return grads

    def mask_numel(self):
        return int(self.lib.tmpnn_finetune_mask_numel(self.L))


def _features(src):
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    pdb = alt_parse_PDB(os.path.join(GOLDEN, src), ["A"])
    f = tied_featurize([pdb[0]], "cpu", None, None, None, None, None, None, ca_only=False)
    return pdb, (f[0][0], f[1][0], f[2][0], f[12][0], f[5][0])          # X, S, mask, residue_idx, chain_enc


def _smoothed_and_dlp(S, lp, weight_mask):
    """loss_smoothed on the device's log_probs, summed in float64, and its gradient with respect to log_probs."""
    from thermompnn_amd.model_utils import loss_smoothed
    leaf = lp.detach().cpu().double().requires_grad_(True)
    _, loss = loss_smoothed(torch.as_tensor(S).long()[None], leaf[None], torch.as_tensor(weight_mask).double()[None])
    loss.backward()
    return float(loss.detach()), leaf.grad.float()


# ---- 1. the reference's goldens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["2OCJ_A", "2OCJ_A_gap", "2OCJ_A_fixed", "2OCJ_A_hot"])
def test_log_probs_loss_and_gradients_match_the_reference_golden(case):
    """The imported reference in float64 (tests/golden/make_seqloss_golden.py), all-ones and generator-drawn dropout masks, with the
    criteria test_gpu_finetune.py applies to the same kernels.

    2OCJ_A_hot is 2OCJ_A from the heavy weight draw (hot, seed 2; the drawn masks only; max|log_probs| 29.3). The fixture records how
    far the imported reference ITSELF is from its float64 result when run in float32: log_probs 1.81e-5, loss 4.7e-9 relative, worst
    gradient 1.4e-6 of max|g|. log_probs and the loss are held to max(the Xavier line, 2.5 x that recorded distance) - 4.5e-5 for
    log_probs, the unchanged 1e-6 for the loss - and the gradients to the unchanged 1e-4 x max|g|. First passing run (MI355X):
    log_probs 2.10e-5, loss 1.6e-9 relative, worst gradient 2.05e-6 of max|g|."""
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    g = load_golden("seqloss_" + case)
    _, (X, S, mask, ridx, cenc) = _features("2OCJ_gap_chainA.pdb" if case.endswith("gap") else "2OCJ.pdb")
    chain_M = torch.from_numpy(g["chain_M"])
    ranks = decoding_ranks(chain_M * mask, torch.from_numpy(g["randn"]))
    sd = mpnn_weights(str(g["weight_style"]), int(g["weight_seed"])) if "weight_style" in g else None
    call = Call(X, S, mask, ridx, cenc, ranks, sd=sd)
    L, K = call.L, call.Keff
    seed, step = int(g["seed"]), int(g["step"])
    drawn = np.concatenate([numpy_site_mask(seed, step, s, L * K if s < 9 and s % 3 == 2 else L).reshape(-1) for s in range(15)])
    live = mask.numpy() > 0
    for tag in [t for t in ("ones", "drawn") if f"{t}_loss" in g]:
        kw = dict(keep_in=torch.from_numpy(drawn).cuda(), p=0.1) if tag == "drawn" else dict(p=0.0)
        # a fixture of a heavy draw carries the reference's own float32 distance from its float64 result: the line is 2.5 x that
        lp_line = max(1e-5, HOT_F64_FACTOR * float(g.get(f"{tag}_log_probs_d32", 0.0)))
        loss_line = max(1e-6, HOT_F64_FACTOR * float(g.get(f"{tag}_loss_d32", 0.0)))
        lp = call.forward(seed=seed, step=step, **kw)
        assert np.array_equal(call.E_idx.cpu().numpy()[live], g["E_idx"][live]), "the device's k-NN graph differs from the reference's"
        assert bool(torch.isfinite(lp).all())
        err = float(np.abs(lp.cpu().numpy() - g[f"{tag}_log_probs"]).max())
        print(case, tag, "max |log_probs - reference|:", err, "line", lp_line)
        assert err <= lp_line
        loss, dlp = _smoothed_and_dlp(S, lp, mask * chain_M)
        ref_loss = float(g[f"{tag}_loss"])
        print(case, tag, "loss", loss, "reference", ref_loss)
        assert abs(loss - ref_loss) <= loss_line * abs(ref_loss)
        grads = _split(call.backward(dlp, seed=seed, step=step, **kw))
        assert "W_out.weight" in grads and "W_out.bias" in grads
        worst = 0.0
        for name, gt in grads.items():
            dev = gt.reshape(-1).double().cpu().numpy()
            if f"{tag}|{name}|full" in g:
                ref = g[f"{tag}|{name}|full"].astype(np.float64)
                gmax, e = float(np.abs(ref).max()), float(np.abs(dev - ref).max())
                assert e <= 1e-4 * gmax or e <= 1e-12, (tag, name, e, gmax)
            else:
                idx, sign = _golden_sample_index(name, dev.size)
                gmax = float(g[f"{tag}|{name}|absmax"])
                e = float(np.abs(dev[idx] - g[f"{tag}|{name}|val"]).max())
                assert abs(float(np.abs(dev).max()) - gmax) <= 1e-4 * gmax, (tag, name)
                assert e <= 1e-4 * gmax, (tag, name, e, gmax)
                sumsq = float(g[f"{tag}|{name}|sumsq"])
                assert abs(float((dev * dev).sum()) - sumsq) <= 1e-4 * sumsq + 1e-20, (tag, name)
                assert abs(float((dev * sign).sum()) - float(g[f"{tag}|{name}|dot"])) <= 1e-4 * np.sqrt(dev.size * sumsq) + 1e-12, (tag, name)
            worst = max(worst, e / gmax if gmax > 1e-12 else 0.0)
        for name in ("W_out.weight", "W_out.bias"):
            assert float(grads[name].abs().max()) > 0.0
        print(case, tag, "worst gradient error / max|g|:", worst)


# ---- 2. the float64 restatement ------------------------------------------------------------------------------------------------------
def _ranks(kind, L, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "perm":
        return rng.permutation(L)
    if kind == "ties":
        return rng.integers(0, 5, L)                   # five groups: equal ranks inside a group, invisible both ways
    if kind == "equal":
        return np.full(L, 7)
    assert kind == "arange"
    return np.arange(L)


# (layout, k_neighbors, ranks, dropout)
RESTATE_CASES = [("msk_L17", 48, "perm", True), ("msk_L40", 48, "perm", True), ("msk_L56_2ch", 48, "perm", False),
                 ("msk_L56", 30, "perm", True), ("msk_L40", 48, "ties", False), ("msk_L40", 48, "equal", False),
                 ("msk_L40", 48, "arange", False)]


def _restated(call, arrays, ranks, site_mult, dlp, sd=None):
    X, S, mask, ridx, cenc = arrays
    Ei = call.E_idx.cpu().numpy()
    assert ((Ei >= 0) & (Ei < call.L)).all()
    lp, W = log_probs_f64(sd or _sd(), X, S, mask, ridx, cenc, Ei, ranks, site_mult)
    return lp.detach(), grads_f64(lp, W, dlp)


def _restated_fp32_log_probs(call, arrays, ranks, site_mult, sd):
    """The restatement's forward in float32 on the CPU, on the device's graph: what fp32 alone is away from float64 on this case."""
    X, S, mask, ridx, cenc = arrays
    with torch.no_grad():
        return log_probs_f64(sd, X, S, mask, ridx, cenc, call.E_idx.cpu().numpy(), ranks, site_mult, dtype=torch.float32)[0].double()


@pytest.mark.parametrize("name,K,kind,dropout", RESTATE_CASES, ids=[f"{c[0]}-K{c[1]}-{c[2]}-d{int(c[3])}" for c in RESTATE_CASES])
def test_every_gradient_matches_the_float64_restatement(name, K, kind, dropout):
    """log_probs within 1e-5 and every gradient within GRAD_TOL x max|g| (or 1e-12 on a structural zero) of
    tests/seqloss_restatement.py, from a random dL/dlog_probs on every row (masked rows included).

    Worst error / max|g| per case on the first passing run (MI355X; reruns give the same bits): msk_L17 1.44e-6, msk_L40 1.32e-6,
    msk_L56_2ch 1.01e-6, msk_L56 at K = 30 1.56e-6, ties 1.78e-6, all ranks equal 1.65e-6, ranks 0..L-1 2.39e-6 (the largest:
    MEASURED_WORST); log_probs errors 2.3e-6 .. 3.6e-6. Every run prints its own figures."""
    arrays = layout_arrays(name)
    X, S, mask, ridx, cenc = arrays
    L = len(S)
    ranks = _ranks(kind, L)
    call = Call(X, S, mask, ridx, cenc, ranks, K)
    Keff = call.Keff
    assert Keff == min(K, L)
    keep_out = torch.full((call.mask_numel(),), -1.0, device="cuda") if dropout else None
    lp = call.forward(p=0.1 if dropout else 0.0, seed=7, step=3, keep_out=keep_out)
    dlp = torch.from_numpy(np.random.default_rng(1).normal(size=(L, 21)).astype(np.float32))
    grads = _split(call.backward(dlp, p=0.1 if dropout else 0.0, seed=7, step=3))
    site_mult = None
    if dropout:
        keep = split_masks(keep_out.cpu().numpy(), L, Keff)
        assert all(set(np.unique(k).tolist()) <= {0.0, 1.0} for k in keep) and 0.85 < float(np.mean(keep[2])) < 0.95
        for s in range(15):                            # the in-kernel masks are the documented generator's
            assert np.array_equal(keep[s], numpy_site_mask(7, 3, s, keep[s].shape[0])), s
        site_mult = [k * SCALE for k in keep]
    ref_lp, ref = _restated(call, arrays, ranks, site_mult, dlp)
    assert bool(torch.isfinite(lp).all())
    lp_err = float((lp.cpu().double() - ref_lp).abs().max())
    assert lp_err <= 1e-5, lp_err
    worst = {}
    for k, gt in grads.items():
        d, r = gt.cpu().double(), ref[k]
        gmax, err = float(r.abs().max()), float((d - r).abs().max())
        worst[k] = err / gmax if gmax > 1e-12 else 0.0
        assert err <= GRAD_TOL * gmax or err <= 1e-12, (k, err, gmax)
    print(f"{name}-K{K}-{kind}: log_probs error {lp_err:.3g}, worst gradient error / max|g|: {max(worst.values()):.3g}",
          max(worst, key=worst.get))
    if kind == "equal":                                # every edge invisible: no sequence information reaches the loss
        assert float(grads["W_s.weight"].abs().max()) == 0.0
        for l in range(3):
            assert float(grads[f"decoder_layers.{l}.W1.weight"][:, 256:384].abs().max()) == 0.0
            assert float(grads[f"decoder_layers.{l}.W1.weight"][:, 384:].abs().max()) > 0.0
    else:
        assert float(grads["W_s.weight"].abs().max()) > 0.0
    if name.startswith("msk_"):                        # a masked row is finite and carries the bias-only distribution
        dead = np.nonzero(mask == 0)[0]
        assert len(dead) and bool(torch.equal(lp[dead[0]], lp[dead[-1]]))


@pytest.mark.parametrize("name,K,kind,dropout,style,seed", SEQLOSS_WEIGHT_CASES, ids=[seq_id(c) for c in SEQLOSS_WEIGHT_CASES])
def test_every_gradient_matches_the_float64_restatement_on_heavy_weight_draws(name, K, kind, dropout, style, seed):
    """The body of test_every_gradient_matches_the_float64_restatement away from the Xavier draw of seed 0: "hot" weights (matrices
    x 3, biases x 5, LayerNorm gamma in [-2, 2]; |log_probs| to 28), "wide" weights (matrices x 8; |log_probs| to 61) and a second
    Xavier seed. gelu' sees saturated and strongly negative pre-activations, the LayerNorm backward negative and large gamma, the
    log-softmax backward rows whose probabilities span e^-60 .. 1.

    Every gradient within FINETUNE_TOL x max|g| (or 1e-12 on a structural zero): GRAD_TOL was measured on the Xavier cases and the
    restatement in float32 alone is at 7.5e-6 at wide (tests/test_train_weights_host.py, which also asserts that float32 meets
    FINETUNE_TOL / 2.5 on each of these cases). log_probs within max(1e-5, 2.5 x |restatement float32 - restatement float64|), the
    float32 side computed here on the CPU on the device's graph: float32 alone is 1.1e-5 .. 1.5e-5 from float64 at hot and
    3.1e-5 .. 3.6e-5 at wide.

    First passing run (MI355X), in the order of SEQLOSS_WEIGHT_CASES - worst device gradient error / max|g| (the restatement's own
    float32 figure from the host test), then the device's log_probs error (the float32 restatement's in the same run):
    hot 0 2.21e-6 (1.62e-6), 1.61e-5 (1.01e-5); hot 2 with dropout 3.28e-6 (2.80e-6), 1.38e-5 (1.40e-5); wide 0 9.21e-6 (7.53e-6),
    2.91e-5 (2.71e-5); xavier 1 1.29e-6 (1.20e-6), 2.71e-6 (1.82e-6); msk_L56 hot 2 2.15e-6 (2.24e-6), 1.91e-5 (9.83e-6); msk_L56 at
    K = 30 wide 0 3.59e-6 (3.89e-6), 3.72e-5 (2.46e-5); msk_L17 hot 0 with dropout 7.33e-6 (4.84e-6), 1.50e-5 (8.99e-6); ties
    1.88e-6 (1.93e-6), 1.13e-5 (9.22e-6); all ranks equal 2.88e-6 (2.04e-6), 1.51e-5 (1.01e-5). Every run prints its own figures."""
    arrays = layout_arrays(name)
    X, S, mask, ridx, cenc = arrays
    L = len(S)
    ranks = _ranks(kind, L)
    sd = mpnn_weights(style, seed)
    call = Call(X, S, mask, ridx, cenc, ranks, K, sd=sd)
    Keff = call.Keff
    assert Keff == min(K, L)
    keep_out = torch.full((call.mask_numel(),), -1.0, device="cuda") if dropout else None
    lp = call.forward(p=0.1 if dropout else 0.0, seed=7, step=3, keep_out=keep_out)
    dlp = torch.from_numpy(np.random.default_rng(1).normal(size=(L, 21)).astype(np.float32))
    grads = _split(call.backward(dlp, p=0.1 if dropout else 0.0, seed=7, step=3))
    site_mult = None
    if dropout:
        keep = split_masks(keep_out.cpu().numpy(), L, Keff)
        for s in range(15):                            # the in-kernel masks are the documented generator's
            assert np.array_equal(keep[s], numpy_site_mask(7, 3, s, keep[s].shape[0])), s
        site_mult = [k * SCALE for k in keep]
    ref_lp, ref = _restated(call, arrays, ranks, site_mult, dlp, sd=sd)
    fp32_dist = float((_restated_fp32_log_probs(call, arrays, ranks, site_mult, sd) - ref_lp).abs().max())
    lp_line = max(1e-5, HOT_F64_FACTOR * fp32_dist)
    assert bool(torch.isfinite(lp).all())
    lp_err = float((lp.cpu().double() - ref_lp).abs().max())
    worst = {}
    for k, gt in grads.items():
        d, r = gt.cpu().double(), ref[k]
        gmax, err = float(r.abs().max()), float((d - r).abs().max())
        worst[k] = err / gmax if gmax > 1e-12 else 0.0
    print(f"{seq_id((name, K, kind, dropout, style, seed))}: max|log_probs| {float(ref_lp.abs().max()):.1f}, log_probs error {lp_err:.3g} "
          f"(restatement float32 {fp32_dist:.3g}, line {lp_line:.3g}), worst gradient error / max|g|: {max(worst.values()):.3g}",
          max(worst, key=worst.get))
    assert lp_err <= lp_line, (lp_err, lp_line)
    for k, gt in grads.items():
        d, r = gt.cpu().double(), ref[k]
        gmax, err = float(r.abs().max()), float((d - r).abs().max())
        assert err <= FINETUNE_TOL * gmax or err <= 1e-12, (k, err, gmax)
    if kind == "equal":                                # every edge invisible: no sequence information reaches the loss
        assert float(grads["W_s.weight"].abs().max()) == 0.0
        for l in range(3):
            assert float(grads[f"decoder_layers.{l}.W1.weight"][:, 256:384].abs().max()) == 0.0
            assert float(grads[f"decoder_layers.{l}.W1.weight"][:, 384:].abs().max()) > 0.0
    else:
        assert float(grads["W_s.weight"].abs().max()) > 0.0
    dead = np.nonzero(mask == 0)[0]                    # a masked row is finite and carries the bias-only distribution
    assert len(dead) and bool(torch.equal(lp[dead[0]], lp[dead[-1]]))


# ---- 3. forward consistency with inference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["msk_L40", "msk_L56"])
def test_eval_forward_agrees_with_the_inference_decoder(name):
    from thermompnn_amd.engine import Engine
    X, S, mask, ridx, cenc = layout_arrays(name)
    L = len(S)
    from thermompnn_amd.weights import synthetic_state_dict
    eng = Engine(synthetic_state_dict(0), "cuda:0", 48, precision="fp32", retry_precision=None)   # (same ProteinMPNN draw as _sd())
    t = lambda a, dt: torch.as_tensor(a).to("cuda", dt)
    offsets = torch.tensor([0, L], dtype=torch.int32)
    enc = eng.encode(t(X, torch.float32), t(mask, torch.float32), t(ridx, torch.int32), t(cenc, torch.int32), offsets, max_len=L)
    for kind in ("perm", "ties", "equal"):
        ranks = _ranks(kind, L)
        want = eng.decode_ordered(enc, t(S, torch.int32)[None], t(ranks, torch.int32)[None], want_log_probs=True)["log_probs"][0]
        got = Call(X, S, mask, ridx, cenc, ranks).forward()
        err = float((got - want).abs().max())
        print(name, kind, "max |seqloss - decode_ordered|:", err)
        assert err <= 1e-5
    allvis = eng.ssm_forward(t(X, torch.float32), t(S, torch.int32), t(mask, torch.float32), t(ridx, torch.int32), t(cenc, torch.int32),
                             offsets, max_len=L, want_ddg=False, want_log_probs=True)["log_probs"]
    got = Call(X, S, mask, ridx, cenc, None).forward()                     # ranks NULL: every neighbour visible
    err = float((got - allvis).abs().max())
    print(name, "max |seqloss(all visible) - ssm_forward|:", err)
    assert err <= 1e-5


# ---- 4. determinism and isolation ----------------------------------------------------------------------------------------------------
def test_reruns_replayed_masks_and_the_ddg_step_keep_their_bits(tmp_path):
    from test_gpu_finetune import _model, _mutants, _pdb
    from thermompnn_amd.finetune import MPNNTrainer
    tr = MPNNTrainer(_model(tmp_path), seed=7)
    pdb = _pdb("msk_L40", tmp_path)
    prot = tr.prepare([(pdb, _mutants(pdb, 24))])[0]
    tr.grad.zero_()
    loss_a = tr.forward_backward(prot, step=3).clone()
    ddg_a = tr.grad.clone()

    arrays = layout_arrays("msk_L40")
    L = len(arrays[1])
    ranks = _ranks("perm", L)
    dlp = torch.from_numpy(np.random.default_rng(2).normal(size=(L, 21)).astype(np.float32))
    a, b = Call(*arrays, ranks), Call(*arrays, ranks)
    keep_out = torch.empty(a.mask_numel(), device="cuda")
    lp_a = a.forward(p=0.1, seed=5, step=9, keep_out=keep_out)
    g_a = a.backward(dlp, p=0.1, seed=5, step=9)
    lp_b = b.forward(p=0.1, seed=5, step=9)
    g_b = b.backward(dlp, p=0.1, seed=5, step=9)
    assert torch.equal(lp_a, lp_b) and torch.equal(g_a, g_b)               # two runs, separate buffers
    assert torch.equal(a.backward(dlp, p=0.1, seed=5, step=9), g_a)        # a second backward over the same saved buffer
    assert 0.85 < float(keep_out.mean()) < 0.95
    lp_c = b.forward(p=0.1, seed=99, step=1, keep_in=keep_out)             # the drawn masks replayed as injected ones
    g_c = b.backward(dlp, p=0.1, seed=99, step=1, keep_in=keep_out)
    assert torch.equal(lp_c, lp_a) and torch.equal(g_c, g_a)
    assert not torch.equal(b.forward(p=0.1, seed=6, step=9), lp_a)         # another key draws other masks

    tr.grad.zero_()
    loss_b = tr.forward_backward(prot, step=3)
    assert torch.equal(loss_a, loss_b) and torch.equal(tr.grad, ddg_a)     # the ddG step is untouched by the calls in between


# ---- 5. the autograd surface -----------------------------------------------------------------------------------------------------
def _module(k_neighbors=48, dropout=0.0, sd=None):
    from thermompnn_amd import model_utils as mu
    model = mu.ProteinMPNN(k_neighbors=k_neighbors, augment_eps=0.0, dropout=dropout)
    model.load_state_dict(sd or _sd())
    return model.cuda()


def _batch(names):
    """Padded batch of layouts, as featurize pads: zeros, mask 0, chain_M 0 beyond a member's length."""
    arrs = [layout_arrays(n) for n in names]
    Lm = max(len(a[1]) for a in arrs)
    pad = lambda x, dt: torch.stack([torch.cat([torch.as_tensor(v).to(dt), torch.zeros((Lm - len(v),) + v.shape[1:], dtype=dt)]) for v in x])
    X, S, mask = pad([a[0] for a in arrs], torch.float32), pad([a[1] for a in arrs], torch.long), pad([a[2] for a in arrs], torch.float32)
    ridx, cenc = pad([a[3] for a in arrs], torch.long), pad([a[4] for a in arrs], torch.long)
    return [t.cuda() for t in (X, S, mask, mask.clone(), ridx, cenc)]


def test_module_backward_fills_every_grad_with_the_c_abi_gradients():
    _module_backward_equals_the_c_abi("xavier", 0)


def test_module_backward_fills_every_grad_with_the_c_abi_gradients_on_a_hot_draw():
    """The same bit equality from the heavy draw (hot, seed 2): the module hands the kernels the weights it holds, whatever they are."""
    _module_backward_equals_the_c_abi("hot", 2)


def _module_backward_equals_the_c_abi(style, seed):
    from thermompnn_amd import model_utils as mu
    from thermompnn_amd.autograd import dropout_key
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    sd = mpnn_weights(style, seed)
    model = _module(dropout=0.1, sd=sd).train()
    X, S, mask, chain_M, ridx, cenc = _batch(["msk_L40"])
    randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(4)).cuda()
    with dropout_key(5, 9):
        lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
    assert lp.shape == (1, 40, 21) and lp.requires_grad
    loss = mu.loss_smoothed(S, lp, mask * chain_M)[1]
    loss.backward()
    ranks = decoding_ranks(chain_M * mask, randn)[0].cpu().numpy()
    call = Call(*layout_arrays("msk_L40"), ranks, sd=sd)
    lp_c = call.forward(p=0.1, seed=5, step=9)
    assert torch.equal(lp_c, lp[0].detach())
    leaf = lp_c.clone().requires_grad_(True)
    mu.loss_smoothed(S, leaf[None], mask * chain_M)[1].backward()
    want = _split(call.backward(leaf.grad, p=0.1, seed=5, step=9))
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, want[k]), k
    with torch.no_grad():                              # no graph: the same entry, nothing kept for a backward
        assert not model(X, S, mask, chain_M, ridx, cenc, randn=randn).requires_grad
    model.eval()
    lp_eval = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
    assert torch.equal(lp_eval[0].detach(), call.forward())                # eval mode: no dropout
    drawn = model(X, S, mask, chain_M, ridx, cenc)                         # an order of its own
    assert not torch.equal(drawn, lp_eval)


def test_autograd_grad_with_a_random_upstream_gradient_matches_the_restatement():
    model = _module(k_neighbors=30).eval()
    arrays = layout_arrays("msk_L56")
    X, S, mask, chain_M, ridx, cenc = _batch(["msk_L56"])
    randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(8)).cuda()
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    ranks = decoding_ranks(chain_M * mask, randn)[0].cpu().numpy()
    lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
    dlp = torch.from_numpy(np.random.default_rng(6).normal(size=(56, 21)).astype(np.float32))
    params = dict(model.named_parameters())
    got = torch.autograd.grad(lp, list(params.values()), grad_outputs=dlp.cuda()[None])
    call = Call(*arrays, ranks, 30)
    call.forward()
    ref_lp, ref = _restated(call, arrays, ranks, None, dlp)
    assert float((lp[0].detach().cpu().double() - ref_lp).abs().max()) <= 1e-5
    for (k, _), gt in zip(params.items(), got):
        gmax, err = float(ref[k].abs().max()), float((gt.cpu().double() - ref[k]).abs().max())
        assert err <= FINETUNE_TOL * gmax or err <= 1e-12, (k, err, gmax)      # (a case outside RESTATE_CASES: the fine-tune tests' line)
    assert all(p.grad is None for p in params.values())                    # torch.autograd.grad leaves .grad alone


def test_padded_batch_members_contribute_what_their_single_calls_do():
    from thermompnn_amd import model_utils as mu
    model = _module().eval()
    X, S, mask, chain_M, ridx, cenc = _batch(["msk_L40", "msk_L17"])
    assert X.shape[:2] == (2, 40) and float(mask[1, 17:].abs().max()) == 0.0
    randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(9)).cuda()
    lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
    losses = mu.loss_smoothed(S, lp, mask * chain_M)[0] * mask * chain_M
    params = list(model.parameters())
    both = torch.autograd.grad(losses.sum(), params, retain_graph=True)
    singles = []
    for b in range(2):
        sl = slice(b, b + 1)
        lp_b = model(X[sl], S[sl], mask[sl], chain_M[sl], ridx[sl], cenc[sl], randn=randn[sl])
        assert torch.equal(lp_b[0], lp[b])
        l_b = (mu.loss_smoothed(S[sl], lp_b, (mask * chain_M)[sl])[0] * (mask * chain_M)[sl]).sum()
        singles.append(torch.autograd.grad(l_b, params))
        member = torch.autograd.grad(losses[b].sum(), params, retain_graph=True)
        assert all(torch.equal(x, y) for x, y in zip(member, singles[b])), b
    assert all(torch.equal(t, x + y) for t, x, y in zip(both, *singles))


def test_transfer_model_joint_loss_accumulates_both_backwards(tmp_path):
    from test_gpu_autograd import _loss, _model
    from test_gpu_finetune import _mutants, _pdb
    from thermompnn_amd import model_utils as mu
    from thermompnn_amd.autograd import dropout_key
    model = _model(tmp_path)
    pdb = _pdb("msk_L40", tmp_path)
    muts = _mutants(pdb, 16)
    with pytest.raises(RuntimeError, match="differentiable"):
        model.sequence_log_probs(pdb)
    model.differentiable = True
    model.train()
    _, S, mask, _, _ = layout_arrays("msk_L40")
    S, mask = torch.as_tensor(S).cuda(), torch.as_tensor(mask).cuda()
    randn = torch.randn(40, generator=torch.Generator().manual_seed(2))
    grads = {}
    for which in ("ddg", "seq", "joint"):
        model.zero_grad(set_to_none=True)
        with dropout_key(3, 4):
            if which in ("ddg", "joint"):
                pred, _ = model(pdb, muts)
                _loss(pred, muts).backward()
            if which == "ddg":
                assert model.prot_mpnn.W_out.weight.grad is None           # the ddG Function's behaviour is untouched
            if which in ("seq", "joint"):
                lp = model.sequence_log_probs(pdb, randn=randn)
                assert lp.shape == (40, 21)
                mu.loss_smoothed(S[None], lp[None], mask[None])[1].backward()
        grads[which] = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    for k, j in grads["joint"].items():
        d, s = grads["ddg"][k], grads["seq"][k]
        want = d + s if d is not None and s is not None else d if d is not None else s
        assert (j is None and want is None) or torch.equal(j, want), k
    assert grads["seq"]["prot_mpnn.W_out.weight"] is not None and float(grads["seq"]["prot_mpnn.W_out.bias"].abs().max()) > 0
    assert grads["seq"]["ddg_out.weight"] is None


# ---- 6. it learns ---------------------------------------------------------------------------------------------------------------
# The float64 restatement's smoothed loss over the same twenty steps (tests/seqloss_restatement.py under torch.optim.Adam on the CPU,
# same weights, backbone, order and optimiser settings), recorded once.
F64_LOSSES = [0.0696355, 0.0750301, 0.0720872, 0.0687927, 0.0617797, 0.0567146, 0.0558795, 0.0544738, 0.0544858, 0.0545648, 0.0540642,
              0.0533028, 0.0527801, 0.0526643, 0.0525354, 0.052103, 0.0515112, 0.0509264, 0.0503773, 0.0497844]
_LEARN = {}


def _twenty_steps(style="xavier", seed=0):
    """Twenty steps of get_std_opt's Adam (betas 0.9 / 0.98, eps 1e-9) at a fixed lr of 1e-3 on one L = 40 synthetic backbone, no
    dropout, one fixed order, from the synthetic weights (style, seed) -> the smoothed loss before each step. Run once per start."""
    if (style, seed) not in _LEARN:
        from thermompnn_amd import model_utils as mu
        from thermompnn_amd.synthetic import AA20, synthetic_backbone
        from thermompnn_amd.weights import synthetic_state_dict
        model = _module(sd=synthetic_state_dict(seed, "mpnn", style)).train()         # dropout 0.0
        Xn, seq = synthetic_backbone(40, 5)
        X = torch.from_numpy(Xn.astype(np.float32))[None].cuda()
        S = torch.tensor([AA20.index(c) for c in seq])[None].cuda()
        mask = torch.ones(1, 40).cuda()
        ridx, cenc = torch.arange(40)[None].cuda(), torch.ones(1, 40, dtype=torch.long).cuda()
        randn = torch.randn(1, 40, generator=torch.Generator().manual_seed(1)).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            loss = mu.loss_smoothed(S, model(X, S, mask, mask, ridx, cenc, randn=randn), mask)[1]
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        print(f"smoothed loss over 20 steps ({style}, seed {seed}):", [round(v, 7) for v in losses])
        _LEARN[style, seed] = losses
    return _LEARN[style, seed]


def test_twenty_adam_steps_follow_the_float64_trajectory():
    """Training through the Function moves the weights as the float64 mathematics does (Xavier-scale weights of seed 0): every one of
    the twenty losses within 1e-3 relative of the restatement's. Why 1e-3: a step's fp32 loss is within ~1e-6 relative of float64
    (log_probs errors of 3e-6 on values of ~3); Adam normalises each gradient entry, so an entry at fp32 noise level may step the
    other way, but such an entry moves the loss by |g| lr, far below 1e-3 of it; the trajectory's own features (the rise of 7.7 % at
    step 2, the plateau of steps 8-10) are ten to a hundred times larger than the line."""
    losses = _twenty_steps()
    for i, (a, b) in enumerate(zip(losses, F64_LOSSES)):
        assert abs(a - b) <= 1e-3 * b, (i, a, b)


def test_smoothed_loss_falls_over_twenty_adam_steps():
    """The smoothed loss falls monotonically over the first five steps and ends below half its start.

    The start is the suite's heavy weight draw ("hot": matrices x 3, biases x 5), seed 2, and it was chosen on the float64
    restatement alone (tests/seqloss_restatement.py under the same optimiser on the CPU), before the device ran it. Twenty steps at
    lr 1e-3 cannot halve a loss that starts at the uniform prediction's: from Xavier-scale weights the loss starts at 0.070 (uniform:
    40 ln 21 / 2000 = 0.061) and the float64 trajectory is F64_LOSSES above, which rises at step 2 (Adam's first update moves every
    parameter by the full 1e-3 whatever its gradient) and ends at 0.715 of its start; seeds 1-3 and the module's own initialisation
    end at 0.59 .. 0.74 in float64, each with a rise in the first three steps. From an over-confident start there is that much to
    learn: the heavy draw starts at 0.17 .. 0.23 and in float64 meets both criteria at seeds 1, 2 and 3 (seed 0 rises at step 3),
    seed 2 with the widest margins: 0.23108, 0.18396, 0.14521, 0.11714, 0.09736, 0.08717, ... 0.05537 (each of the five steps falls
    by 10 % or more, end / start 0.24)."""
    losses = _twenty_steps("hot", 2)
    assert all(b < a for a, b in zip(losses[:5], losses[1:6])), losses[:6]
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
