"""What plain fp32 costs on the training paths at the heavy weight draws (no GPU): the float64 restatements (tests/
seqloss_restatement.py, restate() of tests/test_gpu_finetune.py, the head of tests/train_weight_cases.py) evaluated in float32
against themselves in float64, by torch on the CPU, for every (path, layout, style, seed) the GPU tests hold the device to
(tests/train_weight_cases.py). The GPU tests keep the lines of the Xavier cases on those draws - every gradient within 1e-4 x max|g|,
the fine-tune loss within 1e-5 relative, the head's input rows within 1e-4, the smoothed sequence loss within 1e-6 relative - and
they may only because a correct fp32 evaluation meets each line with a factor of 2.5 to spare (conftest.HOT_F64_FACTOR); that is
asserted here, on the reference alone. Where fp32 does not - log_probs at hot and wide, the head's loss with one mutant - the GPU
test's line is max(the Xavier line, 2.5 x the case's own float32 distance), the distance computed inside that test on the CPU.

Measured (every run prints its own figures; the oracle's k-NN graph, dropout masks of the documented generator at seed 7 step 3 where
the case has dropout (d1), upstream gradient default_rng(1).normal((L, 21)) for the sequence loss, 40 mutants for fine-tuning;
"err32" = |float32 - float64|, for gradients over the worst tensor and divided by its max|g|):

sequence loss                  max|log_probs|  log_probs err32  smoothed loss rel. err32  worst gradient err32 / max|g|
  msk_L40-K48-perm-d0-hot0          21.8           1.11e-5            3.5e-8              1.62e-6  features.edge_embedding.weight
  msk_L40-K48-perm-d1-hot2          28.2           1.53e-5            3.4e-8              2.80e-6  features.embeddings.linear.weight
  msk_L40-K48-perm-d0-wide0         58.3           3.10e-5            2.2e-7              7.53e-6  features.embeddings.linear.weight
  msk_L40-K48-perm-d0-xavier1        8.8           2.44e-6            2.8e-8              1.20e-6  encoder_layers.1.norm1.weight
  msk_L56-K48-perm-d0-hot2          23.2           1.17e-5            3.7e-9              2.24e-6  decoder_layers.0.norm1.weight
  msk_L56-K30-perm-d0-wide0         61.0           3.59e-5            2.3e-8              3.89e-6  features.embeddings.linear.weight
  msk_L17-K48-perm-d1-hot0          22.8           1.16e-5            1.6e-7              4.84e-6  encoder_layers.0.norm1.weight
  msk_L40-K48-ties-d0-hot0          22.0           1.14e-5            3.1e-8              1.93e-6  encoder_layers.0.W1.weight
  msk_L40-K48-equal-d0-hot0         22.0           1.14e-5            3.0e-8              2.04e-6  features.norm_edges.weight
  lines / 2.5                                      4e-6 (Xavier only)  4e-7                4e-5

fine-tune                              loss    loss rel. err32  rows err32  worst gradient err32 / max|g|
  msk_L40-nf2-la1-s1-d1-hot0          2.56e4      2.6e-7         3.15e-6     4.92e-6  prot_mpnn.features.embeddings.linear.weight
  msk_L40-nf2-la1-s0-d0-hot2          3360        5.1e-7         3.47e-6     2.42e-6  prot_mpnn.features.edge_embedding.weight
  msk_L40-nf2-la1-s1-d0-wide0         8.44e7      6.8e-8         2.72e-6     7.19e-6  prot_mpnn.encoder_layers.0.W11.bias
  msk_L56-nf2-la1-s1-d1-hot2          1.01e4      3.1e-8         3.44e-6     3.90e-6  prot_mpnn.features.embeddings.linear.weight
  msk_L40-nf0-la1-s1-d0-hot0          839         2.1e-8         0           4.68e-7  light_attention.feature_convolution.weight
  syn_L17-nf1-la0-s1-d0-wide0         5236        2.8e-7         2.42e-6     1.21e-5  prot_mpnn.features.embeddings.linear.weight
  msk_L40-nf2-la1-s1-d0-xavier1       3.06        4.4e-8         1.72e-6     1.32e-6  prot_mpnn.W_s.weight
  syn_L40 hot0, sum(pred * c)         -81.7       1.4e-6         4.20e-6     4.96e-6  prot_mpnn.features.embeddings.linear.weight
  lines / 2.5                                     4e-6           4e-5        4e-5

head training (hot, seed 2, 2OCJ_A)    loss    loss rel. err32  worst gradient err32 / max|g|
  released, M = 1                     242         1.58e-5        1.50e-5  ddg_out.weight      (outside 1e-5 / 2.5: the 2.5 x rule)
  released, M = 17                    1.15e4      3.9e-7         3.9e-7   both_out.5.bias
  released, M = 64                    9563        8.4e-8         3.4e-7   both_out.1.weight
  no hidden layer, M = 1              46.3        1.8e-7         1.4e-7   both_out.1.weight
  no hidden layer, M = 17             19.6        1.4e-7         7.2e-7   both_out.1.weight
  no hidden layer, M = 64             66.9        9.3e-8         7.8e-8   both_out.1.weight
  lines / 2.5                                     4e-6           4e-6
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from masked_backbones import layout_arrays
from seqloss_restatement import grads_f64, log_probs_f64
from train_weight_cases import (FINETUNE_WEIGHT_CASES, HOT_F64_FACTOR, SCALE, SEQLOSS_WEIGHT_CASES, UPSTREAM_CASE, cpu_protein, ft_id,
                                head_restatement, mpnn_weights, oracle_graph, seq_id, transfer_weights, worst_ratio)

GRAD_LINE, LOSS_LINE, ROWS_LINE, LOG_PROBS_LINE, SMOOTHED_LINE = 1e-4, 1e-5, 1e-4, 1e-5, 1e-6
_DONE = {}


def _smoothed(S, lp, weight_mask):
    from thermompnn_amd.model_utils import loss_smoothed
    return float(loss_smoothed(torch.as_tensor(S).long()[None], lp.double()[None], torch.as_tensor(weight_mask).double()[None])[1])


def seqloss_pair(case):
    """One sequence-loss case in float64 and in float32 -> {dtype: (log_probs, {name: grad})}, S, mask. Computed once per case."""
    if case not in _DONE:
        from test_gpu_finetune import numpy_site_mask
        from test_gpu_seqloss import _ranks
        name, K, kind, dropout, style, seed = case
        X, S, mask, ridx, cenc = layout_arrays(name)
        L = len(S)
        Ei = oracle_graph(X, mask, K)
        Keff = Ei.shape[1]
        assert Keff == min(K, L)
        site_mult = None
        if dropout:
            site_mult = [numpy_site_mask(7, 3, s, L * Keff if s < 9 and s % 3 == 2 else L) * SCALE for s in range(15)]
        dlp = np.random.default_rng(1).normal(size=(L, 21)).astype(np.float32)
        out = {}
        for dt in (torch.float64, torch.float32):
            lp, W = log_probs_f64(mpnn_weights(style, seed), X, S, mask, ridx, cenc, Ei, _ranks(kind, L), site_mult, dtype=dt)
            assert lp.dtype == dt
            out[dt] = (lp.detach(), grads_f64(lp, W, dlp))
        _DONE[case] = (out, S, mask)
    return _DONE[case]


def finetune_pair(case, upstream=False):
    """One fine-tune case in float64 and in float32 -> {dtype: (loss, {name: grad}, rows)}. Computed once per case."""
    key = (ft_id(case), upstream)
    if key not in _DONE:
        from test_gpu_finetune import _case_mutants, _mutants, _pdb, numpy_head_mask, numpy_site_mask
        from thermompnn_amd.finetune import slab_shapes
        name, head, subtract, dropout, style, seed = case
        nf, la = head["num_final_layers"], head["lightattn"]
        with tempfile.TemporaryDirectory() as tmp:
            pdb = _pdb(name, tmp)
        muts = _mutants(pdb, 30, with_none=False) if upstream else _case_mutants(name, pdb)
        prot = cpu_protein(pdb, muts)
        L, K = prot.L, min(48, prot.L)
        Ei = oracle_graph(prot.X, prot.mask, 48)
        rows_of = lambda s: L * K if s < 9 and s % 3 == 2 else L
        site_mult = [(numpy_site_mask(7, 3, s, rows_of(s)) * SCALE if dropout and nf else np.ones((rows_of(s), 128), np.float32))
                     for s in range(15)]
        head_mult = numpy_head_mask(7, 3, prot.M, 128 * nf + 128) / 0.75 if dropout and la else None
        c = np.random.default_rng(4).normal(size=prot.M).astype(np.float32) if upstream else None
        sd = transfer_weights(head, style, seed)
        names = list(slab_shapes(head["hidden_dims"], nf, la))
        _DONE[key] = {dt: restate(sd, names, prot, Ei, site_mult, head_mult, nf, la, subtract, dtype=dt, upstream=c)
                      for dt in (torch.float64, torch.float32)}
    return _DONE[key]


def restate(*a, **k):
    from test_gpu_finetune import restate as r
    return r(*a, **k)


def _check_gradients(tag, g64, g32, must_be_nonzero, cancels=()):
    """``cancels``: tensors whose gradient is analytically zero as a difference of equal sums (ddg_out.bias under subtract_mut:
    d_i - d_i). float64 autograd leaves at most 1e-12 there and the device writes an exact zero; float32 autograd leaves the rounding
    of the two sums (4.8e-6 on terms of 1e3 at hot), which is no property of the mathematics and is not compared."""
    for k, r in g64.items():
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(g32[k]).all()), (tag, k)
        gmax, err = float(r.abs().max()), float((g32[k].double() - r).abs().max())
        if k in cancels:
            assert gmax <= 1e-12, (tag, k, gmax)
            continue
        assert err <= GRAD_LINE * gmax / HOT_F64_FACTOR or err <= 1e-12, (tag, k, err, gmax)
    for k in must_be_nonzero:
        assert float(g64[k].abs().max()) > 0.0, (tag, k)
    return worst_ratio(g32, g64)


@pytest.mark.parametrize("case", SEQLOSS_WEIGHT_CASES, ids=[seq_id(c) for c in SEQLOSS_WEIGHT_CASES])
def test_sequence_loss_gradients_in_fp32_meet_the_line_with_a_factor_to_spare(case):
    """Every gradient of the restatement in float32 is within 1e-4 x max|g| / 2.5 of float64, tensor by tensor (the table in the
    module docstring); log_probs and the smoothed loss are measured and printed: at hot and wide fp32 alone is outside 1e-5 / 2.5
    resp. 1e-6 / 2.5 on them, so the GPU tests take 2.5 x the case's own fp32 distance there, never less than the Xavier line."""
    (out, S, mask), kind = seqloss_pair(case), case[2]
    (lp64, g64), (lp32, g32) = out[torch.float64], out[torch.float32]
    assert bool(torch.isfinite(lp64).all()) and bool(torch.isfinite(lp32).all())
    gammas = [k for k in g64 if ".norm" in k or "norm_edges" in k]
    gammas = [k for k in gammas if k.endswith(".weight")]
    assert len(gammas) == 16
    live = ["W_out.weight", "W_out.bias"] + gammas + ([] if kind == "equal" else ["W_s.weight"])
    worst, where = _check_gradients(seq_id(case), g64, g32, live)
    if kind == "equal":                               # no sequence information reaches the loss: a structural zero, in both dtypes
        assert float(g64["W_s.weight"].abs().max()) == 0.0 == float(g32["W_s.weight"].abs().max())
    lp_err = float((lp32.double() - lp64).abs().max())
    sm64, sm32 = _smoothed(S, lp64, mask), _smoothed(S, lp32, mask)
    print(f"seqloss {seq_id(case)}: max|log_probs| {float(lp64.abs().max()):.1f}, log_probs err32 {lp_err:.3g}, smoothed loss {sm64:.6g} "
          f"rel. err32 {abs(sm32 - sm64) / sm64:.3g}, worst gradient err32 / max|g| {worst:.3g} ({where})")
    assert abs(sm32 - sm64) <= SMOOTHED_LINE * sm64 / HOT_F64_FACTOR       # the smoothed loss keeps its 1e-6 relative on every draw
    if case[4] == "xavier":                           # log_probs: the Xavier line is met by fp32 with the factor to spare, as on seed 0
        assert lp_err <= LOG_PROBS_LINE / HOT_F64_FACTOR


# the autograd test's case in the fine-tune cases' form (no dropout), flagged as the upstream-gradient objective
FT_ALL = [(c, False) for c in FINETUNE_WEIGHT_CASES] + [(UPSTREAM_CASE[:3] + (False,) + UPSTREAM_CASE[3:], True)]


@pytest.mark.parametrize("case,upstream", FT_ALL, ids=[ft_id(c) + ("-upstream" if u else "") for c, u in FT_ALL])
def test_fine_tune_loss_rows_and_gradients_in_fp32_meet_their_lines_with_a_factor_to_spare(case, upstream):
    """restate() in float32 against float64: every gradient within 1e-4 x max|g| / 2.5, the loss within 1e-5 relative / 2.5, the
    head's input rows within 1e-4 / 2.5 (the table in the module docstring). The last case is the autograd test's arbitrary upstream
    gradient: the objective sum(pred * c) instead of the loss."""
    res = finetune_pair(case, upstream)
    (l64, g64, r64), (l32, g32, r32) = res[torch.float64], res[torch.float32]
    nf = case[1]["num_final_layers"]
    assert np.isfinite(l64) and np.isfinite(l32) and bool(torch.isfinite(r32).all())
    gammas = [k for k in g64 if (".norm" in k or "norm_edges" in k) and k.endswith(".weight")]
    assert len(gammas) == (16 if nf else 0)
    worst, where = _check_gradients(ft_id(case), g64, g32, ["prot_mpnn.W_s.weight", "ddg_out.weight"] + gammas,
                                    cancels=("ddg_out.bias",) if case[2] else ())
    loss_err = abs(l32 - l64) / max(abs(l64), 1e-3)
    rows_err = float((r32.double() - r64).abs().max())
    print(f"finetune {ft_id(case)}{' upstream' if upstream else ''}: loss {l64:.4g} rel. err32 {loss_err:.3g}, rows err32 {rows_err:.3g}, "
          f"worst gradient err32 / max|g| {worst:.3g} ({where})")
    assert loss_err <= LOSS_LINE / HOT_F64_FACTOR
    assert rows_err <= ROWS_LINE / HOT_F64_FACTOR


HEAD_LINE = 1e-5                                     # tests/test_gpu_train.py: loss relative, gradients relative to max|g|
_FEATURES = {}


def _hot_feature_rows(pos):
    """[len(pos), 384] rows of the oracle's fp32 forward of 2OCJ chain A at the hot draw of seed 2: the two last decoder states and
    the sequence embedding, as the engine caches them for the head."""
    if "x" not in _FEATURES:
        from oracle import thermompnn_oracle as O
        from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
        pdb = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), "A")
        f = tied_featurize([pdb[0]], "cpu", None, None, None, None, None, None, ca_only=False)
        mp, _ = O.split_weights(transfer_weights(None, "hot", 2))
        with torch.no_grad():
            hidden, h_S, _ = O.mpnn_forward(mp, f[0], f[1], f[2], f[4], f[12], f[5], 48)
        _FEATURES["x"] = torch.cat([hidden[0][0], hidden[1][0], h_S[0]], -1)
        _FEATURES["seq"] = pdb[0]["seq"]
    return _FEATURES["x"][pos], _FEATURES["seq"]


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("head", ["released", "nohidden"])
def test_head_training_in_fp32_meets_its_lines_with_a_factor_to_spare(M, head):
    """The head of tests/test_gpu_train.py's hot cases (hot draw, seed 2, on hot ProteinMPNN features of 2OCJ chain A) in float32
    against float64: from M = 17 on the loss is within 1e-5 relative / 2.5 and every weight gradient within 1e-5 x max|g| / 2.5.
    With M = 1 and the released head it is not: the loss is the square of one difference out[mut] - out[wt] of two outputs of 1e2 ..
    1e3, and float32 alone is 1.58e-5 (loss) and 1.5e-5 (ddg_out.weight) away. The GPU test therefore takes max(1e-5, 2.5 x the
    case's own float32 distance) on these cases, measured on the CPU inside the test."""
    from test_gpu_train import NO_HIDDEN, RELEASED, _many_mutants, numpy_keep_mask
    from thermompnn_amd.datasets import ALPHABET
    from thermompnn_amd.weights import head_param_shapes
    cfg = RELEASED if head == "released" else NO_HIDDEN
    _, seq = _hot_feature_rows([0])
    muts = _many_mutants(seq, M, M)
    x, _ = _hot_feature_rows([m.position for m in muts])
    mut = torch.tensor([ALPHABET.index(m.mutation) for m in muts])
    wt = torch.tensor([ALPHABET.index(m.wildtype) for m in muts])
    target = torch.tensor([float(m.ddG) for m in muts])
    keep = torch.from_numpy(numpy_keep_mask(3, 5, M, 384))
    sd = transfer_weights(cfg, "hot", 2)
    names = list(head_param_shapes(cfg["hidden_dims"], cfg["num_final_layers"], cfg["lightattn"]))
    res = {}
    for dt in (torch.float64, torch.float32):
        P = {k: sd[k].to(dt).clone().requires_grad_(True) for k in names}
        res[dt] = head_restatement(P, x.to(dt), mut, wt, target.to(dt), keep, cfg["lightattn"], len(cfg["hidden_dims"]) + 1, True)
    (l64, g64), (l32, g32) = res[torch.float64], res[torch.float32]
    g64.pop("ddg_out.bias")                           # d_i - d_i: analytically zero (see _check_gradients)
    used = {k: r for k, r in g64.items() if float(r.abs().max()) > 0.0}
    worst, where = worst_ratio(g32, used)
    print(f"head {head} M {M}: loss {l64:.5g} rel. err32 {abs(l32 - l64) / l64:.3g}, max|feature| {float(x.abs().max()):.3g}, "
          f"worst gradient err32 / max|g| {worst:.3g} ({where})")
    assert np.isfinite(l32) and all(bool(torch.isfinite(g).all()) for g in g32.values())
    if M > 1:
        assert abs(l32 - l64) <= HEAD_LINE * l64 / HOT_F64_FACTOR and worst <= HEAD_LINE / HOT_F64_FACTOR
    else:   # one mutant: one difference of ~15 between outputs of <= 1e3 rounded at 2^-24 each (1e3 / 15 x 6e-8 x a few roundings ~ 1e-5),
        # twice that in the square. 1e-4 only keeps the figure sane; the device is held to 2.5 x the float32 distance, not to this.
        assert abs(l32 - l64) <= 1e-4 * l64 and worst <= 1e-4
    assert all(float(g64[f"both_out.{2 * i + 1}.weight"].abs().max()) > 0.0 for i in range(len(cfg["hidden_dims"]) + 1))
