"""The weight draws the training tests hold every gradient to (test helper, imported like seqloss_restatement.py; never imported by
the product), with what the host and GPU tests of those draws share.

thermompnn_amd.weights.synthetic_state_dict draws three styles: "xavier" (Xavier-uniform matrices, biases sigma 0.02, LayerNorm gamma
1 +- 0.1), "hot" (matrices x 3, biases x 5, gamma in [-2, 2]: activations to 1e2, |log_probs| to 28, fine-tune losses of 1e3 .. 1e4)
and "wide" (matrices x 8, biases sigma 0.5: activations to 1e4, |log_probs| to 61, losses to 8e7). The case lists below are shared by
the GPU tests (the device against the float64 restatement) and by tests/test_train_weights_host.py (the restatement in float32
against itself in float64, which is what entitles the GPU tests to their lines).
"""
import numpy as np
import torch
from conftest import HOT_F64_FACTOR        # noqa: F401  (2.5: no line sits closer than 2.5 x the reference's own fp32 distance)

RELEASED = dict(hidden_dims=[64, 32], num_final_layers=2, lightattn=True)
NF0 = dict(hidden_dims=[64, 32], num_final_layers=0, lightattn=True)
NO_LA = dict(hidden_dims=[48], num_final_layers=1, lightattn=False)
SCALE = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)      # what a kept entry is multiplied by at p = 0.1 (a 24-bit threshold)

# (layout, k_neighbors, ranks, dropout, style, weight seed): tests/test_gpu_seqloss.py
SEQLOSS_WEIGHT_CASES = [("msk_L40", 48, "perm", False, "hot", 0), ("msk_L40", 48, "perm", True, "hot", 2),
                        ("msk_L40", 48, "perm", False, "wide", 0), ("msk_L40", 48, "perm", False, "xavier", 1),
                        ("msk_L56", 48, "perm", False, "hot", 2), ("msk_L56", 30, "perm", False, "wide", 0),
                        ("msk_L17", 48, "perm", True, "hot", 0), ("msk_L40", 48, "ties", False, "hot", 0),
                        ("msk_L40", 48, "equal", False, "hot", 0)]
# (case, head, subtract_mut, dropout, style, weight seed): tests/test_gpu_finetune.py
FINETUNE_WEIGHT_CASES = [("msk_L40", RELEASED, True, True, "hot", 0), ("msk_L40", RELEASED, False, False, "hot", 2),
                         ("msk_L40", RELEASED, True, False, "wide", 0), ("msk_L56", RELEASED, True, True, "hot", 2),
                         ("msk_L40", NF0, True, False, "hot", 0), ("syn_L17", NO_LA, True, False, "wide", 0),
                         ("msk_L40", RELEASED, True, False, "xavier", 1)]
# the autograd surface's arbitrary upstream gradient (tests/test_gpu_autograd.py): sum(pred * c) on syn_L40, 30 labelled mutants
UPSTREAM_CASE = ("syn_L40", RELEASED, True, "hot", 0)


def seq_id(c):
    return f"{c[0]}-K{c[1]}-{c[2]}-d{int(c[3])}-{c[4]}{c[5]}"


def ft_id(c):
    return f"{c[0]}-nf{c[1]['num_final_layers']}-la{int(c[1]['lightattn'])}-s{int(c[2])}-d{int(c[3])}-{c[4]}{c[5]}"


def mpnn_weights(style, seed):
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(seed, "mpnn", style)


def transfer_weights(head, style, seed):
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(seed, style=style, head=head)


def cpu_protein(pdb, mutations):
    """finetune.MPNNTrainer.prepare without a device: the featurized protein and its labelled mutants as CPU tensors."""
    from thermompnn_amd.datasets import ALPHABET
    from thermompnn_amd.finetune import Protein
    from thermompnn_amd.pdb_io import tied_featurize
    p = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
    f = tied_featurize([p], "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask, cenc, ridx = f[0][0], f[1][0], f[2][0], f[5][0], f[12][0]
    live = [m for m in mutations if m is not None and m.ddG is not None]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return Protein(X.float(), S.to(torch.int32), mask.float(), ridx.to(torch.int32), cenc.to(torch.int32),
                   i32([int(m.position) for m in live]), i32([ALPHABET.index(m.mutation) for m in live]),
                   i32([ALPHABET.index(m.wildtype) for m in live]), torch.tensor([float(m.ddG) for m in live], dtype=torch.float32))


def oracle_graph(X, mask, K):
    """The oracle's k-NN graph [L, min(K, L)] (torch.topk on the adjusted C-alpha distances, in float64)."""
    from oracle import thermompnn_oracle as O
    Xd = torch.as_tensor(np.asarray(X)).double()[None]
    return O.knn(O.backbone_atoms(Xd)[O.CA], torch.as_tensor(np.asarray(mask)).double()[None], K)[1][0].numpy()


def worst_ratio(got, ref):
    """-> (max over tensors of |got - ref| / max|ref|, its tensor) over the tensors whose reference is not a structural zero."""
    worst = {k: float((got[k].double() - r.double()).abs().max()) / float(r.abs().max()) for k, r in ref.items()
             if float(r.abs().max()) > 1e-12}
    name = max(worst, key=worst.get)
    return worst[name], name


def head_restatement(P, x, mut, wt, target, keep, lightattn, n_layers, subtract, p_drop=0.25):
    """The head's training forward and loss under torch.autograd in the dtype of its inputs: LightAttention's centre tap times the
    given dropout mask, [ReLU, Linear] x n_layers, ddg_out, mut - wt, mean squared error. ``P``: {name: leaf}; ``x`` [M, D0] the
    mutants' feature rows. -> (loss, {name: grad})"""
    h = x
    if lightattn:
        h = x @ P["light_attention.feature_convolution.weight"][:, :, 4].T + P["light_attention.feature_convolution.bias"]
        h = h * keep.to(x.dtype) / (1.0 - p_drop)
    for i in range(n_layers):
        h = torch.relu(h) @ P[f"both_out.{2 * i + 1}.weight"].T + P[f"both_out.{2 * i + 1}.bias"]
    out = h * P["ddg_out.weight"].view(()) + P["ddg_out.bias"].view(())
    ar = torch.arange(x.shape[0], device=out.device)
    pred = out[ar, mut] - out[ar, wt] if subtract else out[ar, mut]
    loss = ((pred - target) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in P.items()}


def check_against_golden(g, tag, grads, rel):
    """{name: gradient tensor} against a make_finetune_golden / make_seqloss_golden fixture in its storage scheme (full tensors,
    or a seeded sample with the sum of squares, the signed sum and max|g|), each within ``rel`` x max|g|; -> the worst error / max|g|."""
    from test_gpu_finetune import _golden_sample_index
    worst = 0.0
    for name, gt in grads.items():
        dev = gt.detach().reshape(-1).double().cpu().numpy()
        if f"{tag}|{name}|full" in g:
            ref = g[f"{tag}|{name}|full"].astype(np.float64)
            gmax, err = float(np.abs(ref).max()), float(np.abs(dev - ref).max())
            assert err <= rel * gmax or err <= 1e-12, (tag, name, err, gmax)
        else:
            idx, sign = _golden_sample_index(name, dev.size)
            gmax, sumsq = float(g[f"{tag}|{name}|absmax"]), float(g[f"{tag}|{name}|sumsq"])
            err = float(np.abs(dev[idx] - g[f"{tag}|{name}|val"]).max())
            assert abs(float(np.abs(dev).max()) - gmax) <= rel * gmax, (tag, name)
            assert err <= rel * gmax, (tag, name, err, gmax)
            assert abs(float((dev * dev).sum()) - sumsq) <= rel * sumsq + 1e-20, (tag, name)
            assert abs(float((dev * sign).sum()) - float(g[f"{tag}|{name}|dot"])) <= rel * np.sqrt(dev.size * sumsq) + 1e-12, (tag, name)
        worst = max(worst, err / gmax if gmax > 1e-12 else 0.0)
    return worst
