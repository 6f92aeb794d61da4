"""ProteinMPNN's sequence loss, host side (no GPU): the C-ABI entries' sizers and argument checks (they refuse before any device
call), the losses and the schedule against values recorded from the reference (tests/golden/make_seqloss_golden.py), the module's
state-dict names and the fixtures' decoding order."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

E_WORKSPACE = -4                                    # TMPNN_E_WORKSPACE (include/tmpnn.h)
NEW = ("tmpnn_seqloss_slab_numel", "tmpnn_seqloss_saved_bytes", "tmpnn_seqloss_scratch_bytes", "tmpnn_seqloss_forward",
       "tmpnn_seqloss_backward")


def _lib():
    from thermompnn_amd import _lib, build
    build.build_library()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound():
    from test_cabi import declared_symbols
    from thermompnn_amd import _lib as L
    lib = _lib()
    names = declared_symbols()
    for n in NEW:
        assert n in names and n in L.SIGNATURES and hasattr(lib, n), n


def test_slab_is_the_whole_state_dict_and_sizers_grow_with_length():
    from thermompnn_amd.weights import mpnn_param_shapes
    lib = _lib()
    shapes = mpnn_param_shapes()
    assert list(shapes)[-2:] == ["W_out.weight", "W_out.bias"]
    assert lib.tmpnn_seqloss_slab_numel() == sum(int(np.prod(s)) for s in shapes.values())
    # the fine-tune slab is unchanged: ProteinMPNN without W_out, then the released head
    dims = (C.c_int32 * 4)(384, 64, 32, 21)
    assert lib.tmpnn_finetune_slab_numel(2, 1, 3, dims) - lib.tmpnn_head_slab_numel(2, 1, 3, dims) == \
        lib.tmpnn_seqloss_slab_numel() - 21 * 128 - 21
    for sizer in (lib.tmpnn_seqloss_saved_bytes, lib.tmpnn_seqloss_scratch_bytes):
        assert sizer(1) == 0 and sizer(0) == 0 and sizer(-5) == 0 and sizer(8193) == 0
        sizes = [sizer(L) for L in (2, 3, 16, 17, 40, 47, 48, 49, 56, 194, 1024, 8192)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # what the backward reads: the graph, 416 features and >= 20 [E,128] activations per edge, log_probs
    assert lib.tmpnn_seqloss_saved_bytes(40) > 40 * 40 * (416 + 20 * 128) * 4 + 40 * 21 * 4


def test_argument_errors_come_before_any_launch():
    lib = _lib()
    n = lib.tmpnn_seqloss_slab_numel()
    p = C.c_void_p(256)                            # never dereferenced: every call below is refused first
    sv, sc = lib.tmpnn_seqloss_saved_bytes(40), lib.tmpnn_seqloss_scratch_bytes(40)

    def fwd(L=40, K=48, numel=n, p_mpnn=0.1, keep_in=None, keep_out=None, lp=p, saved=p, saved_bytes=sv, X=p):
        return lib.tmpnn_seqloss_forward(X, p, p, p, p, L, K, None, p, numel, p_mpnn, keep_in, keep_out, 0, 0, lp, None, saved, saved_bytes,
                                         None)

    def bwd(L=40, K=48, numel=n, dlp=p, grads=p, saved=p, saved_bytes=sv, scratch=p, scratch_bytes=sc):
        return lib.tmpnn_seqloss_backward(p, p, p, p, p, L, K, p, p, numel, 0.0, None, 0, 0, dlp, grads, saved, saved_bytes, scratch,
                                          scratch_bytes, None)
    err = lambda: lib.tmpnn_last_error()
    for L in (1, 0, 8193):
        assert fwd(L=L) == -1 and b"outside [2, 8192]" in err()
        assert bwd(L=L) == -1 and b"outside [2, 8192]" in err()
    for K in (0, 49, -1):
        assert fwd(K=K) == -1 and b"k_neighbors" in err()
        assert bwd(K=K) == -1 and b"k_neighbors" in err()
    assert fwd(numel=n - 21) == -1 and b"slab" in err()
    assert bwd(numel=n + 1) == -1 and b"slab" in err()
    assert fwd(X=None) == -1 and b"null pointer" in err()
    assert fwd(lp=None) == -1 and b"null pointer" in err()
    assert bwd(dlp=None) == -1 and b"null pointer" in err()
    assert bwd(grads=None) == -1 and b"null pointer" in err()
    assert fwd(p_mpnn=1.0) == -1 and b"dropout" in err()
    assert fwd(keep_in=p, keep_out=p) == -1 and b"exclude each other" in err()
    assert fwd(saved_bytes=sv - 1) == E_WORKSPACE and b"saved" in err()
    assert fwd(saved=None) == E_WORKSPACE and b"saved" in err()
    assert bwd(saved_bytes=sv - 1) == E_WORKSPACE and b"saved" in err()
    assert bwd(scratch_bytes=sc - 1) == E_WORKSPACE and b"scratch" in err()
    assert bwd(scratch=None) == E_WORKSPACE and b"scratch" in err()


def test_losses_and_schedule_equal_the_recorded_reference_values():
    from thermompnn_amd import model_utils as mu
    g = load_golden("seqloss_losses")
    S, lp, mask = torch.from_numpy(g["S"]), torch.from_numpy(g["log_probs"]), torch.from_numpy(g["mask"])
    nll, nll_av, hits = mu.loss_nll(S, lp, mask)
    assert np.array_equal(nll.numpy(), g["nll"]) and float(nll_av) == float(g["nll_av"]) and np.array_equal(hits.numpy(), g["hits"])
    sm, sm_av = mu.loss_smoothed(S, lp, mask)
    assert np.array_equal(sm.numpy(), g["smoothed"]) and float(sm_av) == float(g["smoothed_av"])
    assert float(sm_av) == float((sm * mask).sum() / 2000.0)                      # the fixed divisor
    assert float(mu.loss_smoothed(S, lp, mask, weight=0.3)[1]) == float(g["smoothed_av_w03"])
    opt = mu.get_std_opt([torch.nn.Parameter(torch.zeros(1))], 128, 0)
    assert isinstance(opt, mu.NoamOpt) and isinstance(opt.optimizer, torch.optim.Adam)
    d = opt.optimizer.defaults
    assert [d["lr"], *d["betas"], d["eps"]] == list(g["adam"])
    assert [opt.rate(int(t)) for t in g["steps"]] == list(g["rates"])
    w = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
    opt = mu.NoamOpt(128, 2, 4000, torch.optim.SGD([w], lr=0.0), 9)
    w.grad = torch.ones(1, dtype=torch.float64)
    opt.step()
    assert opt._step == 10 and opt.param_groups[0]["lr"] == opt.rate(10) == float(g["rates"][2])
    assert float(w.detach()) == 1.0 - opt.rate(10)                                # the step ran at the new rate
    opt.zero_grad()
    assert w.grad is None or float(w.grad) == 0.0


def test_module_shares_its_state_dict_with_the_inference_class():
    from thermompnn_amd import model_utils as mu
    from thermompnn_amd import protein_mpnn_utils as pu
    from thermompnn_amd.weights import synthetic_state_dict
    train = mu.ProteinMPNN(k_neighbors=48, augment_eps=0.0)
    infer = pu.ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
    a, b = train.state_dict(), infer.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert {k for k, _ in train.named_parameters()} == set(a)
    sd = synthetic_state_dict(0, "mpnn")
    assert not train.load_state_dict(sd, strict=True).missing_keys
    assert not infer.load_state_dict(train.state_dict(), strict=True).missing_keys
    assert all(torch.equal(infer.state_dict()[k], sd[k]) for k in sd)
    # the reference's defaults, and the rules of this build
    d = mu.ProteinMPNN()
    assert (d.k_neighbors, d.augment_eps, d.dropout) == (32, 0.1, 0.1)
    for bad in (dict(k_neighbors=0), dict(k_neighbors=49), dict(dropout=0.2), dict(hidden_dim=64), dict(num_decoder_layers=2)):
        with pytest.raises(NotImplementedError):
            mu.ProteinMPNN(**bad)
    assert mu.ProteinMPNN(dropout=0.0, k_neighbors=1).dropout == 0.0
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), os.pardir, "compat"))
    try:
        import model_utils as compat_mu
    finally:
        sys.path.pop(0)
    for name in ("ProteinMPNN", "loss_nll", "loss_smoothed", "NoamOpt", "get_std_opt", "featurize"):
        assert getattr(compat_mu, name) is getattr(mu, name), name


@pytest.mark.parametrize("case", ["2OCJ_A", "2OCJ_A_gap", "2OCJ_A_fixed"])
def test_decoding_ranks_reproduce_the_order_the_reference_drew(case):
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    g = load_golden("seqloss_" + case)
    src = "2OCJ_gap_chainA.pdb" if case.endswith("gap") else "2OCJ.pdb"
    feats = tied_featurize([alt_parse_PDB(os.path.join(GOLDEN, src), ["A"])[0]], "cpu", None, None, None, None, None, None, ca_only=False)
    mask = feats[2][0]
    chain_M = torch.from_numpy(g["chain_M"])
    ranks = decoding_ranks(chain_M * mask, torch.from_numpy(g["randn"])).numpy()
    order = g["decoding_order"]
    L = len(order)
    assert sorted(order.tolist()) == list(range(L)) and np.array_equal(ranks[order], np.arange(L))
    first = (chain_M * mask).numpy() == 0                                     # fixed and masked residues decode first
    assert first.sum() == {"2OCJ_A": 0, "2OCJ_A_gap": 4, "2OCJ_A_fixed": 65}[case]
    assert set(order[:int(first.sum())].tolist()) == set(np.nonzero(first)[0].tolist())


@pytest.mark.parametrize("case", ["2OCJ_A", "2OCJ_A_hot"])
def test_restatement_reproduces_the_reference_golden(case):
    """tests/seqloss_restatement.py in float64 against the imported reference's float64 results under the drawn dropout masks, on
    the Xavier draw and on the heavy one (hot, seed 2): the GPU tests' yardstick computes what the reference computes, also where
    activations reach 1e2 and |log_probs| 29. The fixtures store float32 (2^-24 relative: 1.8e-6 on a log-probability of 29, 6e-8 of
    max|g|), so log_probs agree to 4e-6 and gradients to 1e-6 x max|g|; the loss is stored in float64 and agrees to 1e-12. The hot
    fixture's float32 distances are the figures the GPU test's docstring quotes."""
    from seqloss_restatement import log_probs_f64
    from test_gpu_finetune import numpy_site_mask
    from thermompnn_amd.model_utils import loss_smoothed
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    from thermompnn_amd.weights import synthetic_state_dict
    from train_weight_cases import SCALE, check_against_golden
    g = load_golden("seqloss_" + case)
    f = tied_featurize([alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A"])[0]], "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask, ridx, cenc = f[0][0], f[1][0], f[2][0], f[12][0], f[5][0]
    L, K = len(S), 48
    ranks = decoding_ranks(torch.from_numpy(g["chain_M"]) * mask, torch.from_numpy(g["randn"])).numpy()
    seed, step = int(g["seed"]), int(g["step"])
    mult = [numpy_site_mask(seed, step, s, L * K if s < 9 and s % 3 == 2 else L).astype(np.float64) * SCALE for s in range(15)]
    sd = synthetic_state_dict(int(g["weight_seed"]), "mpnn", str(g["weight_style"]) if "weight_style" in g else "xavier")
    lp, W = log_probs_f64(sd, X.numpy(), S.numpy(), mask.numpy(), ridx.numpy(), cenc.numpy(), g["E_idx"], ranks, mult)
    err = float(np.abs(lp.detach().numpy() - g["drawn_log_probs"]).max())
    loss = loss_smoothed(S.long()[None], lp[None], (mask * torch.from_numpy(g["chain_M"])).double()[None])[1]
    print(case, "max|log_probs|", float(lp.detach().abs().max()), "restatement - reference:", err, "loss", float(loss.detach()),
          float(g["drawn_loss"]))
    assert err <= 4e-6
    assert abs(float(loss.detach()) - float(g["drawn_loss"])) <= 1e-12 * float(g["drawn_loss"])
    for v in W.values():
        v.grad = None
    loss.backward()
    worst = check_against_golden(g, "drawn", {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in W.items()}, 1e-6)
    print(case, "worst gradient distance / max|g|:", worst)
    if case.endswith("_hot"):
        assert str(g["weight_style"]) == "hot" and float(np.abs(g["drawn_log_probs"]).max()) > 20.0
        assert 1e-6 < float(g["drawn_log_probs_d32"]) < 1e-4 and float(g["drawn_loss_d32"]) <= 1e-6 / 2.5
        assert all(float(g[f"drawn|{k}|d32"]) <= 1e-4 / 2.5 * float(v.grad.abs().max()) for k, v in W.items())


def test_cpu_model_raises_the_device_error():
    from thermompnn_amd import model_utils as mu
    model = mu.ProteinMPNN(augment_eps=0.0)
    X = torch.zeros(1, 5, 4, 3)
    one, idx = torch.ones(1, 5), torch.arange(5)[None]
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(X, torch.zeros(1, 5, dtype=torch.long), one, one, idx, torch.ones(1, 5, dtype=torch.long))
