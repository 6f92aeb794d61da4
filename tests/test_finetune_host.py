"""Fine-tuning of ProteinMPNN, host side (no GPU): configuration rules, the slab layout and its AdamW segments, and the C-ABI
entries' argument checks (they refuse before any device call)."""
import ctypes as C

import numpy as np
import pytest

from conftest import REPO  # noqa: F401

HEADS = [([64, 32], 2, True), ([64, 32], 0, True), ([48], 1, False), ([32, 16, 8], 3, True)]


def _cfg(**over):
    from thermompnn_amd.train import Config
    base = dict(datasets=["megascale"], training=dict(learn_rate=1e-3, mpnn_learn_rate=1e-4, epochs=1),
                model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=False, load_pretrained=True,
                           lightattn=True))
    for k, v in over.items():
        base.setdefault(k, {})
        base[k].update(v) if isinstance(v, dict) else base.__setitem__(k, v)
    return Config.wrap(base)


def test_configuration_rules():
    from thermompnn_amd.finetune import check_finetune_config, finetune
    assert check_finetune_config(_cfg()) == 1e-4
    with pytest.raises(ValueError, match="thermompnn_amd.train"):
        finetune(_cfg(model=dict(freeze_weights=True)))
    for bad in (None, "fast", True):
        with pytest.raises(ValueError, match="mpnn_learn_rate"):
            finetune(_cfg(training=dict(mpnn_learn_rate=bad)))
    cfg = _cfg()
    del cfg.training["mpnn_learn_rate"]
    with pytest.raises(ValueError, match="mpnn_learn_rate"):
        finetune(cfg)
    with pytest.raises(NotImplementedError, match="two_stage"):
        finetune(_cfg(training=dict(two_stage=True)))
    with pytest.raises(NotImplementedError, match="reduce"):
        finetune(_cfg(reduce="prot"))


def test_train_still_refuses_the_unfrozen_recipe():
    from thermompnn_amd.train import train
    with pytest.raises(NotImplementedError):
        train(_cfg())


@pytest.mark.parametrize("hidden,nf,la", HEADS)
def test_slab_layout_and_segments(hidden, nf, la):
    from thermompnn_amd import _lib
    from thermompnn_amd.finetune import MAX_SEGMENTS, segment_table, slab_shapes
    from thermompnn_amd.train import SEGMENT_CENTRE, SEGMENT_DECAY, SEGMENT_DENSE
    from thermompnn_amd.weights import head_param_shapes, mpnn_param_shapes
    shapes = slab_shapes(hidden, nf, la)
    names = list(shapes)
    assert not any(k.startswith("prot_mpnn.W_out") for k in names)
    mp = [k for k in names if k.startswith("prot_mpnn.")]
    if nf == 0:
        assert mp == ["prot_mpnn.W_s.weight"]
    else:
        assert mp == ["prot_mpnn." + k for k in mpnn_param_shapes() if not k.startswith("W_out.")] and len(mp) == 116
    assert names[len(mp):] == list(head_param_shapes(hidden, nf, la))
    begins, kinds, groups = segment_table(shapes, True)
    assert len(kinds) <= MAX_SEGMENTS and begins[0] == 0 and begins[-1] == sum(int(np.prod(v)) for v in shapes.values())
    assert groups[0] == "prot_mpnn" and kinds[0] == SEGMENT_DENSE and begins[1] == sum(int(np.prod(shapes[k])) for k in mp)
    head_kinds = dict(zip([k for k in names if not k.startswith("prot_mpnn.")], kinds[1:]))
    if la:
        assert head_kinds["light_attention.attention_convolution.weight"] == SEGMENT_DECAY
        assert head_kinds["light_attention.feature_convolution.weight"] == SEGMENT_CENTRE
    assert head_kinds["ddg_out.bias"] == SEGMENT_DECAY and head_kinds["ddg_out.weight"] == SEGMENT_DENSE
    lib = _lib.load()
    dims = [128 * nf + 128, *hidden, 21]
    cd = (C.c_int32 * len(dims))(*dims)
    assert lib.tmpnn_finetune_slab_numel(nf, int(la), len(dims) - 1, cd) == begins[-1]


def test_learning_rate_per_segment():
    """configure_optimizers: the ProteinMPNN group at mpnn_learn_rate, the head groups at learn_rate (checked without a device)."""
    from thermompnn_amd.finetune import segment_table, slab_shapes
    _, _, groups = segment_table(slab_shapes([64, 32], 2, True), True)
    assert groups == ["prot_mpnn", "light_attention", "light_attention", "light_attention", "light_attention",
                      "both_out", "both_out", "both_out", "both_out", "both_out", "both_out", "ddg_out", "ddg_out"]


def test_mask_layout_matches_the_library():
    from thermompnn_amd import _lib
    from thermompnn_amd.finetune import mask_offsets
    lib = _lib.load()
    for L in (2, 32, 47, 48, 72, 2048):
        assert lib.tmpnn_finetune_mask_numel(L) == mask_offsets(L)[-1] == (12 * L + 3 * L * min(48, L)) * 128
    assert lib.tmpnn_finetune_mask_numel(1) == -1


def test_entries_refuse_bad_arguments_without_a_device():
    from thermompnn_amd import _lib
    lib = _lib.load()
    dims = [384, 64, 32, 21]
    cd = (C.c_int32 * 4)(*dims)
    assert lib.tmpnn_finetune_workspace_bytes(72, 40, 2, 1, 3, cd) > 0
    for L, M in ((1, 40), (0, 40), (72, 0), (72, -1), (10 ** 6, 4)):
        assert lib.tmpnn_finetune_workspace_bytes(L, M, 2, 1, 3, cd) == 0
    bad = (C.c_int32 * 4)(*[300, 64, 32, 21])
    assert lib.tmpnn_finetune_workspace_bytes(72, 40, 2, 1, 3, bad) == 0
    assert lib.tmpnn_finetune_slab_numel(2, 1, 3, bad) == -1
    numel = lib.tmpnn_finetune_slab_numel(2, 1, 3, cd)
    fake = C.c_void_p(0x1000)            # never dereferenced: every check runs before any launch

    def step(**kw):
        a = dict(X=fake, S=fake, mask=fake, ridx=fake, cenc=fake, L=72, pos=fake, mut=fake, wt=fake, target=fake, M=40, nf=2, la=1,
                 nl=3, dims=cd, sub=1, params=fake, grads=fake, numel=numel, pm=0.1, ph=0.25, keep_in=None, keep_out=None, hk=None,
                 seed=0, step=1, loss=fake, pred=None, eidx=None, rows=None, ws=None, wsb=0)
        a.update(kw)
        return lib.tmpnn_finetune_step(*a.values(), None)

    for kw in (dict(X=None), dict(S=None), dict(grads=None), dict(loss=None), dict(L=1), dict(M=0), dict(dims=bad),
               dict(numel=numel - 1), dict(pm=1.0), dict(ph=-0.5), dict(la=0)):
        assert step(**kw) == -1, kw
        assert lib.tmpnn_last_error()
    assert step() == -4                   # TMPNN_E_WORKSPACE: arguments fine, no workspace
    assert lib.tmpnn_finetune_eval(None, fake, fake, fake, fake, 72, fake, fake, fake, 40, 2, 1, 3, cd, 1, fake, numel, fake, None, None,
                                   None, 0, None) == -1


def test_documented_learning_rate_override_is_read_as_a_number(tmp_path):
    """PyYAML reads 1e-4 (no dot) as text; the documented CLI override and the same value in a YAML file are accepted, as
    OmegaConf accepts them in the reference, and non-numeric text is still refused."""
    from thermompnn_amd.finetune import check_finetune_config
    from thermompnn_amd.train import load_config
    base = tmp_path / "config.yaml"
    base.write_text("datasets: [megascale]\ntraining:\n  learn_rate: 1e-3\n  epochs: 1\n"
                    "model:\n  hidden_dims: [64, 32]\n  subtract_mut: true\n  num_final_layers: 2\n  freeze_weights: true\n"
                    "  load_pretrained: true\n  lightattn: true\n")
    cfg = load_config([str(base)], ["model.freeze_weights=false", "training.mpnn_learn_rate=1e-4"])
    assert cfg.training.mpnn_learn_rate == "1e-4"                 # what PyYAML gives
    assert check_finetune_config(cfg) == 1e-4
    local = tmp_path / "local.yaml"
    local.write_text("model:\n  freeze_weights: false\ntraining:\n  mpnn_learn_rate: 3e-5\n")
    assert check_finetune_config(load_config([str(base), str(local)])) == 3e-5
    for bad in ("fast", "nan", "-1e-4", "true"):
        with pytest.raises(ValueError, match="mpnn_learn_rate"):
            check_finetune_config(load_config([str(base)], ["model.freeze_weights=false", f"training.mpnn_learn_rate={bad}"]))


@pytest.mark.parametrize("name", ["msk_L40", "msk_L56"])
def test_masked_backbones_parse_to_the_intended_mask_and_gaps(tmp_path, name):
    """tests/masked_backbones.py: a missing N line keeps the letter with mask 0, a removed residue becomes '-' (token 20)."""
    from masked_backbones import LAYOUTS, expected, write_layout
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    from thermompnn_amd.synthetic import synthetic_backbone
    L, seed, missing_n, gaps = LAYOUTS[name]
    pdb = alt_parse_PDB(write_layout(name, tmp_path), ["A"])
    want_mask, want_gaps = expected(name)
    seq = pdb[0]["seq"]
    _, full = synthetic_backbone(L, seed)
    assert len(seq) == L and [i for i, c in enumerate(seq) if c == "-"] == want_gaps
    assert all(seq[i] == full[i] for i in range(L) if i not in gaps)
    f = tied_featurize(pdb, "cpu", None, None, None, None, None, None, ca_only=False)
    X, S, mask = f[0][0], f[1][0], f[2][0]
    assert mask.tolist() == want_mask
    assert [i for i in range(L) if int(S[i]) == 20] == want_gaps
    assert {0, L - 1} <= set(missing_n) | set(gaps) and sum(want_mask) < L
    assert bool(np.isfinite(X.numpy()).all())                      # NaN coordinates are zeroed once the mask holds them


@pytest.mark.parametrize("case", ["2OCJ_A", "2OCJ_A_hot"])
def test_restatement_reproduces_the_reference_golden(case):
    """restate() of tests/test_gpu_finetune.py in float64 against the imported reference's float64 loss and gradients under the drawn
    dropout masks (tests/golden/make_finetune_golden.py), on the Xavier draw and on the heavy one (hot, seed 2; loss 8682): the GPU
    tests' yardstick computes what the reference computes on both. The loss is stored in float64 and agrees to 1e-12; gradients are
    stored in float32 (2^-24 relative) and agree to 1e-6 x max|g|. On the hot fixture the reference's own float32 distances, which
    the GPU test's lines are set against, are checked to sit inside those lines / 2.5."""
    import os
    import torch
    from conftest import GOLDEN, load_golden
    from test_gpu_finetune import AA20, RELEASED, numpy_site_mask, restate
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.finetune import slab_shapes
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from train_weight_cases import SCALE, check_against_golden, cpu_protein, transfer_weights
    g = load_golden("finetune_" + case)
    pdb = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A"])
    muts = [Mutation(int(p), AA20[w], AA20[m], None if np.isnan(t) else torch.tensor([float(t)]), "2OCJ")
            for p, w, m, t in zip(g["positions"], g["wildtype"], g["mutation"], g["targets"])]
    prot = cpu_protein(pdb, muts)
    L, K = prot.L, 48
    seed, step = int(g["seed"]), int(g["step"])
    mult = [numpy_site_mask(seed, step, s, L * K if s < 9 and s % 3 == 2 else L).astype(np.float64) * SCALE for s in range(15)]
    sd = transfer_weights(RELEASED, str(g["weight_style"]) if "weight_style" in g else "xavier", int(g["weight_seed"]))
    names = list(slab_shapes(RELEASED["hidden_dims"], 2, True))
    loss, grads, _ = restate(sd, names, prot, g["E_idx"].astype(np.int64), mult, None, 2, True, True)
    print(case, "loss", loss, "reference", float(g["drawn_loss"]))
    assert abs(loss - float(g["drawn_loss"])) <= 1e-12 * float(g["drawn_loss"])
    worst = check_against_golden(g, "drawn", grads, 1e-6)
    print(case, "worst gradient distance / max|g|:", worst)
    if case.endswith("_hot"):
        assert str(g["weight_style"]) == "hot" and float(g["drawn_loss"]) > 1e3
        assert float(g["drawn_loss_d32"]) <= 1e-6 / 2.5
        for k, v in grads.items():
            gmax = float(v.abs().max())
            assert float(g[f"drawn|{k}|d32"]) <= 1e-4 / 2.5 * gmax or gmax <= 1e-12, k
