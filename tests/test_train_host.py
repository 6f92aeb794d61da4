"""Head training, host side (no GPU): Mega-scale reader, refused configurations, C-ABI argument checks, checkpoint naming and the
ReduceLROnPlateau wiring of thermompnn_amd.train."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from conftest import REPO  # noqa: F401

RELEASED_DIMS = [384, 64, 32, 21]


def _cfg(**over):
    from thermompnn_amd.train import Config
    base = dict(datasets=["megascale"], training=dict(learn_rate=1e-3, epochs=1),
                model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=True, load_pretrained=True,
                           lightattn=True))
    for k, v in over.items():
        base.setdefault(k, {})
        if isinstance(v, dict):
            base[k].update(v)
        else:
            base[k] = v
    return Config.wrap(base)


def _write_megascale(tmp_path, rows, seq):
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    X, _ = synthetic_backbone(len(seq), 3)
    pdbs = tmp_path / "pdbs"
    pdbs.mkdir()
    (pdbs / "prot1:A.pdb").write_text(backbone_pdb_text(X, seq))      # WT_name 'prot1|A.pdb': '.pdb' stripped, '|' -> ':'
    with open(tmp_path / "mega.csv", "w") as fh:
        fh.write("name,ddG_ML,mut_type,WT_name,aa_seq,dG_ML,extra\n")
        for r in rows:
            fh.write(",".join(["x", *r, "1.0", "z"]) + "\n")
    with open(tmp_path / "splits.pkl", "wb") as fh:
        pickle.dump({"train": ["prot1|A.pdb"], "val": ["prot1|A.pdb"], "test": []}, fh)
    return _cfg(data_loc=dict(megascale_csv=str(tmp_path / "mega.csv"), megascale_splits=str(tmp_path / "splits.pkl"),
                              megascale_pdbs=str(pdbs)))


def _mut_seq(seq, i, a):
    return seq[:i] + a + seq[i + 1:]


def test_megascale_dataset_filters_sign_and_positions(tmp_path):
    from thermompnn_amd.datasets import MegaScaleDataset
    seq = "ACDEFGHIKLMNPQ"
    rows = [("0.0", "wt", "prot1|A.pdb", seq),
            ("1.5", "A1G", "prot1|A.pdb", _mut_seq(seq, 0, "G")),
            ("-0.25", "E4W", "prot1|A.pdb", _mut_seq(seq, 3, "W")),
            ("-", "C2A", "prot1|A.pdb", _mut_seq(seq, 1, "A")),                    # unreliable: dropped
            ("0.7", "insG5", "prot1|A.pdb", seq), ("0.7", "delK9", "prot1|A.pdb", seq),
            ("0.3", "A1G:E4W", "prot1|A.pdb", seq),                               # double mutant: dropped
            ("2.0", "Q14R", "other|B.pdb", seq)]                                  # another protein, not in the split
    cfg = _write_megascale(tmp_path, rows, seq)
    ds = MegaScaleDataset(cfg, "train")
    assert len(ds) == 1
    pdb, muts = ds[0]
    assert pdb[0]["seq"] == seq
    assert [(m.position, m.wildtype, m.mutation) for m in muts] == [(0, "A", "G"), (3, "E", "W")]
    assert [float(m.ddG) for m in muts] == [-1.5, 0.25]                          # ddG = -ddG_ML
    assert all(m.pdb == "prot1:A" for m in muts)


def test_megascale_dataset_checks_the_wild_type(tmp_path):
    from thermompnn_amd.datasets import ComboDataset, MegaScaleDataset
    seq = "ACDEFGHIKLMNPQ"
    cfg = _write_megascale(tmp_path, [("0.0", "wt", "prot1|A.pdb", seq), ("1.0", "D2G", "prot1|A.pdb", _mut_seq(seq, 1, "G"))], seq)
    with pytest.raises(AssertionError, match="wild type"):
        MegaScaleDataset(cfg, "val")[0]
    combo = ComboDataset(cfg, "train")
    assert len(combo) == 1


def test_unsupported_recipes_are_refused():
    from thermompnn_amd.train import train
    for cfg in (_cfg(model=dict(freeze_weights=False)), _cfg(training=dict(mpnn_learn_rate=1e-3)),
                _cfg(training=dict(two_stage=True)), _cfg(reduce="prot")):
        with pytest.raises(NotImplementedError):
            train(cfg)


def test_config_merge_and_overrides(tmp_path):
    from thermompnn_amd.train import load_config
    (tmp_path / "a.yaml").write_text("training:\n  learn_rate: 0.001\n  epochs: 100\nmodel:\n  hidden_dims: [64, 32]\n")
    (tmp_path / "b.yaml").write_text("training:\n  epochs: 5\nplatform:\n  accel: gpu\n")
    cfg = load_config([str(tmp_path / "a.yaml"), str(tmp_path / "b.yaml")], ["training.learn_rate=0.01", "name=run1"])
    assert cfg.training.learn_rate == 0.01 and cfg.training.epochs == 5 and cfg.model.hidden_dims == [64, 32]
    assert cfg.platform.accel == "gpu" and cfg.name == "run1"


def test_training_entries_reject_bad_arguments_without_a_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    dims = (C.c_int32 * 4)(*RELEASED_DIMS)
    numel = 2 * (384 * 384 * 9 + 384) + 384 * 64 + 64 + 64 * 32 + 32 + 32 * 21 + 21 + 2
    assert lib.tmpnn_head_slab_numel(2, 1, 3, dims) == numel
    assert lib.tmpnn_head_slab_numel(2, 0, 3, dims) == numel - 2 * (384 * 384 * 9 + 384)
    assert lib.tmpnn_head_slab_numel(1, 1, 3, dims) == -1                      # D0 must be 128 * n_final + 128
    assert lib.tmpnn_head_train_workspace_bytes(100, 2, 1, 3, dims) > 100 * 384 * 4
    assert lib.tmpnn_head_train_workspace_bytes(100, 3, 1, 3, dims) == 0
    p = C.c_void_p(256)
    args = lambda **o: dict(dict(feat=p, n_feat=10, rows=p, mut=p, wt=p, target=p, M=5, n_final=2, la=1, n_layers=3, dims=dims, sub=1,
                                 params=p, grads=p, numel=numel, p_drop=0.25, keep_in=None, keep_out=None, ws=p, wsb=1 << 30), **o)

    def step(a):
        return lib.tmpnn_head_train_step(a["feat"], a["n_feat"], a["rows"], a["mut"], a["wt"], a["target"], a["M"], a["n_final"], a["la"],
                                         a["n_layers"], a["dims"], a["sub"], a["params"], a["grads"], a["numel"], a["p_drop"],
                                         a["keep_in"], a["keep_out"], 0, 1, p, None, a["ws"], a["wsb"], None)
    for bad, msg in ((dict(numel=numel - 1), b"slab"), (dict(n_final=1), b"dims"), (dict(feat=None), b"null"),
                     (dict(p_drop=1.0), b"dropout"), (dict(la=0, numel=numel - 2 * (384 * 384 * 9 + 384)), b"LightAttention"),
                     (dict(keep_in=p, keep_out=p), b"exclude"), (dict(M=0), b"at least one"), (dict(M=-3), b"mutants"),
                     (dict(n_feat=0), b"feature rows")):
        assert step(args(**bad)) == -1, bad
        assert msg in lib.tmpnn_last_error(), (bad, lib.tmpnn_last_error())
    assert step(args(wsb=16)) == -4 and b"workspace" in lib.tmpnn_last_error()
    assert lib.tmpnn_head_eval(p, 10, p, p, p, 0, 2, 1, 3, dims, 1, p, numel, p, p, 0, None) == 0   # nothing to predict
    assert lib.tmpnn_head_eval(p, 10, p, p, p, 4, 2, 1, 3, dims, 1, p, numel + 1, p, p, 1 << 30, None) == -1

    beg = (C.c_int64 * 3)(0, 10, 20)
    kind = (C.c_int32 * 2)(1, 0)
    lr = (C.c_double * 2)(1e-3, 1e-3)
    adam = lambda n=20, nseg=2, b=beg, k=kind, step=1, b1=0.9: lib.tmpnn_adamw_step(p, p, p, p, n, nseg, b, k, lr, b1, 0.999, 1e-8, 0.01,
                                                                                     step, None)
    assert adam(n=21) == -1 and b"cover" in lib.tmpnn_last_error()
    assert adam(nseg=0) == -1 and b"segments" in lib.tmpnn_last_error()
    assert adam(step=0) == -1 and b"step" in lib.tmpnn_last_error()
    assert adam(b1=1.0) == -1 and b"hyper" in lib.tmpnn_last_error()
    assert adam(k=(C.c_int32 * 2)(1, 7)) == -1 and b"kind" in lib.tmpnn_last_error()
    assert adam(b=(C.c_int64 * 3)(0, 25, 20)) == -1 and b"negative length" in lib.tmpnn_last_error()


def test_checkpoint_name_follows_lightning():
    from thermompnn_amd.train import checkpoint_name
    assert checkpoint_name("test", 3, 0.5312) == "test_epoch=03_val_ddG_spearman=0.53.ckpt"
    assert checkpoint_name("run", 12, -0.0471) == "run_epoch=12_val_ddG_spearman=-0.047.ckpt"


def test_reduce_lr_on_plateau_wiring():
    """ReduceLROnPlateau(mode='min', factor=0.5, patience=10): a flat validation MSE halves every group's lr on the 12th epoch."""
    from thermompnn_amd.train import make_scheduler
    sched = make_scheduler({"light_attention": 1e-3, "both_out": 1e-3, "ddg_out": 1e-3})
    lrs = []
    for mse in [2.0, 1.0] + [1.0] * 20:
        sched.step(mse)
        lrs.append(sched.optimizer.param_groups[0]["lr"])
    assert all(pg["lr"] == lrs[-1] for pg in sched.optimizer.param_groups)
    assert lrs[:12] == [1e-3] * 12 and lrs[12] == 5e-4
    assert lrs[12:] == [5e-4] * 10


def test_training_kernels_are_in_the_build():
    from thermompnn_amd import build
    assert "tmpnn_train.hip" in build.SOURCES
    text = open(os.path.join(os.path.dirname(build.__file__), "csrc", "tmpnn_train.hip")).read()
    assert "atomicAdd" not in text and "getenv" not in text and "hipMalloc" not in text
    assert text.count("\n") < 1300


def test_train_golden_fixture_is_small_and_complete():
    path = os.path.join(REPO, "tests", "golden", "train_2OCJ_A.npz")
    assert os.path.getsize(path) <= 800 * 1024
    with np.load(path) as z:
        assert {"ones_loss", "p25_loss", "keep_p25", "ones_conv_center", "p25_both_out.5.weight", "p25_ddg_out.weight"} <= set(z.files)
        assert np.isnan(z["targets"]).sum() >= 1 and len(np.unique(z["positions"])) < len(z["positions"])
