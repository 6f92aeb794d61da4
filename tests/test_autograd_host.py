"""The autograd split of fine-tuning, host side (no GPU): the split C-ABI entries refuse bad arguments before any launch, their buffer
sizes cover the fused path's, and compat's TransferModelPL.configure_optimizers builds the reference's parameter groups."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

from conftest import REPO

DIMS = [384, 64, 32, 21]
FAKE = C.c_void_p(0x1000)            # never dereferenced: every check runs before any launch


def _cd(dims=DIMS):
    return (C.c_int32 * len(dims))(*dims)


def _forward(lib, **kw):
    cd = _cd()
    numel = lib.tmpnn_finetune_slab_numel(2, 1, 3, cd)
    a = dict(X=FAKE, S=FAKE, mask=FAKE, ridx=FAKE, cenc=FAKE, L=72, pos=FAKE, mut=FAKE, wt=FAKE, M=40, nf=2, la=1, nl=3, dims=cd, sub=1,
             params=FAKE, numel=numel, pm=0.1, ph=0.25, keep_in=None, keep_out=None, hk=None, seed=0, step=1, pred=FAKE, eidx=None,
             rows=None, saved=None, saved_bytes=0)
    a.update(kw)
    return lib.tmpnn_finetune_forward(*a.values(), None)


def _backward(lib, **kw):
    cd = _cd()
    numel = lib.tmpnn_finetune_slab_numel(2, 1, 3, cd)
    big = 1 << 40
    a = dict(X=FAKE, S=FAKE, mask=FAKE, ridx=FAKE, cenc=FAKE, L=72, pos=FAKE, mut=FAKE, wt=FAKE, M=40, nf=2, la=1, nl=3, dims=cd, sub=1,
             params=FAKE, numel=numel, pm=0.1, ph=0.25, keep_in=None, hk=None, seed=0, step=1, dpred=FAKE, grads=FAKE, mpnn=1,
             saved=FAKE, saved_bytes=big, scratch=None, scratch_bytes=0)
    a.update(kw)
    return lib.tmpnn_finetune_backward(*a.values(), None)


def test_split_entries_refuse_bad_arguments_without_a_device():
    from thermompnn_amd import _lib
    lib = _lib.load()
    bad = _cd([300, 64, 32, 21])
    for kw in (dict(X=None), dict(S=None), dict(mask=None), dict(pos=None), dict(params=None), dict(pred=None), dict(L=1), dict(L=8193),
               dict(M=0), dict(dims=bad), dict(numel=7), dict(pm=1.0), dict(ph=-0.5), dict(la=0), dict(keep_in=FAKE, keep_out=FAKE),
               dict(nf=0, dims=_cd([128, 64, 32, 21]), numel=0)):
        assert _forward(lib, **kw) == -1, kw
        assert lib.tmpnn_last_error()
    assert _forward(lib) == -4                                    # TMPNN_E_WORKSPACE: arguments fine, no saved buffer
    need = lib.tmpnn_finetune_saved_bytes(72, 40, 2, 1, 3, _cd())
    assert _forward(lib, saved=FAKE, saved_bytes=need - 1) == -4
    for kw in (dict(X=None), dict(dpred=None), dict(grads=None), dict(params=None), dict(L=1), dict(L=10 ** 6), dict(M=0),
               dict(dims=bad), dict(pm=1.5), dict(la=0), dict(nf=0, dims=_cd([128, 64, 32, 21]), numel=0, keep_in=FAKE)):
        assert _backward(lib, **kw) == -1, kw
    assert _backward(lib) == -4                                   # no scratch buffer
    assert _backward(lib, saved=None, scratch=FAKE, scratch_bytes=1 << 40) == -4
    assert _backward(lib, saved_bytes=need - 1, scratch=FAKE, scratch_bytes=1 << 40) == -4
    scratch = lib.tmpnn_finetune_scratch_bytes(72, 40, 2, 1, 3, _cd())
    assert _backward(lib, scratch=FAKE, scratch_bytes=scratch - 1) == -4


@pytest.mark.parametrize("L,M,nf,la,hidden", [(2, 1, 2, 1, [64, 32]), (40, 37, 2, 1, [64, 32]), (72, 300, 0, 1, [64, 32]),
                                              (256, 900, 3, 1, [32]), (1024, 50, 1, 0, [48])])
def test_saved_and_scratch_cover_the_fused_workspace(L, M, nf, la, hidden):
    from thermompnn_amd import _lib
    lib = _lib.load()
    cd = _cd([128 * nf + 128, *hidden, 21])
    nl = len(hidden) + 1
    fused = lib.tmpnn_finetune_workspace_bytes(L, M, nf, la, nl, cd)
    saved = lib.tmpnn_finetune_saved_bytes(L, M, nf, la, nl, cd)
    scratch = lib.tmpnn_finetune_scratch_bytes(L, M, nf, la, nl, cd)
    assert fused > 0 and saved > 0 and scratch > 0
    assert saved + scratch >= fused
    assert saved < fused and scratch < fused                      # each is a real part of the whole
    for bad in ((1, M), (L, 0), (8193, M)):
        assert lib.tmpnn_finetune_saved_bytes(*bad, nf, la, nl, cd) == 0
        assert lib.tmpnn_finetune_scratch_bytes(*bad, nf, la, nl, cd) == 0


def _compat_module():
    """compat/train_thermompnn.py as the reference's drivers import it (compat/ on the path, without shadowing this process's
    modules): its `_repo` helper first, then the module itself under a private name."""
    compat = os.path.join(REPO, "compat")
    if "_repo" not in sys.modules:
        spec = importlib.util.spec_from_file_location("_repo", os.path.join(compat, "_repo.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sys.modules["_repo"] = mod
    spec = importlib.util.spec_from_file_location("compat_train_thermompnn", os.path.join(compat, "train_thermompnn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pl(tmp_path, freeze=False, lightattn=True, lr_schedule=None):
    from thermompnn_amd import weights
    from thermompnn_amd.train import Config
    head = dict(hidden_dims=[64, 32], num_final_layers=2, lightattn=lightattn)
    sd = weights.synthetic_state_dict(0, head=head)
    vdir = os.path.join(str(tmp_path), "vanilla_model_weights")
    os.makedirs(vdir, exist_ok=True)
    weights.save_vanilla_checkpoint(os.path.join(vdir, "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    training = dict(learn_rate=1e-3, mpnn_learn_rate=1e-4)
    if lr_schedule is not None:
        training["lr_schedule"] = lr_schedule
    cfg = Config.wrap(dict(model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=freeze,
                                      load_pretrained=True, lightattn=lightattn),
                           training=training, platform=dict(thermompnn_dir=str(tmp_path))))
    return _compat_module().TransferModelPL(cfg)


def _ids(params):
    return [id(p) for p in params]


def test_configure_optimizers_builds_the_reference_groups(tmp_path):
    pl = _pl(tmp_path)
    m = pl.model
    assert m.differentiable is True and pl.stage == 1
    assert _ids(pl.parameters()) == _ids(m.parameters())
    opt = pl.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW) and opt.defaults["lr"] == 1e-3
    g = opt.param_groups
    assert len(g) == 4
    assert _ids(g[0]["params"]) == _ids(m.prot_mpnn.parameters()) and g[0]["lr"] == 1e-4
    assert _ids(g[1]["params"]) == _ids(m.light_attention.parameters()) and g[1]["lr"] == 1e-3
    assert _ids(g[2]["params"]) == _ids(m.both_out.parameters()) and g[2]["lr"] == 1e-3
    assert _ids(g[3]["params"]) == _ids(m.ddg_out.parameters()) and g[3]["lr"] == 1e-3
    assert all(x["weight_decay"] == 0.01 and x["betas"] == (0.9, 0.999) and x["eps"] == 1e-8 for x in g)


def test_configure_optimizers_stage_two_frozen_and_no_lightattn(tmp_path):
    pl = _pl(tmp_path, freeze=True)
    pl.stage = 2
    opt = pl.configure_optimizers()
    assert abs(pl.learn_rate - 1e-4) < 1e-18 and opt.defaults["lr"] == pl.learn_rate
    g = opt.param_groups
    assert len(g) == 3                                            # frozen ProteinMPNN: no group
    assert _ids(g[0]["params"]) == _ids(pl.model.light_attention.parameters()) and g[0]["lr"] == 0.0
    assert g[1]["lr"] == g[2]["lr"] == pl.learn_rate
    pl2 = _pl(tmp_path / "nola", lightattn=False)
    g2 = pl2.configure_optimizers().param_groups
    assert len(g2) == 3 and _ids(g2[1]["params"]) == _ids(pl2.model.both_out.parameters())


def test_configure_optimizers_with_a_schedule(tmp_path):
    pl = _pl(tmp_path, lr_schedule=True)
    out = pl.configure_optimizers()
    assert set(out) == {"optimizer", "lr_scheduler", "monitor"} and out["monitor"] == "val_ddG_mse"
    s = out["lr_scheduler"]
    assert isinstance(s, torch.optim.lr_scheduler.ReduceLROnPlateau) and s.optimizer is out["optimizer"]
    assert s.mode == "min" and s.factor == 0.5


def test_the_gradient_path_is_opt_in_and_the_dropout_key_can_be_pinned(tmp_path):
    from thermompnn_amd.transfer_model import TransferModel
    from thermompnn_amd import autograd
    assert TransferModel.differentiable is False
    pl = _pl(tmp_path)
    assert autograd.wants_grad(pl.model)
    with torch.no_grad():
        assert not autograd.wants_grad(pl.model)
    pl.model.differentiable = False
    assert not autograd.wants_grad(pl.model)
    with autograd.dropout_key(5, 9):
        assert autograd._draw_key() == (5, 9)
        with autograd.dropout_key(1, 2):
            assert autograd._draw_key() == (1, 2)
        assert autograd._draw_key() == (5, 9)
    torch.manual_seed(3)
    a = autograd._draw_key()
    torch.manual_seed(3)
    assert autograd._draw_key() == a
