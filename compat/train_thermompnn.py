"""``train_thermompnn.TransferModelPL`` of the reference (/root/reference/train_thermompnn.py:28-121) without Lightning.

The drivers call ``TransferModelPL.load_from_checkpoint(path, cfg=config).model`` (analysis/thermompnn_benchmarking.py:78-84): the
checkpoint's ``state_dict`` is read with the restricted loader and the ``model.`` prefix stripped. The LightningModule body —
``forward``, ``shared_eval``, ``training_step`` / ``validation_step`` / ``test_step`` and ``configure_optimizers`` — runs through torch
autograd on the engine (``model.differentiable = True``, thermompnn_amd/autograd.py), so a hand-written loop or a trainer can drive it.
Metrics are kept with thermompnn_amd.metrics; ``log`` does nothing."""
import _repo  # noqa: F401
import numpy as np
import torch
import torch.nn.functional as F

from thermompnn_amd.metrics import get_metrics
from thermompnn_amd.transfer_model import TransferModel
from thermompnn_amd.weights import load_thermompnn_checkpoint


def train(cfg):
    """The reference's train(cfg) for the frozen-encoder recipe (thermompnn_amd.train.train)."""
    from thermompnn_amd.train import train as _train
    return _train(cfg)


def _has(node, key):
    try:
        return key in node
    except TypeError:
        return hasattr(node, key)


class _Metrics:
    """The (prediction, target) pairs of one split, scored with thermompnn_amd.metrics (r2, mse, rmse, spearman, pearson)."""

    def __init__(self):
        self.pred, self.target = [], []

    def update(self, pred, target):
        self.pred.append(float(pred.detach().reshape(-1)[0]))
        self.target.append(float(torch.as_tensor(target).reshape(-1)[0]))

    def compute(self):
        return get_metrics(np.array(self.pred), np.array(self.target))

    def reset(self):
        self.pred, self.target = [], []


class TransferModelPL:
    def __init__(self, cfg):
        self.cfg = cfg
        self.model = TransferModel(cfg)
        self.model.differentiable = True
        training = cfg.training if _has(cfg, "training") else {}
        self.learn_rate = training.learn_rate if _has(training, "learn_rate") else None
        self.mpnn_learn_rate = training.mpnn_learn_rate if _has(training, "mpnn_learn_rate") else None
        self.lr_schedule = training.lr_schedule if _has(training, "lr_schedule") else False
        self.stage = 1
        self.metrics = {f"{split}_metrics": {"ddG": _Metrics()} for split in ("train", "val", "test")}

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, cfg=None, map_location=None, allow_pickle=None, **_ignored):
        if cfg is None:
            raise TypeError("load_from_checkpoint(path, cfg=config): the reference passes its OmegaConf config here")
        self = cls(cfg)
        self.model.load_state_dict(load_thermompnn_checkpoint(checkpoint_path, allow_pickle=allow_pickle))
        return self

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def eval(self):
        self.model.eval()
        return self

    def cuda(self, device=None):
        self.model.cuda(device)
        return self

    def to(self, *args, **kwargs):
        self.model.to(*args, **kwargs)
        return self

    def parameters(self, recurse=True):
        return self.model.parameters(recurse)

    def named_parameters(self, *args, **kwargs):
        return self.model.named_parameters(*args, **kwargs)

    def forward(self, *args):
        return self.model(*args)

    def __call__(self, *args, **kwargs):
        return self.model(*args, **kwargs)

    def log(self, *args, **kwargs):
        pass

    def shared_eval(self, batch, batch_idx, prefix):
        """train_thermompnn.py:50-77: the mean of the per-mutant F.mse_loss over the labelled mutants (with its graph), or None."""
        assert len(batch) == 1
        mut_pdb, mutations = batch[0]
        pred, _ = self(mut_pdb, mutations)
        ddg_mses = []
        for mut, out in zip(mutations, pred):
            if mut is not None and mut.ddG is not None:
                target = mut.ddG.to(out["ddG"].device)
                ddg_mses.append(F.mse_loss(out["ddG"], target))
                self.metrics[f"{prefix}_metrics"]["ddG"].update(out["ddG"], mut.ddG)
        if not ddg_mses:
            return None
        for name, value in self.metrics[f"{prefix}_metrics"]["ddG"].compute().items():
            self.log(f"{prefix}_ddG_{name}", value, prog_bar=True, on_step=False, on_epoch=True, batch_size=len(batch))
        return torch.stack(ddg_mses).mean()

    def training_step(self, batch, batch_idx):
        return self.shared_eval(batch, batch_idx, "train")

    def validation_step(self, batch, batch_idx):
        return self.shared_eval(batch, batch_idx, "val")

    def test_step(self, batch, batch_idx):
        return self.shared_eval(batch, batch_idx, "test")

    def configure_optimizers(self):
        """train_thermompnn.py:88-121, with self.cfg where the reference reads its global cfg."""
        if self.stage == 2:                        # for the second stage the learning rate drops by a factor of 10
            self.learn_rate /= 10.
            print("New second-stage learning rate: ", self.learn_rate)
        if not self.cfg.model.freeze_weights:      # ProteinMPNN unfrozen
            param_list = [{"params": self.model.prot_mpnn.parameters(), "lr": self.mpnn_learn_rate}]
        else:
            param_list = []
        if self.model.lightattn:
            if self.stage == 2:
                param_list.append({"params": self.model.light_attention.parameters(), "lr": 0.})
            else:
                param_list.append({"params": self.model.light_attention.parameters()})
        mlp_params = [
            {"params": self.model.both_out.parameters()},
            {"params": self.model.ddg_out.parameters()},
        ]
        param_list = param_list + mlp_params
        opt = torch.optim.AdamW(param_list, lr=self.learn_rate)
        if self.lr_schedule:                       # ReduceLROnPlateau on the validation ddG MSE
            lr_sched = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer=opt, mode="min", factor=0.5)
            return {"optimizer": opt, "lr_scheduler": lr_sched, "monitor": "val_ddG_mse"}
        return opt
