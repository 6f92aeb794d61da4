"""Training of the ThermoMPNN ddG head with ProteinMPNN frozen: the counterpart of /root/reference/train_thermompnn.py.

The released recipe (config.yaml: ``freeze_weights: true``) trains only the head — LightAttention, ``both_out`` and ``ddg_out``
(transfer_model.py:31-36, train_thermompnn.py:88-113). So an epoch is one encoder/decoder forward per protein — done ONCE here,
batched, into a device-resident feature cache (``Engine.ssm_forward(want_hidden=True)``) — and, per protein, a forward/backward of
the small head over its labelled mutants plus an AdamW step, both in HIP (csrc/tmpnn_train.hip). The loss stays on the device; the
host reads the epoch's losses once per epoch.

    python -m thermompnn_amd.train config.yaml [local.yaml] key=value ...

Deviations from the reference ("Training"): the encoder runs in eval mode with the embeddings cached once per
protein (under Lightning, ``trainer.fit`` may put the frozen ProteinMPNN back in train mode and so enable its p = 0.1 dropout — not
verified, Lightning is not a dependency); the dropout random stream is this project's counter-based generator, not torch's; no
wandb; ``num_workers`` is ignored.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import TmpnnError, check
from .datasets import ALPHABET
from .metrics import get_metrics

_AA = {a: i for i, a in enumerate(ALPHABET)}
CONV_DROPOUT = 0.25                       # LightAttention(conv_dropout=0.25), transfer_model.py:129
BETAS, EPS, WEIGHT_DECAY = (0.9, 0.999), 1e-8, 0.01   # torch.optim.AdamW defaults (train_thermompnn.py:107)
SEGMENT_DENSE, SEGMENT_CENTRE, SEGMENT_DECAY = 1, 2, 0


class Config(dict):
    """A nested dict with attribute access: the subset of OmegaConf's DictConfig the training driver and TransferModel use."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError as e:
            raise AttributeError(key) from e

    def __setattr__(self, key, value):
        self[key] = value

    @classmethod
    def wrap(cls, obj):
        if isinstance(obj, dict):
            return cls({k: cls.wrap(v) for k, v in obj.items()})
        if isinstance(obj, list):
            return [cls.wrap(v) for v in obj]
        return obj


def _merge(a: dict, b: dict) -> dict:
    out = dict(a)
    for k, v in b.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def load_config(paths: Sequence[str], overrides: Sequence[str] = ()) -> Config:
    """YAML files merged left to right, then ``a.b.c=value`` overrides (values parsed as YAML) — OmegaConf.merge's behaviour
    for the reference's config.yaml + local.yaml + CLI (train_thermompnn.py:205-209)."""
    import yaml
    cfg: dict = {}
    for p in paths:
        with open(p) as fh:
            cfg = _merge(cfg, yaml.safe_load(fh) or {})
    for item in overrides:
        key, sep, val = item.partition("=")
        if not sep:
            raise ValueError(f"override {item!r}: expected key=value")
        node = cfg
        *path, leaf = key.split(".")
        for part in path:
            node = node.setdefault(part, {})
        node[leaf] = yaml.safe_load(val)
    return Config.wrap(cfg)


def _has(node, key) -> bool:
    try:
        return key in node
    except TypeError:
        return hasattr(node, key)


def check_supported(cfg) -> None:
    """Refuse what needs more than the frozen-encoder head training (NotImplementedError, before any data is read)."""
    if not cfg.model.freeze_weights or (_has(cfg.training, "mpnn_learn_rate") and cfg.training.mpnn_learn_rate is not None):
        raise NotImplementedError("freeze_weights: false / mpnn_learn_rate trains ProteinMPNN itself, which needs the encoder "
                                  "backward; only the head is trained here (the released recipe)")
    if _has(cfg.training, "two_stage") and cfg.training.two_stage:
        raise NotImplementedError("two_stage training (train_thermompnn.py:178-192) is not supported")
    if _has(cfg, "reduce") and cfg.reduce not in (None, ""):
        raise NotImplementedError("reduce (MegaScaleDataset subsampling) is not supported")


def checkpoint_name(name: str, epoch: int, spearman: float) -> str:
    """ModelCheckpoint(filename=cfg.name + '_{epoch:02d}_{val_ddG_spearman:.02}') (train_thermompnn.py:164-167) with Lightning's
    default auto_insert_metric_name=True, which writes each '{metric...}' group as 'metric=value'."""
    return f"{name}_epoch={epoch:02d}_val_ddG_spearman={spearman:.02}.ckpt"


def _ptr(t: Optional[torch.Tensor], offset_elems: int = 0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Split:
    """Device feature cache of one split: feat [T, D0], and the labelled mutants of every protein as slices of flat arrays."""

    def __init__(self, feat, rows, mut, wt, target, starts, counts, names):
        self.feat, self.rows, self.mut, self.wt, self.target = feat, rows, mut, wt, target
        self.starts, self.counts, self.names = starts, counts, names
        self.target_host = target.cpu().numpy()

    def __len__(self):
        return len(self.starts)


class HeadTrainer:
    """AdamW training of ``model``'s head (TransferModel with any head configuration) on the GPU; ``model`` itself only
    changes in ``write_back()``."""

    def __init__(self, model, seed: int = 0, learn_rate: float = 1e-3, p_drop: float = CONV_DROPOUT):
        self.model, self.seed, self.lib = model, int(seed), _lib.load()
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise TmpnnError("HeadTrainer needs the model on a CUDA (ROCm) device: there is no CPU path")
        self.n_final, self.lightattn = int(model.num_final_layers), bool(model.lightattn)
        self.subtract = bool(model.subtract_mut)
        self.p_drop = float(p_drop) if self.lightattn else 0.0
        from .weights import head_param_shapes
        self.shapes = head_param_shapes(model.hidden_dims, self.n_final, self.lightattn)
        self.dims = [128 * self.n_final + 128, *[int(d) for d in model.hidden_dims], 21]
        self.n_layers = len(self.dims) - 1
        self._cdims = (C.c_int32 * len(self.dims))(*self.dims)
        self.numel = int(self.lib.tmpnn_head_slab_numel(self.n_final, int(self.lightattn), self.n_layers, self._cdims))
        if self.numel != sum(int(np.prod(s)) for s in self.shapes.values()):
            raise TmpnnError(f"head slab layout mismatch: library {self.numel}")
        sd = model.state_dict()
        self.slab = torch.cat([sd[k].detach().reshape(-1).to(self.device, torch.float32) for k in self.shapes]).contiguous()
        self.grad = torch.zeros_like(self.slab)
        self.exp_avg = torch.zeros_like(self.slab)
        self.exp_avg_sq = torch.zeros_like(self.slab)
        # param groups of configure_optimizers (train_thermompnn.py:94-107): light_attention, both_out, ddg_out
        self.groups = (["light_attention"] if self.lightattn else []) + ["both_out", "ddg_out"]
        self.lrs = {g: float(learn_rate) for g in self.groups}
        begins, kinds, seg_group, off = [], [], [], 0
        for k, shape in self.shapes.items():
            begins.append(off)
            off += int(np.prod(shape))
            if k.startswith("light_attention.attention_convolution"):
                kinds.append(SEGMENT_DECAY)              # softmax over a size-1 axis: exactly zero gradient
            elif k == "light_attention.feature_convolution.weight":
                kinds.append(SEGMENT_CENTRE)             # only the centre tap meets data
            elif k == "ddg_out.bias" and self.subtract:
                kinds.append(SEGMENT_DECAY)              # cancels in out[mut] - out[wt]
            else:
                kinds.append(SEGMENT_DENSE)
            seg_group.append(k.split(".")[0])
        self._seg_begin = (C.c_int64 * (len(begins) + 1))(*begins, off)
        self._seg_kind = (C.c_int32 * len(kinds))(*kinds)
        self._seg_group = seg_group
        self.offsets = dict(zip(self.shapes, begins))
        self.step_count = 0
        self._ws: Optional[torch.Tensor] = None
        self.losses = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._n_loss = 0

    # -- feature cache -------------------------------------------------------------------------------------------------
    def build_cache(self, items, chunk_residues: int = 1 << 16) -> _Split:
        """items: iterable of (pdb, mutations) as the datasets yield them. One batched encoder/decoder forward per chunk of
        proteins, then feat = [h_dec(last) | ... | W_s[S]] per residue. Mutants without ddG are not training rows."""
        from .pdb_io import tied_featurize
        eng = self.model.engine()
        feats, rows, mut, wt, tgt, starts, counts, names = [], [], [], [], [], [], [], []
        batch, t0 = [], 0

        def flush():
            nonlocal batch
            if not batch:
                return
            X = torch.cat([b[0] for b in batch])
            S = torch.cat([b[1] for b in batch])
            mask = torch.cat([b[2] for b in batch])
            ridx = torch.cat([b[3] for b in batch])
            cenc = torch.cat([b[4] for b in batch])
            lens = [b[1].numel() for b in batch]
            offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
            with torch.cuda.device(eng.device):
                res = eng.ssm_forward(X, S, mask, ridx, cenc, offs, max_len=max(lens), want_ddg=False, want_hidden=True)
                hid = res["hidden"]
                parts = [hid[2 - k] for k in range(self.n_final)] + [eng.seq_embed(S)]
                feats.append(torch.cat(parts, dim=1))
            batch = []

        n_res = 0
        for pdb, mutations in items:
            p = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
            f = tied_featurize([p], self.device, None, None, None, None, None, None, ca_only=False)
            X, S, mask, cenc, ridx = f[0][0], f[1][0], f[2][0], f[5][0], f[12][0]
            L = int(S.numel())
            live = [m for m in mutations if m is not None and m.ddG is not None]
            starts.append(len(rows))
            counts.append(len(live))
            names.append(p.get("name", ""))
            for m in live:
                if not 0 <= int(m.position) < L:
                    raise ValueError(f"{p.get('name', '')}: mutation position {m.position} outside [0, {L})")
                rows.append(t0 + int(m.position))
                mut.append(_AA[m.mutation] if m.mutation in _AA else ALPHABET.index(m.mutation))
                wt.append(_AA[m.wildtype] if m.wildtype in _AA else ALPHABET.index(m.wildtype))
                tgt.append(float(m.ddG))
            batch.append((X, S, mask, ridx, cenc))
            t0 += L
            n_res += L
            if n_res >= chunk_residues:
                flush()
                n_res = 0
        flush()
        dev = self.device
        feat = torch.cat(feats).contiguous() if feats else torch.zeros((1, self.dims[0]), device=dev)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        return _Split(feat, i32(rows), i32(mut), i32(wt), torch.tensor(tgt, dtype=torch.float32, device=dev), starts, counts, names)

    # -- device calls ------------------------------------------------------------------------------------------------
    def _workspace(self, M: int) -> torch.Tensor:
        need = int(self.lib.tmpnn_head_train_workspace_bytes(M, self.n_final, int(self.lightattn), self.n_layers, self._cdims))
        if need == 0:
            raise TmpnnError(f"head dims {self.dims}: no workspace size for M={M}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def forward_backward(self, split: _Split, i: int, keep_in=None, keep_out=None, loss_out=None, pred_out=None, step=None):
        """Gradients of protein ``i``'s loss into ``self.grad`` (the head's forward in train mode, backward). -> loss tensor."""
        start, M = split.starts[i], split.counts[i]
        if M == 0:
            raise ValueError("a protein without labelled mutants takes no step")
        loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=self.device)
        ws = self._workspace(M)
        with torch.cuda.device(self.device):
            check(self.lib.tmpnn_head_train_step(
                _ptr(split.feat), split.feat.shape[0], _ptr(split.rows, start), _ptr(split.mut, start), _ptr(split.wt, start),
                _ptr(split.target, start), M, self.n_final, int(self.lightattn), self.n_layers, self._cdims, int(self.subtract),
                _ptr(self.slab), _ptr(self.grad), self.numel, self.p_drop, _ptr(keep_in), _ptr(keep_out),
                self.seed, self.step_count + 1 if step is None else int(step), _ptr(loss), _ptr(pred_out), _ptr(ws), ws.numel(),
                _stream()), "tmpnn_head_train_step")
        return loss

    def adamw(self) -> None:
        self.step_count += 1
        lrs = (C.c_double * len(self._seg_group))(*[self.lrs[g] for g in self._seg_group])
        with torch.cuda.device(self.device):
            check(self.lib.tmpnn_adamw_step(_ptr(self.slab), _ptr(self.grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), self.numel,
                                            len(self._seg_group), self._seg_begin, self._seg_kind, lrs, BETAS[0], BETAS[1], EPS,
                                            WEIGHT_DECAY, self.step_count, _stream()), "tmpnn_adamw_step")

    def begin_epoch(self, n_steps: int) -> None:
        if self.losses.numel() < max(n_steps, 1):
            self.losses = torch.zeros(max(n_steps, 1), dtype=torch.float32, device=self.device)
        self._n_loss = 0

    def step(self, split: _Split, i: int) -> bool:
        """One optimiser step on protein ``i`` (train_thermompnn.py:64-65): False (no step) when it has no labelled mutant."""
        if split.counts[i] == 0:
            return False
        if self._n_loss >= self.losses.numel():
            self.begin_epoch(2 * self.losses.numel())
        self.forward_backward(split, i, loss_out=self.losses[self._n_loss:self._n_loss + 1])
        self._n_loss += 1
        self.adamw()
        return True

    def epoch_losses(self) -> np.ndarray:
        """The per-step losses of the current epoch: ONE device-to-host copy."""
        return self.losses[:self._n_loss].cpu().numpy()

    def predict(self, split: _Split) -> torch.Tensor:
        """Eval-mode predictions (no dropout) for every labelled mutant of the split, in split order."""
        M = int(split.rows.numel())
        pred = torch.empty(M, dtype=torch.float32, device=self.device)
        if M == 0:
            return pred
        ws = self._workspace(M)
        with torch.cuda.device(self.device):
            check(self.lib.tmpnn_head_eval(_ptr(split.feat), split.feat.shape[0], _ptr(split.rows), _ptr(split.mut), _ptr(split.wt), M,
                                           self.n_final, int(self.lightattn), self.n_layers, self._cdims, int(self.subtract),
                                           _ptr(self.slab), self.numel, _ptr(pred), _ptr(ws), ws.numel(), _stream()), "tmpnn_head_eval")
        return pred

    def evaluate(self, split: _Split) -> Dict[str, float]:
        """r2 / mse / rmse / spearman (+ pearson, n) over the whole split (metrics.get_metrics)."""
        return get_metrics(self.predict(split).cpu().numpy(), split.target_host)

    def tensor(self, name: str, which: str = "param") -> torch.Tensor:
        buf = {"param": self.slab, "grad": self.grad, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}[which]
        o = self.offsets[name]
        return buf[o:o + int(np.prod(self.shapes[name]))].view(self.shapes[name])

    def write_back(self) -> None:
        """Copy the slab into the module's parameters and drop the cached engine (the engine keys on data_ptr / _version)."""
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for k in self.shapes:
                params[k].copy_(self.tensor(k).to(params[k].device))
        self.model._engine = None
        self.model._engine_key = None


def reference_init(model, seed: int) -> None:
    """The head's initial values as the reference constructs them: torch's default nn.Conv1d / nn.Linear initialisation
    (transfer_model.py:57-73, 131-134) in construction order, from ``torch.manual_seed(seed)``."""
    import torch.nn as nn
    torch.manual_seed(int(seed))
    D0 = 128 * int(model.num_final_layers) + 128
    fresh: Dict[str, torch.Tensor] = {}
    if model.lightattn:
        for conv in ("feature_convolution", "attention_convolution"):
            c = nn.Conv1d(D0, D0, 9, stride=1, padding=4)
            fresh[f"light_attention.{conv}.weight"], fresh[f"light_attention.{conv}.bias"] = c.weight, c.bias
    sizes = [D0, *model.hidden_dims, 21]
    for i, (a, b) in enumerate(zip(sizes, sizes[1:])):
        lin = nn.Linear(a, b)
        fresh[f"both_out.{2 * i + 1}.weight"], fresh[f"both_out.{2 * i + 1}.bias"] = lin.weight, lin.bias
    lin = nn.Linear(1, 1)
    fresh["ddg_out.weight"], fresh["ddg_out.bias"] = lin.weight, lin.bias
    params = dict(model.named_parameters())
    with torch.no_grad():
        for k, v in fresh.items():
            params[k].copy_(v.detach().to(params[k].device))


def make_datasets(cfg):
    """train / val datasets for cfg.datasets (train_thermompnn.py:123-143)."""
    from .datasets import ComboDataset, FireProtDataset, MegaScaleDataset
    names = list(cfg.datasets)
    if len(names) == 1:
        d = names[0]
        if d == "fireprot":
            return FireProtDataset(cfg, "train"), FireProtDataset(cfg, "val")
        if d == "megascale_s669":
            return MegaScaleDataset(cfg, "train_s669"), MegaScaleDataset(cfg, "val")
        if d.startswith("megascale_cv"):
            cv = d[-1]
            return MegaScaleDataset(cfg, f"cv_train_{cv}"), MegaScaleDataset(cfg, f"cv_val_{cv}")
        if d == "megascale":
            return MegaScaleDataset(cfg, "train"), MegaScaleDataset(cfg, "val")
        raise ValueError("Invalid dataset specified!")
    return ComboDataset(cfg, "train"), ComboDataset(cfg, "val")


def make_scheduler(lrs: Dict[str, float]):
    """ReduceLROnPlateau(mode='min', factor=0.5), torch's other defaults (train_thermompnn.py:109-111), driving the learning
    rates of the param groups (a parameter-less carrier optimiser holds them)."""
    carrier = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": lr} for lr in lrs.values()], lr=1.0)
    return torch.optim.lr_scheduler.ReduceLROnPlateau(carrier, mode="min", factor=0.5)


def train(cfg, device="cuda", log=print) -> dict:
    """Mirror of the reference's train() for the frozen-encoder recipe. -> {'best_checkpoint', 'history'}."""
    from .transfer_model import TransferModel
    from .weights import save_lightning_checkpoint
    check_supported(cfg)
    if not _has(cfg, "project"):
        cfg.name = "test"                                           # the reference names runs without a project 'test' (:118-121)
    seed = int(cfg.training.seed) if _has(cfg.training, "seed") else 0
    train_ds, val_ds = make_datasets(cfg)
    model = TransferModel(cfg).to(device)
    reference_init(model, seed)
    trainer = HeadTrainer(model, seed=seed, learn_rate=float(cfg.training.learn_rate))
    train_split = trainer.build_cache(iter(train_ds[i] for i in range(len(train_ds))))
    val_split = trainer.build_cache(iter(val_ds[i] for i in range(len(val_ds))))
    sched = make_scheduler(trainer.lrs) if _has(cfg.training, "lr_schedule") and cfg.training.lr_schedule else None
    max_ep = int(cfg.training.epochs) if _has(cfg.training, "epochs") else 100
    ckpt_dir = str(cfg.training.checkpoint_dir) if _has(cfg.training, "checkpoint_dir") else "checkpoints"
    os.makedirs(ckpt_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    best, best_path, history = -np.inf, None, []
    for epoch in range(max_ep):
        order = rng.permutation(len(train_split))                   # DataLoader(shuffle=True), seeded here (:157)
        trainer.begin_epoch(int(sum(1 for i in order if train_split.counts[i])))
        for i in order:
            trainer.step(train_split, int(i))
        losses = trainer.epoch_losses()
        val = trainer.evaluate(val_split)
        rec = {"epoch": epoch, "train_loss": float(losses.mean()) if losses.size else float("nan"),
               **{f"val_ddG_{k}": v for k, v in val.items()}, "lr": dict(trainer.lrs)}
        history.append(rec)
        log(json.dumps(rec))
        if sched is not None:
            sched.step(val["mse"])
            for g, pg in zip(trainer.lrs, sched.optimizer.param_groups):
                trainer.lrs[g] = float(pg["lr"])
        sp = val["spearman"]
        if np.isfinite(sp) and sp > best:                           # ModelCheckpoint(monitor='val_ddG_spearman', mode='max'), top 1
            best = sp
            trainer.write_back()
            path = os.path.join(ckpt_dir, checkpoint_name(cfg.name, epoch, sp))
            save_lightning_checkpoint(path, model.state_dict())
            if best_path and best_path != path and os.path.exists(best_path):
                os.remove(best_path)
            best_path = path
    trainer.write_back()
    return {"best_checkpoint": best_path, "history": history, "model": model, "trainer": trainer}


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    files = [a for a in argv if "=" not in a]
    overrides = [a for a in argv if "=" in a]
    if not files:
        files = ["config.yaml"] + (["local.yaml"] if os.path.exists("local.yaml") else [])
    res = train(load_config(files, overrides))
    print(json.dumps({"best_checkpoint": res["best_checkpoint"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
