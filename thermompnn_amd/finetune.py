"""Fine-tuning of ProteinMPNN together with the ddG head on the GPU: the reference's second recipe (``freeze_weights: false`` with
``mpnn_learn_rate``, transfer_model.py:31-35, train_thermompnn.py:35,88-113).

    python -m thermompnn_amd.finetune config.yaml [local.yaml] model.freeze_weights=false training.mpnn_learn_rate=1e-4 key=value ...

``thermompnn_amd.train`` keeps the released recipe (ProteinMPNN frozen, a feature cache built once). Here the weights change every
step, so there is no cache: every step runs ProteinMPNN's training forward on one protein (dropout active at its 15 sites), the head,
and the backward through both, in HIP (csrc/tmpnn_finetune.hip), then one fused AdamW over a flat slab with the MPNN group at
``mpnn_learn_rate`` and the head groups at ``learn_rate``.

Deviations from the reference ("Fine-tuning ProteinMPNN"): the dropout random stream is this project's counter-based
generator, not torch's; validation runs in eval mode (no dropout) with the current weights; ``W_out`` (log_probs, not in the loss)
is never touched, as torch's AdamW skips a parameter whose ``.grad`` is None; no wandb; ``num_workers`` is ignored.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import TmpnnError, check
from .datasets import ALPHABET
from .metrics import get_metrics
from .train import (BETAS, CONV_DROPOUT, EPS, SEGMENT_CENTRE, SEGMENT_DECAY, SEGMENT_DENSE, WEIGHT_DECAY, _has, _ptr, _stream,
                    checkpoint_name, load_config, make_datasets, make_scheduler, reference_init)

_AA = {a: i for i, a in enumerate(ALPHABET)}
MPNN_DROPOUT = 0.1                        # EncLayer / DecLayer nn.Dropout(dropout=0.1) (protein_mpnn_utils.py:800-856)
N_SITES = 15
MAX_SEGMENTS = 32


def check_finetune_config(cfg) -> float:
    """The unfrozen recipe's rules (before any data is read) -> mpnn_learn_rate."""
    if _has(cfg.model, "freeze_weights") and cfg.model.freeze_weights:
        raise ValueError("freeze_weights: true trains the head only: use thermompnn_amd.train (the released recipe); "
                         "thermompnn_amd.finetune needs model.freeze_weights: false")
    if not _has(cfg.model, "freeze_weights"):
        raise ValueError("thermompnn_amd.finetune needs model.freeze_weights: false")
    lr = cfg.training.mpnn_learn_rate if _has(cfg.training, "mpnn_learn_rate") else None
    # PyYAML (YAML 1.1) reads 1e-4 without a dot as the string '1e-4'; OmegaConf reads it as a float, so such text is accepted
    value = None
    if isinstance(lr, (int, float)) and not isinstance(lr, bool):
        value = float(lr)
    elif isinstance(lr, str):
        try:
            value = float(lr.strip())
        except ValueError:
            value = None
    if value is None or not np.isfinite(value) or value < 0:
        raise ValueError(f"training.mpnn_learn_rate must be a non-negative number (got {lr!r}): the reference builds an AdamW "
                         "group with it")
    if _has(cfg.training, "two_stage") and cfg.training.two_stage:
        raise NotImplementedError("two_stage training (train_thermompnn.py:178-192) is not supported")
    if _has(cfg, "reduce") and cfg.reduce not in (None, ""):
        raise NotImplementedError("reduce (MegaScaleDataset subsampling) is not supported")
    return value


def slab_shapes(hidden_dims, num_final_layers: int, lightattn: bool) -> "Dict[str, tuple]":
    """The slab's tensors in order: ProteinMPNN's (state-dict order, ``prot_mpnn.`` prefix) without W_out.* — only W_s when
    num_final_layers is 0 — then the head's (weights.head_param_shapes)."""
    from collections import OrderedDict
    from .weights import head_param_shapes, mpnn_param_shapes
    s: "OrderedDict[str, tuple]" = OrderedDict()
    for k, v in mpnn_param_shapes().items():
        if k.startswith("W_out."):
            continue
        if int(num_final_layers) == 0 and k != "W_s.weight":
            continue
        s["prot_mpnn." + k] = v
    s.update(head_param_shapes(hidden_dims, int(num_final_layers), bool(lightattn)))
    return s


def segment_table(shapes, subtract_mut: bool):
    """(begins [n + 1], kinds, groups) for tmpnn_adamw_step: ONE segment for the ProteinMPNN block (every element has a gradient),
    then one per head tensor with HeadTrainer's kinds."""
    begins, kinds, groups, off = [], [], [], 0
    mpnn = sum(int(np.prod(v)) for k, v in shapes.items() if k.startswith("prot_mpnn."))
    if mpnn:
        begins.append(0)
        kinds.append(SEGMENT_DENSE)
        groups.append("prot_mpnn")
        off = mpnn
    for k, shape in shapes.items():
        if k.startswith("prot_mpnn."):
            continue
        begins.append(off)
        off += int(np.prod(shape))
        if k.startswith("light_attention.attention_convolution"):
            kinds.append(SEGMENT_DECAY)
        elif k == "light_attention.feature_convolution.weight":
            kinds.append(SEGMENT_CENTRE)
        elif k == "ddg_out.bias" and subtract_mut:
            kinds.append(SEGMENT_DECAY)
        else:
            kinds.append(SEGMENT_DENSE)
        groups.append(k.split(".")[0])
    begins.append(off)
    if len(kinds) > MAX_SEGMENTS:
        raise TmpnnError(f"{len(kinds)} AdamW segments: the fused step takes at most {MAX_SEGMENTS}")
    return begins, kinds, groups


def mask_offsets(L: int) -> List[int]:
    """Start of every dropout site in the flat keep_in / keep_out buffer (site order; [L,128] node sites, [L K,128] edge sites)."""
    K = min(48, L)
    out, o = [], 0
    for s in range(N_SITES):
        out.append(o)
        o += (L * K if s < 9 and s % 3 == 2 else L) * 128
    return out + [o]


class Protein:
    """One protein's device inputs and its labelled mutants (those with a ddG)."""

    def __init__(self, X, S, mask, ridx, cenc, pos, mut, wt, target, name=""):
        self.X, self.S, self.mask, self.ridx, self.cenc = X, S, mask, ridx, cenc
        self.pos, self.mut, self.wt, self.target = pos, mut, wt, target
        self.L, self.M, self.name = int(S.numel()), int(pos.numel()), name
        self.target_host = target.cpu().numpy()


class MPNNTrainer:
    """AdamW training of ``model`` (TransferModel) as a whole, ProteinMPNN included, on the GPU; ``model`` itself only changes in
    ``write_back()``."""

    def __init__(self, model, seed: int = 0, learn_rate: float = 1e-3, mpnn_learn_rate: float = 1e-4, p_mpnn: float = MPNN_DROPOUT,
                 p_head: float = CONV_DROPOUT):
        self.model, self.seed, self.lib = model, int(seed), _lib.load()
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise TmpnnError("MPNNTrainer needs the model on a CUDA (ROCm) device: there is no CPU path")
        self.n_final, self.lightattn = int(model.num_final_layers), bool(model.lightattn)
        self.subtract = bool(model.subtract_mut)
        self.p_mpnn = float(p_mpnn)
        self.p_head = float(p_head) if self.lightattn else 0.0
        self.shapes = slab_shapes(model.hidden_dims, self.n_final, self.lightattn)
        self.dims = [128 * self.n_final + 128, *[int(d) for d in model.hidden_dims], 21]
        self.n_layers = len(self.dims) - 1
        self._cdims = (C.c_int32 * len(self.dims))(*self.dims)
        self.numel = int(self.lib.tmpnn_finetune_slab_numel(self.n_final, int(self.lightattn), self.n_layers, self._cdims))
        if self.numel != sum(int(np.prod(s)) for s in self.shapes.values()):
            raise TmpnnError(f"fine-tune slab layout mismatch: library {self.numel}")
        sd = model.state_dict()
        self.slab = torch.cat([sd[k].detach().reshape(-1).to(self.device, torch.float32) for k in self.shapes]).contiguous()
        self.grad = torch.zeros_like(self.slab)
        self.exp_avg = torch.zeros_like(self.slab)
        self.exp_avg_sq = torch.zeros_like(self.slab)
        begins, kinds, self._seg_group = segment_table(self.shapes, self.subtract)
        # param groups of configure_optimizers (train_thermompnn.py:93-107): prot_mpnn at mpnn_learn_rate, the head at learn_rate
        self.lrs = {g: float(mpnn_learn_rate if g == "prot_mpnn" else learn_rate) for g in dict.fromkeys(self._seg_group)}
        self._seg_begin = (C.c_int64 * len(begins))(*begins)
        self._seg_kind = (C.c_int32 * len(kinds))(*kinds)
        self.offsets, off = {}, 0
        for k, shape in self.shapes.items():
            self.offsets[k] = off
            off += int(np.prod(shape))
        self.step_count = 0
        self._ws: Optional[torch.Tensor] = None
        self.losses = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._n_loss = 0

    # -- data -------------------------------------------------------------------------------------------------------------------
    def prepare(self, items) -> List[Protein]:
        """items: iterable of (pdb, mutations) as the datasets yield them -> one Protein per item (mutants without ddG dropped)."""
        from .pdb_io import tied_featurize
        out = []
        for pdb, mutations in items:
            p = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
            f = tied_featurize([p], self.device, None, None, None, None, None, None, ca_only=False)
            X, S, mask, cenc, ridx = f[0][0], f[1][0], f[2][0], f[5][0], f[12][0]
            L = int(S.numel())
            live = [m for m in mutations if m is not None and m.ddG is not None]
            for m in live:
                if not 0 <= int(m.position) < L:
                    raise ValueError(f"{p.get('name', '')}: mutation position {m.position} outside [0, {L})")
            i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
            out.append(Protein(X.float().contiguous(), S.to(torch.int32).contiguous(), mask.float().contiguous(),
                               ridx.to(torch.int32).contiguous(), cenc.to(torch.int32).contiguous(),
                               i32([int(m.position) for m in live]),
                               i32([_AA[m.mutation] if m.mutation in _AA else ALPHABET.index(m.mutation) for m in live]),
                               i32([_AA[m.wildtype] if m.wildtype in _AA else ALPHABET.index(m.wildtype) for m in live]),
                               torch.tensor([float(m.ddG) for m in live], dtype=torch.float32, device=self.device), p.get("name", "")))
        return out

    # -- device calls ---------------------------------------------------------------------------------------------------------
    def workspace_bytes(self, L: int, M: int) -> int:
        return int(self.lib.tmpnn_finetune_workspace_bytes(L, max(M, 1), self.n_final, int(self.lightattn), self.n_layers, self._cdims))

    def _workspace(self, L: int, M: int) -> torch.Tensor:
        need = self.workspace_bytes(L, M)
        if need == 0:
            raise TmpnnError(f"no fine-tune workspace size for L={L}, M={M}, head dims {self.dims}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def mask_numel(self, L: int) -> int:
        return int(self.lib.tmpnn_finetune_mask_numel(L))

    def forward_backward(self, prot: Protein, keep_in=None, keep_out=None, head_keep_in=None, loss_out=None, pred_out=None, step=None,
                         p_mpnn=None, p_head=None, E_idx_out=None, rows_out=None):
        """Gradients of the protein's loss into ``self.grad`` (training forward, backward). -> loss tensor."""
        if prot.M == 0:
            raise ValueError("a protein without labelled mutants takes no step")
        loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=self.device)
        ws = self._workspace(prot.L, prot.M)
        pm = self.p_mpnn if p_mpnn is None else float(p_mpnn)
        ph = self.p_head if p_head is None else float(p_head)
        with torch.cuda.device(self.device):
            check(self.lib.tmpnn_finetune_step(
                _ptr(prot.X), _ptr(prot.S), _ptr(prot.mask), _ptr(prot.ridx), _ptr(prot.cenc), prot.L, _ptr(prot.pos), _ptr(prot.mut),
                _ptr(prot.wt), _ptr(prot.target), prot.M, self.n_final, int(self.lightattn), self.n_layers, self._cdims,
                int(self.subtract), _ptr(self.slab), _ptr(self.grad), self.numel, pm, ph, _ptr(keep_in), _ptr(keep_out),
                _ptr(head_keep_in), self.seed, self.step_count + 1 if step is None else int(step), _ptr(loss), _ptr(pred_out),
                _ptr(E_idx_out), _ptr(rows_out), _ptr(ws), ws.numel(), _stream()), "tmpnn_finetune_step")
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

    def step(self, prot: Protein) -> bool:
        """One optimiser step on one protein (train_thermompnn.py:64-65): False (no step) when it has no labelled mutant."""
        if prot.M == 0:
            return False
        if self._n_loss >= self.losses.numel():          # grow, keeping the losses already recorded this epoch
            grown = torch.zeros(2 * self.losses.numel(), dtype=torch.float32, device=self.device)
            grown[:self._n_loss].copy_(self.losses[:self._n_loss])
            self.losses = grown
        self.forward_backward(prot, loss_out=self.losses[self._n_loss:self._n_loss + 1])
        self._n_loss += 1
        self.adamw()
        return True

    def epoch_losses(self) -> np.ndarray:
        return self.losses[:self._n_loss].cpu().numpy()

    def predict_one(self, prot: Protein, E_idx_out=None, rows_out=None) -> torch.Tensor:
        pred = torch.empty(prot.M, dtype=torch.float32, device=self.device)
        if prot.M == 0:
            return pred
        ws = self._workspace(prot.L, prot.M)
        with torch.cuda.device(self.device):
            check(self.lib.tmpnn_finetune_eval(
                _ptr(prot.X), _ptr(prot.S), _ptr(prot.mask), _ptr(prot.ridx), _ptr(prot.cenc), prot.L, _ptr(prot.pos), _ptr(prot.mut),
                _ptr(prot.wt), prot.M, self.n_final, int(self.lightattn), self.n_layers, self._cdims, int(self.subtract),
                _ptr(self.slab), self.numel, _ptr(pred), _ptr(E_idx_out), _ptr(rows_out), _ptr(ws), ws.numel(), _stream()),
                "tmpnn_finetune_eval")
        return pred

    def predict(self, prots: List[Protein]) -> torch.Tensor:
        """Eval-mode predictions (no dropout, current weights) for every labelled mutant, in order."""
        parts = [self.predict_one(p) for p in prots if p.M]
        return torch.cat(parts) if parts else torch.zeros(0, device=self.device)

    def evaluate(self, prots: List[Protein]) -> Dict[str, float]:
        tgt = np.concatenate([p.target_host for p in prots if p.M]) if any(p.M for p in prots) else np.zeros(0, np.float32)
        return get_metrics(self.predict(prots).cpu().numpy(), tgt)

    def tensor(self, name: str, which: str = "param") -> torch.Tensor:
        """A slab tensor by its TransferModel state-dict name (``prot_mpnn.`` prefix for ProteinMPNN's)."""
        buf = {"param": self.slab, "grad": self.grad, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}[which]
        o = self.offsets[name]
        return buf[o:o + int(np.prod(self.shapes[name]))].view(self.shapes[name])

    def write_back(self) -> None:
        """Copy the slab into the module's parameters (ProteinMPNN and head) and drop the cached engine, so the inference path
        rebuilds its weight images from the fine-tuned weights."""
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for k in self.shapes:
                params[k].copy_(self.tensor(k).to(params[k].device))
        self.model._engine = None
        self.model._engine_key = None


def finetune(cfg, device="cuda", log=print) -> dict:
    """The reference's train() with ProteinMPNN unfrozen. -> {'best_checkpoint', 'history', 'model', 'trainer'}."""
    from .transfer_model import TransferModel
    from .weights import save_lightning_checkpoint
    mpnn_lr = check_finetune_config(cfg)
    if not _has(cfg, "project"):
        cfg.name = "test"
    seed = int(cfg.training.seed) if _has(cfg.training, "seed") else 0
    train_ds, val_ds = make_datasets(cfg)
    model = TransferModel(cfg).to(device)
    reference_init(model, seed)
    trainer = MPNNTrainer(model, seed=seed, learn_rate=float(cfg.training.learn_rate), mpnn_learn_rate=mpnn_lr)
    train_set = trainer.prepare(train_ds[i] for i in range(len(train_ds)))
    val_set = trainer.prepare(val_ds[i] for i in range(len(val_ds)))
    sched = make_scheduler(trainer.lrs) if _has(cfg.training, "lr_schedule") and cfg.training.lr_schedule else None
    max_ep = int(cfg.training.epochs) if _has(cfg.training, "epochs") else 100
    ckpt_dir = str(cfg.training.checkpoint_dir) if _has(cfg.training, "checkpoint_dir") else "checkpoints"
    os.makedirs(ckpt_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    best, best_path, history = -np.inf, None, []
    for epoch in range(max_ep):
        order = rng.permutation(len(train_set))
        trainer.begin_epoch(int(sum(1 for i in order if train_set[i].M)))
        for i in order:
            trainer.step(train_set[int(i)])
        losses = trainer.epoch_losses()
        val = trainer.evaluate(val_set)
        rec = {"epoch": epoch, "train_loss": float(losses.mean()) if losses.size else float("nan"),
               **{f"val_ddG_{k}": v for k, v in val.items()}, "lr": dict(trainer.lrs)}
        history.append(rec)
        log(json.dumps(rec))
        if sched is not None:                                       # ReduceLROnPlateau halves every group
            sched.step(val["mse"])
            for g, pg in zip(trainer.lrs, sched.optimizer.param_groups):
                trainer.lrs[g] = float(pg["lr"])
        sp = val["spearman"]
        if np.isfinite(sp) and sp > best:
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
    res = finetune(load_config(files, overrides))
    print(json.dumps({"best_checkpoint": res["best_checkpoint"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
