"""TransferModel through torch autograd: the fine-tuning kernels (csrc/tmpnn_finetune.hip) as one ``torch.autograd.Function``.

    model.differentiable = True
    model.train()
    pred, _ = model(pdb, mutations)
    loss = torch.stack([F.mse_loss(p["ddG"], m.ddG) for p, m in zip(pred, mutations) if m.ddG is not None]).mean()
    loss.backward(); opt.step()

The Function's inputs are the module's own parameters in the slab order of ``finetune.slab_shapes`` (ProteinMPNN without W_out, or
only W_s when num_final_layers is 0, then the head); its output is pred [M], one value per live mutant. The forward packs the
parameters into the flat fp32 slab (once per weight version) and runs ``tmpnn_finetune_forward`` into a per-call saved buffer; the
backward runs ``tmpnn_finetune_backward`` from the upstream gradient dL/dpred into a fresh gradient slab and hands torch each
parameter's gradient as a view of it. Torch accumulates into ``.grad`` itself, so hooks, ``torch.autograd.grad``, gradient
accumulation and any optimiser work unchanged. W_out is not an input (it is not in the ddG loss): its ``.grad`` stays None.

``model.sequence_log_probs(pdb, chain_M=None, randn=None)`` is the second differentiable output: ProteinMPNN's own objective,
log_probs [L,21] under a random decoding order (``model_utils.SeqLossFunction`` over ``prot_mpnn``'s parameters, W_out included). A
joint loss is two backward passes, one per Function, into the same ``.grad``s.

Values come from the exact fp32 path, whatever ``model.precision`` says. Dropout follows the submodules' ``training`` flags:
``prot_mpnn.training`` -> p = 0.1 at ProteinMPNN's 15 sites, ``light_attention.training`` -> p = 0.25 on the head's centre tap. The
masks come from the library's counter-based generator keyed on (seed, step): drawn per forward from torch's default CPU generator
(``torch.manual_seed`` makes a run reproducible), or pinned with ``dropout_key(seed, step)``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import TmpnnError, check
from .datasets import ALPHABET
from .finetune import MPNN_DROPOUT, slab_shapes
from .train import CONV_DROPOUT, _ptr, _stream

L_MIN, L_MAX = 2, 8192
_AA = {a: i for i, a in enumerate(ALPHABET)}
_pinned_key: Optional[Tuple[int, int]] = None


@contextlib.contextmanager
def dropout_key(seed: int, step: int):
    """Pin the dropout key of every differentiable forward inside the block to (seed, step) (the generator of
    csrc/tmpnn_finetune.hip: the same key draws the same masks as ``tmpnn_finetune_step`` with that seed and step)."""
    global _pinned_key
    prev = _pinned_key
    _pinned_key = (int(seed), int(step))
    try:
        yield
    finally:
        _pinned_key = prev


def _draw_key() -> Tuple[int, int]:
    if _pinned_key is not None:
        return _pinned_key
    k = torch.randint(0, 2 ** 62, (2,), dtype=torch.int64)      # torch's default CPU generator
    return int(k[0]), int(k[1])


class _Plan:
    """What the device calls need about one TransferModel: the slab layout, the head dims and a scratch buffer shared by the
    backwards (they run in stream order)."""

    def __init__(self, model):
        self.lib = _lib.load()
        self.n_final, self.lightattn = int(model.num_final_layers), bool(model.lightattn)
        self.shapes = slab_shapes(model.hidden_dims, self.n_final, self.lightattn)
        self.names = list(self.shapes)
        self.n_mpnn = sum(1 for k in self.names if k.startswith("prot_mpnn."))
        self.dims = [128 * self.n_final + 128, *[int(d) for d in model.hidden_dims], 21]
        self.n_layers = len(self.dims) - 1
        self.cdims = (C.c_int32 * len(self.dims))(*self.dims)
        self.numel = int(self.lib.tmpnn_finetune_slab_numel(self.n_final, int(self.lightattn), self.n_layers, self.cdims))
        self.sizes = [int(torch.Size(s).numel()) for s in self.shapes.values()]
        if self.numel != sum(self.sizes):
            raise TmpnnError(f"fine-tune slab layout mismatch: library {self.numel}, module {sum(self.sizes)}")
        self._slab: Optional[torch.Tensor] = None
        self._slab_key = None
        self._scratch: Optional[torch.Tensor] = None

    def key(self, model) -> tuple:
        return (tuple(model.hidden_dims), int(model.num_final_layers), bool(model.lightattn))

    def pack(self, params) -> torch.Tensor:
        """The fp32 slab of the parameters' current values; rebuilt when a parameter moves or changes (_version)."""
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._slab is None or key != self._slab_key:
            self._slab = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params])
            self._slab_key = key
        return self._slab

    def saved_bytes(self, L: int, M: int) -> int:
        return int(self.lib.tmpnn_finetune_saved_bytes(L, M, self.n_final, int(self.lightattn), self.n_layers, self.cdims))

    def scratch(self, L: int, M: int, device) -> torch.Tensor:
        need = int(self.lib.tmpnn_finetune_scratch_bytes(L, M, self.n_final, int(self.lightattn), self.n_layers, self.cdims))
        if need == 0:
            raise TmpnnError(f"no fine-tune scratch size for L={L}, M={M}, head dims {self.dims}")
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != device:
            self._scratch = None
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        return self._scratch


def plan_for(model) -> _Plan:
    plan = getattr(model, "_autograd_plan", None)
    if plan is None or plan.key(model) != (tuple(model.hidden_dims), int(model.num_final_layers), bool(model.lightattn)):
        plan = _Plan(model)
        model._autograd_plan = plan
    return plan


class _Inputs:
    """One protein's device inputs and its live mutants (every non-None mutation; ddG labels are not needed)."""

    def __init__(self, X, S, mask, ridx, cenc, pos, mut, wt):
        self.X, self.S, self.mask, self.ridx, self.cenc, self.pos, self.mut, self.wt = X, S, mask, ridx, cenc, pos, mut, wt
        self.L, self.M = int(S.numel()), int(pos.numel())

    def args(self):
        return (_ptr(self.X), _ptr(self.S), _ptr(self.mask), _ptr(self.ridx), _ptr(self.cenc), self.L, _ptr(self.pos), _ptr(self.mut),
                _ptr(self.wt), self.M)


class FinetuneFunction(torch.autograd.Function):
    """pred [M] = TransferModel's ddG of M mutants of one protein, differentiable with respect to the slab parameters."""

    @staticmethod
    def forward(ctx, plan, inp, subtract, p_mpnn, p_head, seed, step, mpnn_grads, *params):
        ctx.x_in = None
        if len(params) == len(plan.sizes) + 1:           # the coordinates follow the parameters (forward_coords): inp.X holds their values
            params, ctx.x_in = params[:-1], (tuple(params[-1].shape), params[-1].dtype)
        slab = plan.pack(params)
        dev = slab.device
        saved = torch.empty(plan.saved_bytes(inp.L, inp.M), dtype=torch.uint8, device=dev)
        pred = torch.empty(inp.M, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(plan.lib.tmpnn_finetune_forward(
                *inp.args(), plan.n_final, int(plan.lightattn), plan.n_layers, plan.cdims, int(subtract), _ptr(slab), plan.numel,
                p_mpnn, p_head, None, None, None, seed, step, _ptr(pred), None, None, _ptr(saved), saved.numel(), _stream()),
                "tmpnn_finetune_forward")
        ctx.plan, ctx.inp, ctx.cfg = plan, inp, (int(subtract), p_mpnn, p_head, seed, step, int(mpnn_grads))
        ctx.save_for_backward(saved, slab)               # freed after a backward without retain_graph
        return pred

    @staticmethod
    @once_differentiable
    def backward(ctx, dpred):
        plan, inp = ctx.plan, ctx.inp
        subtract, p_mpnn, p_head, seed, step, mpnn_grads = ctx.cfg
        saved, slab = ctx.saved_tensors
        dev = slab.device
        dpred = dpred.to(device=dev, dtype=torch.float32).contiguous()
        grads = torch.zeros(plan.numel, dtype=torch.float32, device=dev)
        scratch = plan.scratch(inp.L, inp.M, dev)
        dX = torch.empty_like(inp.X) if ctx.x_in is not None and ctx.needs_input_grad[-1] else None
        with torch.cuda.device(dev):
            if dX is None:
                check(plan.lib.tmpnn_finetune_backward(
                    *inp.args(), plan.n_final, int(plan.lightattn), plan.n_layers, plan.cdims, subtract, _ptr(slab), plan.numel, p_mpnn,
                    p_head, None, None, seed, step, _ptr(dpred), _ptr(grads), mpnn_grads, _ptr(saved), saved.numel(), _ptr(scratch),
                    scratch.numel(), _stream()), "tmpnn_finetune_backward")
            else:
                check(plan.lib.tmpnn_finetune_backward_x(
                    *inp.args(), plan.n_final, int(plan.lightattn), plan.n_layers, plan.cdims, subtract, _ptr(slab), plan.numel, p_mpnn,
                    p_head, None, None, seed, step, _ptr(dpred), _ptr(grads), _ptr(dX), mpnn_grads, _ptr(saved), saved.numel(),
                    _ptr(scratch), scratch.numel(), _stream()), "tmpnn_finetune_backward_x")
        out, off = [], 0
        for i, (shape, n) in enumerate(zip(plan.shapes.values(), plan.sizes)):
            out.append(grads[off:off + n].view(shape) if ctx.needs_input_grad[8 + i] else None)
            off += n
        out = (None,) * 8 + tuple(out)
        return out if ctx.x_in is None else out + (None if dX is None else dX.view(ctx.x_in[0]).to(ctx.x_in[1]),)


def wants_grad(model) -> bool:
    """The gradient path is taken when the model opted in, grad mode is on and some parameter requires grad."""
    return bool(getattr(model, "differentiable", False)) and torch.is_grad_enabled() and \
        any(p.requires_grad for p in model.parameters())


_NOT_DIFFERENTIABLE = "{} is part of the gradient path: set model.differentiable = True"
_FROZEN = "{} needs ProteinMPNN's parameters unfrozen (requires_grad): the coordinates' gradient comes out of the ProteinMPNN backward"


def _given_coords(X, parsed, device, what):
    """The caller's coordinates [L,4,3] in place of the parsed ones -> (their float32 values for the device call, the tensor that
    enters the graph or None when nothing asks for its gradient)."""
    if not torch.is_tensor(X) or not X.is_floating_point() or tuple(X.shape) != tuple(parsed.shape):
        raise ValueError(f"{what}: X must be a float tensor of shape {tuple(parsed.shape)} (the parsed structure's residues x N, CA, C, O)")
    if X.device != device:
        raise ValueError(f"{what}: X is on {X.device}, the model on {device}")
    return X.detach().float().contiguous(), (X if X.requires_grad and torch.is_grad_enabled() else None)


def transfer_forward(model, pdb, mutations, X=None):
    """TransferModel.forward on the gradient path -> (list of {"ddG": Tensor[1]} | None, None); the Tensor[1]s are views of one
    pred tensor that carries the graph. ``X`` (TransferModel.forward_coords) replaces the parsed coordinates and, when it requires
    grad, is one more input of the Function (tmpnn_finetune_backward_x)."""
    from .pdb_io import tied_featurize
    params = dict(model.named_parameters())
    device = next(iter(params.values())).device
    if device.type != "cuda":
        raise RuntimeError("thermompnn_amd runs on MI355X only: move the model to a CUDA (ROCm) device with .cuda(); there is no "
                           "CPU execution path")
    plan = plan_for(model)
    slab_params = [params[k] for k in plan.names]
    mpnn_grads = any(p.requires_grad for p in slab_params[:plan.n_mpnn])
    live = [m for m in mutations if m is not None]
    if X is None and not live:
        return [None for _ in mutations], None
    feats = tied_featurize([pdb[0]], device, None, None, None, None, None, None, ca_only=False)
    x_graph = None
    if X is not None:                                    # checked whatever the mutation list holds
        if not mpnn_grads:
            raise RuntimeError(_FROZEN.format("forward_coords"))
        X_val, x_graph = _given_coords(X, feats[0][0], device, "forward_coords")
        if not live:
            return [None for _ in mutations], None
    else:
        X_val = feats[0][0].float().contiguous()
    S, mask, chain_enc, residue_idx = feats[1][0], feats[2][0], feats[5][0], feats[12][0]
    L = int(S.numel())
    if not L_MIN <= L <= L_MAX:
        raise ValueError(f"protein length {L} outside [{L_MIN}, {L_MAX}]: the differentiable path runs one protein per call")
    for m in live:
        if not 0 <= int(m.position) < L:
            raise ValueError(f"mutation position {m.position} outside [0, {L})")
    code = lambda a: _AA[a] if a in _AA else ALPHABET.index(a)
    sel = torch.tensor([[int(m.position) for m in live], [code(m.mutation) for m in live], [code(m.wildtype) for m in live]],
                       dtype=torch.int32).to(device)
    inp = _Inputs(X_val, S.to(torch.int32).contiguous(), mask.float().contiguous(),
                  residue_idx.to(torch.int32).contiguous(), chain_enc.to(torch.int32).contiguous(), sel[0], sel[1], sel[2])
    p_mpnn = MPNN_DROPOUT if model.prot_mpnn.training and plan.n_final > 0 else 0.0
    p_head = CONV_DROPOUT if plan.lightattn and model.light_attention.training else 0.0
    seed, step = _draw_key()
    extra = () if x_graph is None else (x_graph,)
    pred = FinetuneFunction.apply(plan, inp, bool(model.subtract_mut), p_mpnn, p_head, seed, step, mpnn_grads, *slab_params, *extra)
    pieces = iter(pred.split(1))
    return [None if m is None else {"ddG": next(pieces)} for m in mutations], None


def transfer_sequence_log_probs(model, pdb, chain_M=None, randn=None, X=None):
    """TransferModel.sequence_log_probs: log_probs [L,21] of one parsed structure with a graph over prot_mpnn's parameters, and over
    ``X`` [L,4,3] when it is given in place of the parsed coordinates and requires grad."""
    from . import model_utils as mu
    from .pdb_io import tied_featurize
    from .protein_mpnn_utils import decoding_ranks
    if not getattr(model, "differentiable", False):
        raise RuntimeError(_NOT_DIFFERENTIABLE.format("sequence_log_probs"))
    params = [p for _, p in model.prot_mpnn.named_parameters()]
    device = params[0].device
    if device.type != "cuda":
        raise RuntimeError("thermompnn_amd runs on MI355X only: move the model to a CUDA (ROCm) device with .cuda(); there is no "
                           "CPU execution path")
    feats = tied_featurize([pdb[0] if isinstance(pdb, (list, tuple)) else pdb], device, None, None, None, None, None, None, ca_only=False)
    X_parsed, S, mask, chain_enc, residue_idx = feats[0][0], feats[1][0], feats[2][0], feats[5][0], feats[12][0]
    if X is None:
        X = X_parsed
    else:
        if not any(p.requires_grad for p in params):
            raise RuntimeError(_FROZEN.format("sequence_log_probs(X=)"))
        X_val, x_graph = _given_coords(X, X_parsed, device, "sequence_log_probs")
        X = X_val if x_graph is None else x_graph
    cm = mask if chain_M is None else torch.as_tensor(chain_M, dtype=torch.float32, device=device) * mask
    if randn is None:
        randn = torch.randn(cm.shape, device=device)
    ranks = decoding_ranks(cm, torch.as_tensor(randn, dtype=torch.float32).to(device))
    plan = getattr(model, "_seqloss_plan", None)
    if plan is None:
        plan = model._seqloss_plan = mu.SeqPlan()
    p_mpnn = MPNN_DROPOUT if model.prot_mpnn.training else 0.0
    return mu.sequence_log_probs(plan, params, X, S, mask, residue_idx, chain_enc, ranks, model.prot_mpnn.k_neighbors, p_mpnn)
