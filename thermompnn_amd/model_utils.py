"""Counterpart of the training flavour of the reference (/root/reference/model_utils.py): ``ProteinMPNN.forward`` returns
log p(sequence | structure) under a random decoding order with a graph over the parameters, ``loss_nll`` / ``loss_smoothed`` score it,
``NoamOpt`` / ``get_std_opt`` schedule the optimiser, ``featurize`` packs a batch.

    model = ProteinMPNN(k_neighbors=48, augment_eps=0.0).cuda()
    X, S, mask, lengths, chain_M, residue_idx, mask_self, chain_encoding_all = featurize(batch, "cuda")
    log_probs = model(X, S, mask, chain_M, residue_idx, chain_encoding_all)
    _, loss = loss_smoothed(S, log_probs, mask * chain_M)
    loss.backward(); optimizer.step()

The arithmetic runs in csrc/tmpnn_finetune.hip (tmpnn_seqloss_forward / _backward): the exact-fp32 training forward and the
deterministic backward of the ddG fine-tuning path with the order-masked decoder and the output layer. One
``torch.autograd.Function`` call per batch member, or with ``model.packed = True`` one for the whole batch
(csrc/tmpnn_seqbatch.hip, tmpnn_seqloss_batch_*: the same kernels over the packed rows); the Function's inputs are the module's parameters in state-dict order (W_out
included), packed once per weight version into one flat slab. When ``X`` requires grad it is one more input of the Function and the
backward is the ``_x`` entry (tmpnn_seqloss_backward_x / tmpnn_seqloss_batch_backward_x): ``X.grad`` is dL / dX with the neighbour graph
and D_max of ``_dist`` held constant (include/tmpnn.h); the ``augment_eps`` noise is added on the host, so torch carries the gradient
through it to the caller's ``X``. The dropout masks come from the library's counter-based generator, keyed per forward from
torch's default CPU generator or pinned with ``thermompnn_amd.autograd.dropout_key``; the decoding order is drawn with
``torch.randn`` as the reference draws it, or replayed through ``randn=``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import weights as _weights
from ._lib import TmpnnError, check
from .pdb_io import featurize  # noqa: F401  (API surface)
from .protein_mpnn_utils import _register_tree, decoding_ranks
from .train import _ptr, _stream

L_MIN, L_MAX = 2, 8192
MPNN_DROPOUT = 0.1
_CPU_ERROR = ("thermompnn_amd runs on MI355X only: move the model to a CUDA (ROCm) device with .cuda(); there is no "
              "CPU execution path")


class SeqPlan:
    """What the device calls need: the slab layout (weights.mpnn_param_shapes, W_out included), the packed slab of the current
    weight version and a scratch buffer shared by the backwards (they run in stream order)."""

    def __init__(self):
        self.lib = _lib.load()
        self.shapes = _weights.mpnn_param_shapes()
        self.names = list(self.shapes)
        self.sizes = [int(torch.Size(s).numel()) for s in self.shapes.values()]
        self.numel = int(self.lib.tmpnn_seqloss_slab_numel())
        if self.numel != sum(self.sizes):
            raise TmpnnError(f"sequence-loss slab layout mismatch: library {self.numel}, module {sum(self.sizes)}")
        self._slab: Optional[torch.Tensor] = None
        self._slab_key = None
        self._scratch: Optional[torch.Tensor] = None

    def pack(self, params) -> torch.Tensor:
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._slab is None or key != self._slab_key:
            self._slab = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params])
            self._slab_key = key
        return self._slab

    def saved_bytes(self, L: int) -> int:
        n = int(self.lib.tmpnn_seqloss_saved_bytes(L))
        if n == 0:
            raise ValueError(f"protein length {L} outside [{L_MIN}, {L_MAX}]")
        return n

    def scratch(self, L: int, device) -> torch.Tensor:
        need = int(self.lib.tmpnn_seqloss_scratch_bytes(L))
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != device:
            self._scratch = None
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        return self._scratch

    def batch_scratch(self, inp, device) -> torch.Tensor:
        """The same shared buffer, grown to what a packed batch's backward needs."""
        need = int(self.lib.tmpnn_seqloss_batch_scratch_bytes(inp.T, inp.n, inp.K))
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != device:
            self._scratch = None
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        return self._scratch


class SeqInputs:
    """One protein's device inputs: X [L,4,3] fp32, S / residue_idx / chain_enc / ranks [L] int32, mask [L] fp32."""

    def __init__(self, X, S, mask, ridx, cenc, ranks, k_neighbors):
        f = lambda t: t.detach().to(torch.float32).contiguous()
        i = lambda t: t.detach().to(torch.int32).contiguous()
        self.X, self.S, self.mask, self.ridx, self.cenc, self.ranks = f(X), i(S), f(mask), i(ridx), i(cenc), i(ranks)
        self.L, self.K = int(self.S.numel()), int(k_neighbors)
        if not L_MIN <= self.L <= L_MAX:
            raise ValueError(f"protein length {self.L} outside [{L_MIN}, {L_MAX}]")

    def args(self):
        return (_ptr(self.X), _ptr(self.S), _ptr(self.mask), _ptr(self.ridx), _ptr(self.cenc), self.L, self.K, _ptr(self.ranks))


def _split_x(plan, params):
    """The Functions' trailing inputs: ProteinMPNN's parameters, then (optionally) the coordinates as they came from the caller ->
    (params, (shape, dtype) of the coordinates or None)."""
    if len(params) == len(plan.sizes) + 1:
        return params[:-1], (tuple(params[-1].shape), params[-1].dtype)
    return params, None


def _x_grad(x_in, dX):
    """The coordinates' slot of a backward's result: () without that input, else dX in the caller's shape and dtype (or None)."""
    if x_in is None:
        return ()
    return (None if dX is None else dX.view(x_in[0]).to(x_in[1]),)


def _wants_dx(X) -> bool:
    return torch.is_tensor(X) and X.requires_grad and torch.is_grad_enabled()


class SeqLossFunction(torch.autograd.Function):
    """log_probs [L,21] of one protein under ``inp.ranks``, differentiable with respect to ProteinMPNN's parameters, and with respect
    to the coordinates when they follow the parameters as one more input (``inp.X`` holds their values)."""

    @staticmethod
    def forward(ctx, plan, inp, p_mpnn, seed, step, *params):
        params, ctx.x_in = _split_x(plan, params)
        slab = plan.pack(params)
        dev = slab.device
        saved = torch.empty(plan.saved_bytes(inp.L), dtype=torch.uint8, device=dev)
        log_probs = torch.empty((inp.L, 21), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(plan.lib.tmpnn_seqloss_forward(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, None, seed, step, _ptr(log_probs), None,
                                                 _ptr(saved), saved.numel(), _stream()), "tmpnn_seqloss_forward")
        ctx.plan, ctx.inp, ctx.cfg = plan, inp, (p_mpnn, seed, step)
        ctx.save_for_backward(saved, slab)               # dropped at once when nothing requires grad (no_grad, frozen parameters)
        return log_probs

    @staticmethod
    @once_differentiable
    def backward(ctx, dlp):
        plan, inp = ctx.plan, ctx.inp
        p_mpnn, seed, step = ctx.cfg
        saved, slab = ctx.saved_tensors
        dev = slab.device
        dlp = dlp.to(device=dev, dtype=torch.float32).contiguous()
        grads = torch.zeros(plan.numel, dtype=torch.float32, device=dev)
        scratch = plan.scratch(inp.L, dev)
        dX = torch.empty_like(inp.X) if ctx.x_in is not None and ctx.needs_input_grad[-1] else None
        with torch.cuda.device(dev):
            if dX is None:
                check(plan.lib.tmpnn_seqloss_backward(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, seed, step, _ptr(dlp), _ptr(grads),
                                                      _ptr(saved), saved.numel(), _ptr(scratch), scratch.numel(), _stream()),
                      "tmpnn_seqloss_backward")
            else:
                check(plan.lib.tmpnn_seqloss_backward_x(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, seed, step, _ptr(dlp), _ptr(grads),
                                                        _ptr(dX), _ptr(saved), saved.numel(), _ptr(scratch), scratch.numel(), _stream()),
                      "tmpnn_seqloss_backward_x")
        out, off = [], 0
        for i, (shape, n) in enumerate(zip(plan.shapes.values(), plan.sizes)):
            out.append(grads[off:off + n].view(shape) if ctx.needs_input_grad[5 + i] else None)
            off += n
        return (None,) * 5 + tuple(out) + _x_grad(ctx.x_in, dX)


def sequence_log_probs(plan: SeqPlan, params, X, S, mask, residue_idx, chain_enc, ranks, k_neighbors: int, p_mpnn: float):
    """log_probs [L,21] of one protein with a graph over ``params`` (ProteinMPNN's parameters in state-dict order), and over ``X``
    when it requires grad (dL / dX with the graph and D_max of _dist constant: tmpnn_seqloss_backward_x)."""
    from .autograd import _draw_key
    if params[0].device.type != "cuda":
        raise RuntimeError(_CPU_ERROR)
    dev = params[0].device
    inp = SeqInputs(*(t.to(dev) for t in (X, S, mask, residue_idx, chain_enc, ranks)), k_neighbors)
    seed, step = _draw_key() if p_mpnn > 0 else (0, 0)
    extra = (X.to(dev),) if _wants_dx(X) else ()          # the coordinates with their graph: one more input of the node
    return SeqLossFunction.apply(plan, inp, float(p_mpnn), seed, step, *params, *extra)


class SeqBatchInputs:
    """A packed batch's device inputs: X [T,4,3] fp32, S / residue_idx / chain_enc / ranks [T] int32, mask [T] fp32, offsets
    [n + 1] int32 (protein b in the rows offsets[b]:offsets[b+1]), and the bounds the lengths are promised to keep."""

    def __init__(self, X, S, mask, ridx, cenc, ranks, offsets, k_neighbors, min_len=None, max_len=None):
        f = lambda t: t.detach().to(torch.float32).contiguous()
        i = lambda t: t.detach().to(torch.int32).contiguous()
        self.X, self.S, self.mask, self.ridx, self.cenc, self.ranks = f(X), i(S), f(mask), i(ridx), i(cenc), i(ranks)
        host = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
        self.n, self.T, self.k_neighbors = len(host) - 1, int(self.S.numel()), int(k_neighbors)
        if self.n < 1:
            raise ValueError("offsets must hold n_proteins + 1 entries, n_proteins >= 1")
        lens = [b - a for a, b in zip(host, host[1:])]
        self.min_len = int(min(lens) if min_len is None else min_len)
        self.max_len = int(max(lens) if max_len is None else max_len)
        if not L_MIN <= self.min_len <= self.max_len <= L_MAX:
            raise ValueError(f"protein lengths {self.min_len}..{self.max_len} outside [{L_MIN}, {L_MAX}]")
        self.K = min(self.k_neighbors, self.min_len)
        self.offsets = torch.tensor(host, dtype=torch.int32, device=self.S.device)

    def args(self):
        return (_ptr(self.X), _ptr(self.S), _ptr(self.mask), _ptr(self.ridx), _ptr(self.cenc), _ptr(self.offsets), self.n, self.T,
                self.min_len, self.max_len, self.k_neighbors, _ptr(self.ranks))


class SeqBatchFunction(torch.autograd.Function):
    """log_probs [T,21] of a packed batch under ``inp.ranks``: ONE autograd node, one saved buffer, one gradient slab and one backward
    for all its proteins (tmpnn_seqloss_batch_forward / _backward). ``status`` [1] int32 receives the device status word."""

    @staticmethod
    def forward(ctx, plan, inp, status, p_mpnn, seed, step, *params):
        params, ctx.x_in = _split_x(plan, params)
        slab = plan.pack(params)
        dev = slab.device
        need = int(plan.lib.tmpnn_seqloss_batch_saved_bytes(inp.T, inp.n, inp.K))
        if need == 0:
            raise ValueError(f"packed batch of {inp.T} rows, {inp.n} proteins, K = {inp.K}: outside what tmpnn_seqloss_batch_* takes")
        saved = torch.empty(need, dtype=torch.uint8, device=dev)
        log_probs = torch.empty((inp.T, 21), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(plan.lib.tmpnn_seqloss_batch_forward(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, None, seed, step, _ptr(log_probs),
                                                       None, _ptr(status), _ptr(saved), saved.numel(), _stream()),
                  "tmpnn_seqloss_batch_forward")
        ctx.plan, ctx.inp, ctx.cfg = plan, inp, (p_mpnn, seed, step)
        ctx.save_for_backward(saved, slab)
        return log_probs

    @staticmethod
    @once_differentiable
    def backward(ctx, dlp):
        plan, inp = ctx.plan, ctx.inp
        p_mpnn, seed, step = ctx.cfg
        saved, slab = ctx.saved_tensors
        dev = slab.device
        dlp = dlp.to(device=dev, dtype=torch.float32).contiguous()
        grads = torch.zeros(plan.numel, dtype=torch.float32, device=dev)
        scratch = plan.batch_scratch(inp, dev)
        dX = torch.empty_like(inp.X) if ctx.x_in is not None and ctx.needs_input_grad[-1] else None
        with torch.cuda.device(dev):
            if dX is None:
                check(plan.lib.tmpnn_seqloss_batch_backward(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, seed, step, _ptr(dlp),
                                                            _ptr(grads), _ptr(saved), saved.numel(), _ptr(scratch), scratch.numel(), _stream()),
                      "tmpnn_seqloss_batch_backward")
            else:
                check(plan.lib.tmpnn_seqloss_batch_backward_x(*inp.args(), _ptr(slab), plan.numel, p_mpnn, None, seed, step, _ptr(dlp),
                                                              _ptr(grads), _ptr(dX), _ptr(saved), saved.numel(), _ptr(scratch),
                                                              scratch.numel(), _stream()), "tmpnn_seqloss_batch_backward_x")
        out, off = [], 0
        for i, (shape, n) in enumerate(zip(plan.shapes.values(), plan.sizes)):
            out.append(grads[off:off + n].view(shape) if ctx.needs_input_grad[6 + i] else None)
            off += n
        return (None,) * 6 + tuple(out) + _x_grad(ctx.x_in, dX)


def sequence_log_probs_batch(plan: SeqPlan, params, X, S, mask, residue_idx, chain_enc, ranks, offsets, k_neighbors: int, p_mpnn: float,
                             min_len=None, max_len=None):
    """log_probs [T,21] of a packed batch with a graph over ``params``: one forward and one backward for all its proteins. The six
    inputs are packed tensors ([T,4,3] and [T]) with ``offsets`` [n + 1], or lists of per-protein tensors, which are packed here
    (``offsets`` may then be None). One K = min(k_neighbors, shortest protein) serves the batch; proteins shorter than ``k_neighbors``
    need a batch of one length. ``min_len`` / ``max_len`` default to the lengths ``offsets`` gives. Reads the device status word (a
    stream sync) and raises through tmpnn_status_error. Dropout rows are numbered over the packed rows, so a protein's masks depend
    on its place in the batch."""
    from .autograd import _draw_key
    if params[0].device.type != "cuda":
        raise RuntimeError(_CPU_ERROR)
    dev = params[0].device
    if isinstance(S, (list, tuple)):
        lens = [int(s.numel()) for s in S]
        offsets = [0]
        for n in lens:
            offsets.append(offsets[-1] + n)
        X, S, mask, residue_idx, chain_enc, ranks = (torch.cat([t.to(dev) for t in ts]) for ts in (X, S, mask, residue_idx, chain_enc, ranks))
    inp = SeqBatchInputs(*(t.to(dev) for t in (X, S, mask, residue_idx, chain_enc, ranks)), offsets, k_neighbors, min_len, max_len)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    seed, step = _draw_key() if p_mpnn > 0 else (0, 0)
    extra = (X.to(dev),) if _wants_dx(X) else ()          # the packed coordinates with their graph: one more input of the node
    log_probs = SeqBatchFunction.apply(plan, inp, status, float(p_mpnn), seed, step, *params, *extra)
    st = int(status.item())
    if st:
        check(plan.lib.tmpnn_status_error(st), "tmpnn_seqloss_batch_forward")
    return log_probs


class ProteinMPNN(nn.Module):
    """Constructor / forward signature and state-dict names of the reference's training class (model_utils.py:396-470); a checkpoint
    of ``protein_mpnn_utils.ProteinMPNN`` loads into it and the other way round."""

    # Opt-in packed training: with packed = True, forward runs the [B, L] batch as ONE device call over B segments of L rows (padding
    # rows included, exactly what the loop feeds each member) and one autograd node, and draws one dropout key per forward where the
    # loop draws B. log_probs are the loop's bit for bit without dropout; gradients agree to rounding (the weight gradients' fixed row
    # blocks run over the packed rows). A batch of one takes the per-protein call either way.
    packed = False

    def __init__(self, num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3,
                 num_decoder_layers=3, vocab=21, k_neighbors=32, augment_eps=0.1, dropout=0.1):
        super().__init__()
        if (num_letters, node_features, edge_features, hidden_dim, vocab) != (21, 128, 128, 128, 21) or \
                (num_encoder_layers, num_decoder_layers) != (3, 3):
            raise NotImplementedError("the HIP engine is specialised for 21 letters, 128-d features, 3 encoder + 3 decoder layers")
        if not 1 <= int(k_neighbors) <= 48:
            raise NotImplementedError(f"k_neighbors={k_neighbors}: this build supports 1..48")
        if float(dropout) not in (0.0, MPNN_DROPOUT):
            raise NotImplementedError(f"dropout={dropout}: the training kernels draw their masks at p = 0.1 (or 0.0: none)")
        self.node_features, self.edge_features, self.hidden_dim = node_features, edge_features, hidden_dim
        self.k_neighbors, self.augment_eps, self.dropout = int(k_neighbors), float(augment_eps or 0.0), float(dropout)
        _register_tree(self, _weights.mpnn_param_shapes())
        self._plan: Optional[SeqPlan] = None

    def forward(self, X, S, mask, chain_M, residue_idx, chain_encoding_all, randn=None):
        """-> log_probs [B, L, 21]. The decoding order is ``decoding_ranks(chain_M * mask, randn)`` (:452-456)."""
        params = [p for _, p in self.named_parameters()]
        if params[0].device.type != "cuda":
            raise RuntimeError(_CPU_ERROR)
        if self._plan is None:
            self._plan = SeqPlan()
        if self.training and self.augment_eps > 0:
            X = X + self.augment_eps * torch.randn_like(X)                                   # :341
        chain_M = chain_M * mask
        if randn is None:
            randn = torch.randn(chain_M.shape, device=chain_M.device)
        ranks = decoding_ranks(chain_M, randn.to(chain_M.device))
        p = self.dropout if self.training else 0.0
        B, L = int(S.shape[0]), int(S.shape[1])
        if self.packed and B > 1:
            flat = lambda t: t.reshape((B * L,) + tuple(t.shape[2:]))
            out = sequence_log_probs_batch(self._plan, params, flat(X), flat(S), flat(mask), flat(residue_idx), flat(chain_encoding_all),
                                           flat(ranks), list(range(0, B * L + 1, L)), self.k_neighbors, p)
            return out.view(B, L, 21)
        out = [sequence_log_probs(self._plan, params, X[b], S[b], mask[b], residue_idx[b], chain_encoding_all[b], ranks[b],
                                  self.k_neighbors, p) for b in range(X.shape[0])]
        return torch.stack(out)


def loss_nll(S, log_probs, mask):
    """Negative log probabilities (:128-137) -> (loss [B,L], its masked mean, argmax hits [B,L])."""
    criterion = torch.nn.NLLLoss(reduction="none")
    loss = criterion(log_probs.contiguous().view(-1, log_probs.size(-1)), S.contiguous().view(-1)).view(S.size())
    S_argmaxed = torch.argmax(log_probs, -1)
    true_false = (S == S_argmaxed).float()
    loss_av = torch.sum(loss * mask) / torch.sum(mask)
    return loss, loss_av, true_false


def loss_smoothed(S, log_probs, mask, weight=0.1):
    """Label-smoothed negative log probabilities (:140-150) -> (loss [B,L], sum(loss * mask) / 2000.0)."""
    S_onehot = torch.nn.functional.one_hot(S, 21).float()
    S_onehot = S_onehot + weight / float(S_onehot.size(-1))
    S_onehot = S_onehot / S_onehot.sum(-1, keepdim=True)
    loss = -(S_onehot * log_probs).sum(-1)
    loss_av = torch.sum(loss * mask) / 2000.0
    return loss, loss_av


class NoamOpt:
    """Optimiser wrapper with the warm-up schedule of the reference (:474-507)."""

    def __init__(self, model_size, factor, warmup, optimizer, step):
        self.optimizer = optimizer
        self._step = step
        self.warmup = warmup
        self.factor = factor
        self.model_size = model_size
        self._rate = 0

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    def step(self):
        self._step += 1
        rate = self.rate()
        for p in self.optimizer.param_groups:
            p["lr"] = rate
        self._rate = rate
        self.optimizer.step()

    def rate(self, step=None):
        if step is None:
            step = self._step
        return self.factor * (self.model_size ** (-0.5) * min(step ** (-0.5), step * self.warmup ** (-1.5)))

    def zero_grad(self):
        self.optimizer.zero_grad()


def get_std_opt(parameters, d_model, step):
    return NoamOpt(d_model, 2, 4000, torch.optim.Adam(parameters, lr=0, betas=(0.9, 0.98), eps=1e-9), step)
