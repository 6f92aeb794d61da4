"""Thin Python glue over the C-ABI: torch owns device memory and streams (plumbing), libtmpnn.so does
all arithmetic. Every method takes/returns torch CUDA tensors and launches on the current stream."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import weights as _weights
from ._lib import HID, KS, VOCAB, TmpnnError, TmpnnRangeError, check


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise TmpnnError("the ThermoMPNN HIP engine needs CUDA (ROCm) tensors; there is no CPU path")


_selftested: set = set()


def _selftest(lib, device) -> None:
    """tmpnn_selftest once per (library, device) and process: a library built with flags that break the f16x2 overflow
    detection or the persistent tile loops must not produce numbers. One tiny launch + a 4-byte read-back."""
    key = (id(lib), device.index)
    if key in _selftested:
        return
    st = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.tmpnn_selftest(_ptr(st), _stream()), "tmpnn_selftest")
    check(lib.tmpnn_status_error(int(st.item())), "tmpnn_selftest")
    _selftested.add(key)


def range_retry(run, used: str, retry: Optional[str], what: str, stacklevel: int = 2) -> None:
    """The range contract of every checked call. ``run(precision)`` makes the call's launches at that precision and returns the
    device status word. A RANGE bit after an f16x2 run (an operand left the fp16 range) with a ``retry`` precision to go to: one
    RuntimeWarning, attributed ``stacklevel`` frames up as ``warnings.warn`` counts them from the CALLER of this function, and one
    rerun at ``retry``. Whatever bits are left, rerun or not, raise through tmpnn_status_error (TmpnnRangeError for RANGE)."""
    st = run(used)
    if st & _lib.STATUS_RANGE and not st & _lib.STATUS_MAXLEN and used == "f16x2" and retry and retry != used:
        warnings.warn(f"ThermoMPNN HIP engine: non-finite result in {used} (an operand left the fp16 range); "
                      f"rerunning this batch at precision {retry}", RuntimeWarning, stacklevel=stacklevel + 1)
        used = retry
        st = run(retry)
    if st:
        check(_lib.load().tmpnn_status_error(st), f"tmpnn_{what}[{used}]")


class Weights:
    """Device-resident weight set + the native handle (tmpnn_weights_create)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device, with_head: Optional[bool] = None,
                 precision: Optional[str] = None, tensors: Optional[List[torch.Tensor]] = None, ca_only: Optional[bool] = None):
        """``ca_only``: the C-alpha-only flavour (a ProteinMPNN(ca_only=True) state dict: tmpnn_weights_create_ca); None detects it by
        the edge embedding's 167 inputs. The five parameters of such a state dict that its forward never reads are dropped.
        ``precision``: "f16x2" | "bf16x3" | "fp32" (matrix-core path of every call through this handle) or None for
        the library default. ``tensors``: device tensors of another Weights of the same model to share (a second handle
        costs only its derived data: 0.8 MB of tables, plus 7.2 MB of f16 fragment images for an "f16x2" handle)."""
        lib = _lib.load()
        if precision is not None and precision not in _lib.PRECISIONS:
            raise TmpnnError(f"precision={precision!r}: expected one of {_lib.PRECISIONS}")
        device = torch.device(device)
        if device.type != "cuda":
            raise TmpnnError("weights must live on a CUDA (ROCm) device")
        names = _lib.tensor_names()
        sd = dict(state_dict)
        if ca_only is None:
            ca_only = _weights.is_ca_state_dict(sd)
        if ca_only and with_head:
            raise ValueError("a ca_only model has no ddG head (ThermoMPNN has no CA flavour)")
        if with_head is None:
            with_head = not ca_only and all(n in sd for n in names[_lib.N_MPNN_TENSORS:])
        n = _lib.N_TENSORS if with_head else _lib.N_MPNN_TENSORS
        numel = lib.tmpnn_tensor_numel_ca if ca_only else lib.tmpnn_tensor_numel
        self.tensors: List[torch.Tensor] = list(tensors) if tensors is not None else []
        for i, name in enumerate(names[:n] if tensors is None else []):
            key = name if i >= _lib.N_MPNN_TENSORS else ("prot_mpnn." + name if ("prot_mpnn." + name) in sd else name)
            if key not in sd:
                raise KeyError(f"state dict lacks {key!r}")
            t = sd[key].detach().to(device=device, dtype=torch.float32).contiguous()
            if t.numel() != numel(i):
                raise TmpnnError(f"{key}: {t.numel()} elements, engine expects {numel(i)}")
            if t.data_ptr() % 16:
                t = t.clone()
            self.tensors.append(t)
        self.device = device
        self.with_head = with_head
        self.ca_only = bool(ca_only)
        _selftest(lib, device)
        sizer, create = (lib.tmpnn_weights_ca_packed_bytes_p, lib.tmpnn_weights_create_ca) if ca_only else \
            (lib.tmpnn_weights_packed_bytes_p, lib.tmpnn_weights_create_p)
        nbytes = sizer(precision.encode() if precision else None) or lib.tmpnn_weights_packed_bytes()
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=device)      # (0 = unknown name: create_p reports it)
        arr = (C.c_void_p * n)(*[t.data_ptr() for t in self.tensors])
        self.handle = C.c_void_p()
        with torch.cuda.device(device):
            check(create(C.byref(self.handle), arr, n, _ptr(self.packed), self.packed.numel(),
                         precision.encode() if precision else None, _stream()), "tmpnn_weights_create_ca" if ca_only else "tmpnn_weights_create_p")
        self.precision = lib.tmpnn_weights_precision(self.handle).decode()

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _lib.load().tmpnn_weights_destroy(h)
            except Exception:      # interpreter shutdown: the library may already be gone
                pass
            self.handle = None


class EncodedBackbone:
    """What ``Engine.encode`` leaves on the device for ``Engine.decode_variants``: the opaque ctx buffer of tmpnn_encode (k-NN
    graph, final edge features, encoder node state, decoder layer 0's sequence-free projection), the mask and offsets of the
    packed batch, its length T and the precision it was made at (a ctx is decoded by a handle of the same precision). ``inputs``
    keeps the backbone tensors for the range retry, which has to encode again at another precision."""

    def __init__(self, ctx: torch.Tensor, mask: torch.Tensor, offsets: torch.Tensor, T: int, precision: str, inputs: tuple):
        self.ctx, self.mask, self.offsets, self.T, self.precision, self.inputs = ctx, mask, offsets, int(T), precision, inputs

    @property
    def E_idx(self) -> torch.Tensor:
        """The k-NN graph [T,48] (global rows of the packed batch, -1 = no neighbour): the first array of the ctx."""
        return self.ctx[: self.T * KS * 4].view(torch.int32).view(self.T, KS)


class Engine:
    """One weight set on one GPU. All tensors are packed along the residue axis (T = sum of lengths)."""

    def __init__(self, state_dict, device="cuda", k_neighbors: int = 48, precision: Optional[str] = None,
                 retry_precision: Optional[str] = "bf16x3", with_head: Optional[bool] = None, ca_only: Optional[bool] = None):
        """``ca_only``: a ProteinMPNN(ca_only=True) weight set (None: detected by the edge embedding's shape); ``X`` stays [T,4,3] in
        every call, with only slot 1 (C-alpha) read, and ``want_ddg`` is refused.
        ``precision``: matrix-core path of the per-edge GEMMs ("f16x2" default | "bf16x3" | "fp32").
        ``retry_precision``: when a forward in f16x2 leaves the finite range (an operand >= 65504 overflowed fp16), it is
        rerun once at this precision with a warning (None: raise TmpnnRangeError instead)."""
        self.lib = _lib.load()
        self.w = Weights(state_dict, device, with_head=with_head, precision=precision, ca_only=ca_only)
        self.ca_only = self.w.ca_only
        self.device = self.w.device
        self.precision = self.w.precision
        self.retry_precision = retry_precision
        if not 1 <= int(k_neighbors) <= KS:
            raise TmpnnError(f"k_neighbors={k_neighbors} outside [1, {KS}]")
        self.K = int(k_neighbors)
        self._ws: Optional[torch.Tensor] = None
        self._alt: Dict[str, Weights] = {self.precision: self.w}
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def weights_for(self, precision: str) -> Weights:
        """The handle for ``precision`` (created on first use; shares the raw tensors)."""
        if precision not in self._alt:
            self._alt[precision] = Weights({}, self.device, with_head=self.w.with_head, precision=precision,
                                           tensors=self.w.tensors, ca_only=self.ca_only)
        return self._alt[precision]

    def _raise_status(self, what: str, status: Optional[torch.Tensor] = None) -> int:
        """Reads the device status word (ONE 4-byte D2H copy = a stream sync) and raises on TMPNN_STATUS_MAXLEN;
        returns the remaining bits (TMPNN_STATUS_RANGE is the caller's to handle)."""
        st = int((self._status if status is None else status).item())
        if st & _lib.STATUS_MAXLEN:
            check(self.lib.tmpnn_status_error(_lib.STATUS_MAXLEN), what)
        return st

    @staticmethod
    def _max_len(offsets, given: Optional[int]) -> int:
        """Longest protein of the batch. Derived from ``offsets`` whenever that costs no device sync (host data);
        a caller-supplied value is only trusted for device-resident offsets (the kernel still guards it and reports
        TMPNN_STATUS_MAXLEN instead of overrunning its scratch)."""
        if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda):
            o = np.asarray(offsets).astype(np.int64)
            true_len = int((o[1:] - o[:-1]).max()) if o.size > 1 else 0
            if given is not None and given < true_len:
                raise TmpnnError(f"max_len={given} is smaller than the longest protein ({true_len})")
            return max(true_len, 1) if given is None else int(given)
        if given is not None:
            return int(given)
        return int((offsets[1:] - offsets[:-1]).max().item()) if offsets.numel() > 1 else 0

    # -- buffers ---------------------------------------------------------------------------------
    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _i32(self, t) -> torch.Tensor:
        return torch.as_tensor(t).to(device=self.device, dtype=torch.int32).contiguous()

    def _f32(self, t) -> torch.Tensor:
        return torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous()

    # -- individual operators (parity tests drive these) --------------------------------------------
    def knn_topk(self, X, mask, offsets, max_len: Optional[int] = None):
        max_len = self._max_len(offsets, max_len)
        X, mask, offsets = self._f32(X), self._f32(mask), self._i32(offsets)
        T, N = X.shape[0], offsets.numel() - 1
        E_idx = torch.empty((T, KS), dtype=torch.int32, device=self.device)
        D_nb = torch.empty((T, KS), dtype=torch.float32, device=self.device)
        self._status.zero_()
        check(self.lib.tmpnn_knn_topk(_ptr(X), _ptr(mask), _ptr(offsets), N, T, max_len, self.K, _ptr(E_idx), _ptr(D_nb),
                                      _ptr(self._status), _stream()), "tmpnn_knn_topk")
        self._raise_status("tmpnn_knn_topk")
        return E_idx, D_nb

    def centrality(self, X, mask, offsets, radius: float = 10.0, out: Optional[torch.Tensor] = None):
        X, mask, offsets = self._f32(X), self._f32(mask), self._i32(offsets)
        if out is None:
            out = torch.empty(X.shape[0], dtype=torch.int32, device=self.device)
        check(self.lib.tmpnn_centrality(_ptr(X), _ptr(mask), _ptr(offsets), offsets.numel() - 1, X.shape[0], float(radius),
                                        _ptr(out), _stream()), "tmpnn_centrality")
        return out

    def ca_frames(self, X, offsets):
        """_orientations_coarse's frames O [T,9] of the packed batch (tmpnn_ca_frames): X [T,4,3] (slot 1 read), a segment per protein."""
        X, offsets = self._f32(X), self._i32(offsets)
        _need_cuda(X)
        O = torch.empty((X.shape[0], 9), dtype=torch.float32, device=self.device)
        check(self.lib.tmpnn_ca_frames(_ptr(X), _ptr(offsets), offsets.numel() - 1, X.shape[0], _ptr(O), _stream()), "tmpnn_ca_frames")
        return O

    def edge_featurize(self, X, residue_idx, chain_enc, E_idx, D_nb, want_E: bool = False, offsets=None):
        """``offsets`` (a CA engine only): the proteins of the packed axis, default one protein [0, T)."""
        X, ridx, cenc = self._f32(X), self._i32(residue_idx), self._i32(chain_enc)
        T = X.shape[0]
        h_E = torch.empty((T, KS, HID), dtype=torch.float32, device=self.device)
        E = torch.empty_like(h_E) if want_E else None
        if self.ca_only:
            offsets = self._i32([0, T] if offsets is None else offsets)
            O = self.ca_frames(X, offsets)
            check(self.lib.tmpnn_edge_featurize_ca(self.w.handle, _ptr(X), _ptr(ridx), _ptr(cenc), _ptr(offsets), offsets.numel() - 1,
                                                   _ptr(E_idx), _ptr(D_nb), _ptr(O), T, _ptr(h_E), _ptr(E), _stream()),
                  "tmpnn_edge_featurize_ca")
            return (h_E, E) if want_E else h_E
        check(self.lib.tmpnn_edge_featurize(self.w.handle, _ptr(X), _ptr(ridx), _ptr(cenc), _ptr(E_idx), _ptr(D_nb), T,
                                            _ptr(h_E), _ptr(E), _stream()), "tmpnn_edge_featurize")
        return (h_E, E) if want_E else h_E

    def enc_layer(self, layer: int, h_V, h_E, E_idx, mask):
        T = h_V.shape[0]
        ws = self._workspace(self.lib.tmpnn_layer_workspace_bytes(T))
        check(self.lib.tmpnn_enc_layer(self.w.handle, layer, _ptr(h_V), _ptr(h_E), _ptr(E_idx), _ptr(mask), T, _ptr(ws),
                                       ws.numel(), _stream()), "tmpnn_enc_layer")
        return h_V, h_E

    def dec_layer(self, layer: int, h_V, h_E, E_idx, S, mask):
        T = h_V.shape[0]
        out = torch.empty_like(h_V)
        ws = self._workspace(self.lib.tmpnn_layer_workspace_bytes(T))
        check(self.lib.tmpnn_dec_layer(self.w.handle, layer, _ptr(h_V), _ptr(out), _ptr(h_E), _ptr(E_idx), _ptr(S),
                                       _ptr(mask), T, _ptr(ws), ws.numel(), _stream()), "tmpnn_dec_layer")
        return out

    def seq_embed(self, S):
        S = self._i32(S)
        out = torch.empty((S.numel(), HID), dtype=torch.float32, device=self.device)
        check(self.lib.tmpnn_seq_embed(self.w.handle, _ptr(S), S.numel(), _ptr(out), _stream()), "tmpnn_seq_embed")
        return out

    def log_probs(self, h_V):
        out = torch.empty((h_V.shape[0], VOCAB), dtype=torch.float32, device=self.device)
        check(self.lib.tmpnn_log_probs(self.w.handle, _ptr(h_V), h_V.shape[0], _ptr(out), None, _stream()), "tmpnn_log_probs")
        return out

    def ddg_head(self, hV_last, hV_prev, S, want_z: bool = False):
        S = self._i32(S)
        T = S.numel()
        ddg = torch.empty((T, VOCAB), dtype=torch.float32, device=self.device)
        z = torch.empty_like(ddg) if want_z else None
        check(self.lib.tmpnn_ddg_head(self.w.handle, _ptr(hV_last), _ptr(hV_prev), _ptr(S), T, _ptr(ddg), _ptr(z),
                                      None, _stream()), "tmpnn_ddg_head")
        return (ddg, z) if want_z else ddg

    def ddg_head_generic(self, hidden: Sequence[torch.Tensor], S, Ws: torch.Tensor, mlp_w: Sequence[torch.Tensor],
                         mlp_b: Sequence[torch.Tensor], ddg_w: torch.Tensor, ddg_b: torch.Tensor,
                         conv_w: Optional[torch.Tensor] = None, conv_b: Optional[torch.Tensor] = None, want_z: bool = False):
        """The head of ANY TransferModel configuration (tmpnn_ddg_head_generic): ``hidden`` = the decoder states that enter the
        input, LAST layer first (all_mpnn_hid[:num_final_layers], transfer_model.py:84-85); ``conv_w`` [D0, D0, 9] / ``conv_b``
        = LightAttention's feature convolution or None; ``mlp_w[l]`` / ``mlp_b[l]`` = both_out's Linear l. -> ddg [T,21] (, z)."""
        S = self._i32(S)
        T = S.numel()
        f = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        hidden = [f(h) for h in hidden]
        mlp_w, mlp_b = [f(w) for w in mlp_w], [f(b) for b in mlp_b]
        Ws, ddg_w, ddg_b, conv_w, conv_b = f(Ws), f(ddg_w), f(ddg_b), f(conv_w), f(conv_b)
        _need_cuda(S, Ws, *hidden)
        n_layers = len(mlp_w)
        dims = [HID * len(hidden) + HID] + [int(w.shape[0]) for w in mlp_w]
        for l, w in enumerate(mlp_w):
            if tuple(w.shape) != (dims[l + 1], dims[l]) or mlp_b[l].numel() != dims[l + 1]:
                raise TmpnnError(f"both_out Linear {l}: weight {tuple(w.shape)}, expected {(dims[l + 1], dims[l])}")
        if conv_w is not None and tuple(conv_w.shape) != (dims[0], dims[0], 9):
            raise TmpnnError(f"feature_convolution weight {tuple(conv_w.shape)}, expected {(dims[0], dims[0], 9)}")
        cdims = (C.c_int32 * len(dims))(*dims)
        arr = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
        need = self.lib.tmpnn_head_generic_workspace_bytes(T, len(hidden), n_layers, cdims)
        if T > 0 and need == 0:
            raise TmpnnError(f"head dims {dims} (num_final_layers {len(hidden)}): not a TransferModel head layout")
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        ddg = torch.empty((T, VOCAB), dtype=torch.float32, device=self.device)
        z = torch.empty_like(ddg) if want_z else None
        self._status.zero_()
        check(self.lib.tmpnn_ddg_head_generic(arr(hidden), len(hidden), _ptr(Ws), _ptr(S), T, _ptr(conv_w), _ptr(conv_b), n_layers,
                                              arr(mlp_w), arr(mlp_b), cdims, _ptr(ddg_w), _ptr(ddg_b), _ptr(ddg), _ptr(z), _ptr(ws),
                                              ws.numel(), _ptr(self._status), _stream()), "tmpnn_ddg_head_generic")
        st = self._raise_status("tmpnn_ddg_head_generic")
        if st:
            check(self.lib.tmpnn_status_error(st), "tmpnn_ddg_head_generic")
        return (ddg, z) if want_z else ddg

    def gather_rows(self, nodes, idx_i32):
        nodes = nodes.contiguous()
        idx = idx_i32.contiguous()
        out = torch.empty((idx.numel(), nodes.shape[-1]), dtype=torch.float32, device=nodes.device)
        check(self.lib.tmpnn_gather_rows_i32(_ptr(nodes), _ptr(idx), idx.numel(), nodes.shape[-1], _ptr(out), _stream()),
              "tmpnn_gather_rows_i32")
        return out

    # -- the fused path -----------------------------------------------------------------------------
    def ssm_forward(self, X, S, mask, residue_idx, chain_enc, offsets, max_len: Optional[int] = None,
                    want_ddg: bool = True, want_hidden: bool = False, want_log_probs: bool = False,
                    want_E_idx: bool = False, out: Optional[dict] = None, check_status: bool = True,
                    precision: Optional[str] = None, _private: Optional[dict] = None):
        """Packed inputs ([T,4,3], [T], ...) -> dict(ddg [T,21], hidden [3,T,128], log_probs [T,21], E_idx [T,48]).

        ``check_status`` (default) reads the 4-byte device status word after the launches — one stream sync — and
          * raises if a protein is longer than ``max_len``,
          * on a non-finite ddG / log-probability (fp16 overflow of the f16x2 path) reruns the batch once at
            ``retry_precision`` with a warning, or raises TmpnnRangeError.
        Throughput loops pass ``check_status=False`` (nothing syncs; call ``check_last_status()`` when convenient).
        ``precision`` overrides the engine's precision for this call. (``_private``: workspace / status word owned by a
        captured graph instead of the engine's shared ones, see ``capture_graph``.)"""
        if want_ddg and self.ca_only:
            raise ValueError("ssm_forward: want_ddg with a ca_only engine (ThermoMPNN has no CA flavour); pass want_ddg=False")
        max_len = self._max_len(offsets, max_len)
        X, mask = self._f32(X), self._f32(mask)
        S, ridx, cenc, offsets = self._i32(S), self._i32(residue_idx), self._i32(chain_enc), self._i32(offsets)
        _need_cuda(X, S, mask)
        T, N = X.shape[0], offsets.numel() - 1
        res = out if out is not None else {}
        dev = self.device
        if want_ddg and "ddg" not in res:
            res["ddg"] = torch.empty((T, VOCAB), dtype=torch.float32, device=dev)
        if want_hidden and "hidden" not in res:
            res["hidden"] = torch.empty((3, T, HID), dtype=torch.float32, device=dev)
        if want_log_probs and "log_probs" not in res:
            res["log_probs"] = torch.empty((T, VOCAB), dtype=torch.float32, device=dev)
        if want_E_idx and "E_idx" not in res:
            res["E_idx"] = torch.empty((T, KS), dtype=torch.int32, device=dev)
        need = self.lib.tmpnn_workspace_bytes(T)
        if _private is not None:
            if _private.get("ws") is None or _private["ws"].numel() < need:
                _private["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
            if _private.get("status") is None:
                _private["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
            ws, status = _private["ws"], _private["status"]
        else:
            ws, status = self._workspace(need), self._status

        def run(precision: str) -> int:
            check(self.lib.tmpnn_ssm_forward(self.weights_for(precision).handle, _ptr(X), _ptr(S), _ptr(mask), _ptr(ridx), _ptr(cenc),
                                             _ptr(offsets), N, T, max_len, self.K, _ptr(res.get("ddg") if want_ddg else None),
                                             _ptr(res.get("hidden") if want_hidden else None),
                                             _ptr(res.get("log_probs") if want_log_probs else None),
                                             _ptr(res.get("E_idx") if want_E_idx else None), _ptr(status), _ptr(ws),
                                             ws.numel(), _stream()), "tmpnn_ssm_forward")
            return int(status.item()) if check_status and T > 0 and N > 0 else 0      # (ONE 4-byte D2H copy = a stream sync)

        range_retry(run, precision or self.precision, self.retry_precision, "ssm_forward")
        return res

    # -- ranked hit lists ------------------------------------------------------------------------------
    def select_hits(self, ddg, S, offsets, k: int, cutoff: Optional[float] = None, include_cys: bool = False,
                    one_per_position: bool = False) -> Dict[str, torch.Tensor]:
        """The ``k`` most stabilising substitutions of every protein of a packed table that is already on the device
        (tmpnn_select_hits: two launches, no table leaves the GPU): ``ddg`` [T, ld >= 20] float32 (``ssm_forward``'s table, rows of a
        scan's ``device_table``), ``S`` [T] the residues' own letters (>= 20: no residue), ``offsets`` [P + 1]. A candidate is a
        substitution a != S[t] of a residue with S[t] < 20 whose value is not NaN and <= ``cutoff`` (None: +inf), cysteine only with
        ``include_cys``; ``one_per_position`` first keeps each position's best candidate. -> dict(hit_ddg [P, k] padded with NaN,
        hit_pos [P, k] local positions and hit_aa [P, k] padded with -1, hit_count [P]) on the device, best first: ascending (value,
        position, letter), -0.0 taken as +0.0. 1 <= k <= 256; every protein <= 8192 residues."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 2:
            raise TmpnnError("select_hits: ddg must be a float32 [T, ld] tensor on the device (the table stays there; there is no CPU path)")
        if ddg.shape[0] > 0 and (ddg.stride(1) != 1 or ddg.stride(0) < ddg.shape[1]):
            ddg = ddg.contiguous()
        T, ld = int(ddg.shape[0]), int(ddg.stride(0)) if ddg.shape[0] > 0 else int(ddg.shape[1])
        if not 1 <= int(k) <= _lib.HITS_MAX_K:
            raise TmpnnError(f"select_hits: k={k} outside [1, {_lib.HITS_MAX_K}]")
        cut = float("inf") if cutoff is None else float(cutoff)
        if cut != cut:
            raise TmpnnError("select_hits: the cutoff is NaN")
        longest = self._max_len(offsets, None)
        if longest > _lib.HITS_MAX_LEN:
            raise TmpnnError(f"select_hits: a protein of {longest} residues exceeds {_lib.HITS_MAX_LEN}, the forward's own bound")
        S, offsets = self._i32(S), self._i32(offsets)
        P = offsets.numel() - 1
        if S.numel() != T or P < 0:
            raise TmpnnError(f"select_hits: S has {S.numel()} entries for a table of {T} rows, offsets {offsets.numel()}")
        dev, k = self.device, int(k)
        res = dict(hit_ddg=torch.empty((P, k), dtype=torch.float32, device=dev), hit_pos=torch.empty((P, k), dtype=torch.int32, device=dev),
                   hit_aa=torch.empty((P, k), dtype=torch.int32, device=dev), hit_count=torch.empty(P, dtype=torch.int32, device=dev))
        if P == 0:
            return res
        if T == 0:                                                  # proteins without a row: padding, no launch (an empty table has no address)
            res["hit_ddg"].fill_(float("nan"))
            res["hit_pos"].fill_(-1)
            res["hit_aa"].fill_(-1)
            res["hit_count"].zero_()
            return res
        need = self.lib.tmpnn_hits_workspace_bytes(T, P, k)
        if need == 0:
            raise TmpnnError(f"select_hits: sizes not served (T={T}, P={P}, k={k})")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)       # (its own buffer: a scan's writer thread may call this beside a forward)
        flags = (_lib.HITS_INCLUDE_CYS if include_cys else 0) | (_lib.HITS_ONE_PER_POSITION if one_per_position else 0)
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_select_hits(_ptr(ddg), ld, _ptr(S), _ptr(offsets), P, T, k, cut, flags, _ptr(res["hit_ddg"]),
                                             _ptr(res["hit_pos"]), _ptr(res["hit_aa"]), _ptr(res["hit_count"]), _ptr(ws), ws.numel(),
                                             _stream()), "tmpnn_select_hits")
        return res

    def select_variant_hits(self, ddg, S_var, base, tag, k: int, skip=None, cutoff: Optional[float] = None, include_cys: bool = False,
                            upper: bool = False, state: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The ``k`` smallest values ``base[v] + ddg[v, q, b]`` over a chunk of variant tables that is already on the device, and over
        what earlier calls left in ``state`` (tmpnn_select_variant_hits: two launches): ``ddg`` [V, L, ld >= 20] float32
        (``decode_variants``' tables), ``S_var`` [V, L] the variants' own letters, and per variant ``base`` [V] (float32), ``tag`` [V]
        (0 .. 65535, distinct over all calls of one selection) and ``skip`` [V] (a position without candidates; None or -1: none).
        A candidate is a substitution b != S_var[v, q] of a residue with S_var[v, q] < 20 at q != skip[v] (``upper``: q > skip[v])
        whose sum — one fp32 add — is not NaN and <= ``cutoff`` (None: +inf), cysteine only with ``include_cys``. ``state=None``
        starts a selection; passing back the returned ``state`` (int64 [k], the 64-bit keys; updated in place) continues it, and the
        result does not depend on how the variants were cut into calls. -> dict(hit_ddg [k] padded with NaN, hit_tag / hit_pos /
        hit_aa [k] padded with -1, hit_count [1], state) on the device, best first: ascending (value, tag, position, letter), -0.0
        taken as +0.0. 1 <= k <= 256, L <= 2048, one protein per selection."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 3:
            raise TmpnnError("select_variant_hits: ddg must be a float32 [V, L, ld] tensor on the device (the tables stay there; there is no CPU path)")
        V, L, cols = (int(n) for n in ddg.shape)
        if V > 0 and L > 0 and (ddg.stride(2) != 1 or ddg.stride(1) < cols or ddg.stride(0) != L * ddg.stride(1)):
            ddg = ddg.contiguous()
        ld = int(ddg.stride(1)) if V > 0 and L > 0 else cols
        if not 1 <= int(k) <= _lib.HITS_MAX_K:
            raise TmpnnError(f"select_variant_hits: k={k} outside [1, {_lib.HITS_MAX_K}]")
        cut = float("inf") if cutoff is None else float(cutoff)
        if cut != cut:
            raise TmpnnError("select_variant_hits: the cutoff is NaN")
        if L > _lib.VHITS_MAX_LEN:
            raise TmpnnError(f"select_variant_hits: L={L} residues exceed {_lib.VHITS_MAX_LEN}, the key's 11 position bits")
        dev, k = self.device, int(k)
        S_var, tag = self._i32(S_var), self._i32(tag)
        skip = torch.full((V,), -1, dtype=torch.int32, device=dev) if skip is None else self._i32(skip)
        base = self._f32(base)
        if tuple(S_var.shape) != (V, L) or base.numel() != V or tag.numel() != V or skip.numel() != V:
            raise TmpnnError(f"select_variant_hits: tables {(V, L, cols)} need S_var [V, L] and base, tag, skip [V]; got "
                             f"{tuple(S_var.shape)}, {base.numel()}, {tag.numel()}, {skip.numel()}")
        flags = (_lib.VHITS_INCLUDE_CYS if include_cys else 0) | (_lib.VHITS_UPPER if upper else 0)
        if state is not None:
            if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.int64 or tuple(state.shape) != (k,) or \
                    not state.is_contiguous():
                raise TmpnnError(f"select_variant_hits: state must be the int64 [{k}] device tensor an earlier call with k={k} returned")
            flags |= _lib.VHITS_CONTINUE
        else:
            state = torch.empty(k, dtype=torch.int64, device=dev)
        need = self.lib.tmpnn_variant_hits_workspace_bytes(V, L, k)
        if need == 0:
            raise TmpnnError(f"select_variant_hits: sizes not served (V={V}, L={L}, k={k})")
        res = dict(hit_ddg=torch.empty(k, dtype=torch.float32, device=dev), hit_tag=torch.empty(k, dtype=torch.int32, device=dev),
                   hit_pos=torch.empty(k, dtype=torch.int32, device=dev), hit_aa=torch.empty(k, dtype=torch.int32, device=dev),
                   hit_count=torch.empty(1, dtype=torch.int32, device=dev), state=state)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_select_variant_hits(_ptr(ddg), ld, _ptr(S_var), _ptr(base), _ptr(tag), _ptr(skip), V, L, k, cut, flags,
                                                     _ptr(state), _ptr(res["hit_ddg"]), _ptr(res["hit_tag"]), _ptr(res["hit_pos"]),
                                                     _ptr(res["hit_aa"]), _ptr(res["hit_count"]), _ptr(ws), ws.numel(), _stream()),
                  "tmpnn_select_variant_hits")
        return res

    def beam_step(self, ddg, S_var, score, muts, depth: int, k: int, allowed=None, cutoff: Optional[float] = None,
                  include_cys: bool = False) -> Dict[str, torch.Tensor]:
        """One step of a beam search over n-point mutants, all on the device (tmpnn_beam_step: three launches): from the V members of
        a beam — ``ddg`` [V, L, ld >= 20] float32 (``decode_variants``' tables of the members), ``S_var`` [V, L] their letters,
        ``score`` [V] their cumulative ddG, ``muts`` [V, depth - 1] their substitutions as q << 5 | b, ascending (None when
        ``depth`` = 1; a member with a negative entry is dead) — the ``k`` best DISTINCT children of ``depth`` substitutions. A
        candidate is a substitution b != S_var[v, q] of a residue with S_var[v, q] < 20 at a position q that the member has not
        mutated and ``allowed`` [L] (None: all) marks nonzero, whose value score[v] + ddg[v, q, b] — one fp32 add — is not NaN and
        <= ``cutoff`` (None: +inf), cysteine only with ``include_cys``. Candidates that make the same set of substitutions are one
        child, represented by its smallest (value, parent slot, q, b). The caller promises that live members are distinct sets.
        -> dict(out_muts [k, depth] and out_parent [k] padded with -1, out_score [k] padded with NaN, out_S [k, L] int32 padded with
        20, out_count [1]) on the device, best first; a padded result can be decoded and stepped again as it is.
        1 <= depth <= 8, k * depth <= 256, L <= 2048, V <= 65536, one protein."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 3:
            raise TmpnnError("beam_step: ddg must be a float32 [V, L, ld] tensor on the device (the tables stay there; there is no CPU path)")
        V, L, cols = (int(n) for n in ddg.shape)
        if V > 0 and L > 0 and (ddg.stride(2) != 1 or ddg.stride(1) < cols or ddg.stride(0) != L * ddg.stride(1)):
            ddg = ddg.contiguous()
        ld = int(ddg.stride(1)) if V > 0 and L > 0 else cols
        depth, k = int(depth), int(k)
        if not 1 <= depth <= _lib.BEAM_MAX_DEPTH:
            raise TmpnnError(f"beam_step: depth={depth} outside [1, {_lib.BEAM_MAX_DEPTH}]")
        if k < 1 or k * depth > _lib.BEAM_MAX_KD:
            raise TmpnnError(f"beam_step: k={k} at depth {depth}: k must be at least 1 and k * depth at most {_lib.BEAM_MAX_KD}")
        cut = float("inf") if cutoff is None else float(cutoff)
        if cut != cut:
            raise TmpnnError("beam_step: the cutoff is NaN")
        if L > _lib.BEAM_MAX_LEN:
            raise TmpnnError(f"beam_step: L={L} residues exceed {_lib.BEAM_MAX_LEN}, the key's 11 position bits")
        if V > _lib.BEAM_MAX_V:
            raise TmpnnError(f"beam_step: V={V} members exceed {_lib.BEAM_MAX_V}, the key's 16 member bits")
        dev = self.device
        S_var, score = self._i32(S_var), self._f32(score)
        if muts is None:
            if depth > 1:
                raise TmpnnError(f"beam_step: depth {depth} needs muts [V, {depth - 1}]")
        else:
            muts = self._i32(muts)
            if tuple(muts.shape) != (V, depth - 1):
                raise TmpnnError(f"beam_step: muts must be [{V}, {depth - 1}] at depth {depth}, got {tuple(muts.shape)}")
            if depth == 1:
                muts = None
        if allowed is not None:
            allowed = self._i32(allowed)
            if allowed.numel() != L:
                raise TmpnnError(f"beam_step: allowed has {allowed.numel()} entries for {L} residues")
        if tuple(S_var.shape) != (V, L) or score.numel() != V:
            raise TmpnnError(f"beam_step: tables {(V, L, cols)} need S_var [V, L] and score [V]; got {tuple(S_var.shape)}, {score.numel()}")
        need = self.lib.tmpnn_beam_step_workspace_bytes(V, L, k, depth)
        if need == 0:
            raise TmpnnError(f"beam_step: sizes not served (V={V}, L={L}, k={k}, depth={depth})")
        res = dict(out_muts=torch.empty((k, depth), dtype=torch.int32, device=dev), out_score=torch.empty(k, dtype=torch.float32, device=dev),
                   out_parent=torch.empty(k, dtype=torch.int32, device=dev), out_S=torch.empty((k, L), dtype=torch.int32, device=dev),
                   out_count=torch.empty(1, dtype=torch.int32, device=dev))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        flags = _lib.BEAM_INCLUDE_CYS if include_cys else 0
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_beam_step(_ptr(ddg), ld, _ptr(S_var), _ptr(score), _ptr(muts), depth, _ptr(allowed), V, L, k, cut, flags,
                                           _ptr(res["out_muts"]), _ptr(res["out_score"]), _ptr(res["out_parent"]),
                                           _ptr(res["out_S"]) if L > 0 else None, _ptr(res["out_count"]), _ptr(ws), ws.numel(), _stream()),
                  "tmpnn_beam_step")
        return res

    def beam_step_each(self, ddg, S_var, score, muts, offsets, depth: int, k: int, allowed=None, cutoff: Optional[float] = None,
                       include_cys: bool = False, max_len: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``beam_step`` for the P proteins of a packed axis of T rows in one call (tmpnn_beam_step_each: three launches): ``ddg``
        [V, T, ld >= 20] float32 (``decode_variants``' tables over the pack: row v holds beam slot v of every protein), ``S_var``
        [V, T], ``score`` [P, V], ``muts`` [P, V, depth - 1] (q << 5 | b with q the position within the protein; None when ``depth``
        = 1), ``offsets`` [P + 1], ``allowed`` [T] or None. Protein p gets exactly what ``beam_step`` gives on its slice
        ddg[:, o_p : o_p + L_p], S_var[:, o_p : o_p + L_p], score[p], muts[p], allowed[o_p : o_p + L_p]: every bit, wherever it lies
        in the pack. -> dict(out_muts [P, k, depth], out_score [P, k], out_parent [P, k], out_count [P], out_S [k, T]) on the device;
        they are the next round's ``muts``, ``score`` and ``S_var`` as they stand. The device checks the offsets: a protein whose
        range is not inside [0, T], descends or is longer than ``max_len`` gets count -1 and padding, and its columns of ``out_S``
        keep the 20 they are allocated with. ``max_len``: the longest protein (derived from host offsets; needed with offsets on
        the device). 1 <= depth <= 8, k * depth <= 256, every protein <= 2048 rows, V <= 65536, V * T <= 2**31 - 1."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 3:
            raise TmpnnError("beam_step_each: ddg must be a float32 [V, T, ld] tensor on the device (the tables stay there; there is no CPU path)")
        V, T, cols = (int(n) for n in ddg.shape)
        if V > 0 and T > 0 and (ddg.stride(2) != 1 or ddg.stride(1) < cols or ddg.stride(0) != T * ddg.stride(1)):
            ddg = ddg.contiguous()
        ld = int(ddg.stride(1)) if V > 0 and T > 0 else cols
        depth, k = int(depth), int(k)
        if not 1 <= depth <= _lib.BEAM_MAX_DEPTH:
            raise TmpnnError(f"beam_step_each: depth={depth} outside [1, {_lib.BEAM_MAX_DEPTH}]")
        if k < 1 or k * depth > _lib.BEAM_MAX_KD:
            raise TmpnnError(f"beam_step_each: k={k} at depth {depth}: k must be at least 1 and k * depth at most {_lib.BEAM_MAX_KD}")
        cut = float("inf") if cutoff is None else float(cutoff)
        if cut != cut:
            raise TmpnnError("beam_step_each: the cutoff is NaN")
        if V > _lib.BEAM_MAX_V:
            raise TmpnnError(f"beam_step_each: V={V} members exceed {_lib.BEAM_MAX_V}, the key's 16 member bits")
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
            if max_len is None:
                raise TmpnnError("beam_step_each: offsets on the device need max_len (the device checks every protein against it)")
            max_len = int(max_len)
        else:                                                       # (host offsets may be wrong on purpose: the device refuses those proteins)
            o = np.asarray(offsets).astype(np.int64).reshape(-1)
            max_len = int(max_len) if max_len is not None else int(np.clip(o[1:] - o[:-1], 0, T).max()) if o.size > 1 else 0
        if not 0 <= max_len <= _lib.BEAM_MAX_LEN:
            raise TmpnnError(f"beam_step_each: max_len={max_len} residues outside [0, {_lib.BEAM_MAX_LEN}], the key's 11 position bits")
        dev = self.device
        S_var, score, offsets = self._i32(S_var), self._f32(score), self._i32(offsets).reshape(-1)
        P = offsets.numel() - 1
        if P < 0:
            raise TmpnnError("beam_step_each: offsets must hold P + 1 entries")
        if muts is None:
            if depth > 1:
                raise TmpnnError(f"beam_step_each: depth {depth} needs muts [P, V, {depth - 1}]")
        else:
            muts = self._i32(muts)
            if tuple(muts.shape) != (P, V, depth - 1):
                raise TmpnnError(f"beam_step_each: muts must be [{P}, {V}, {depth - 1}] at depth {depth}, got {tuple(muts.shape)}")
            if depth == 1:
                muts = None
        if allowed is not None:
            allowed = self._i32(allowed)
            if allowed.numel() != T:
                raise TmpnnError(f"beam_step_each: allowed has {allowed.numel()} entries for {T} rows")
        if tuple(S_var.shape) != (V, T) or tuple(score.shape) != (P, V):
            raise TmpnnError(f"beam_step_each: tables {(V, T, cols)} and {P} proteins need S_var [V, T] and score [P, V]; got "
                             f"{tuple(S_var.shape)}, {tuple(score.shape)}")
        res = dict(out_muts=torch.empty((P, k, depth), dtype=torch.int32, device=dev), out_score=torch.empty((P, k), dtype=torch.float32, device=dev),
                   out_parent=torch.empty((P, k), dtype=torch.int32, device=dev), out_S=torch.full((k, T), 20, dtype=torch.int32, device=dev),
                   out_count=torch.empty(P, dtype=torch.int32, device=dev))
        if P == 0:
            return res
        need = self.lib.tmpnn_beam_step_each_workspace_bytes(P, V, max_len, k, depth)
        if need == 0 or V * T > 0x7fffffff:
            raise TmpnnError(f"beam_step_each: sizes not served (P={P}, V={V}, T={T}, max_len={max_len}, k={k}, depth={depth})")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        flags = _lib.BEAM_INCLUDE_CYS if include_cys else 0
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_beam_step_each(_ptr(ddg), ld, _ptr(S_var), _ptr(score), _ptr(muts), depth, _ptr(allowed), _ptr(offsets), P, T,
                                                V, max_len, k, cut, flags, _ptr(res["out_muts"]), _ptr(res["out_score"]),
                                                _ptr(res["out_parent"]), _ptr(res["out_S"]) if T > 0 else None, _ptr(res["out_count"]),
                                                _ptr(ws), ws.numel(), _stream()), "tmpnn_beam_step_each")
        return res

    def pair_map(self, ddg, S_var, base, row, letter, wt, R: int, skip=None, include_cys: bool = False, upper: bool = False,
                 state: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """One chunk of variant tables that is already on the device reduced into a per-(row, position) state (tmpnn_pair_map: two
        launches): ``ddg`` [V, L, ld >= 20] float32 (``decode_variants``' tables), ``S_var`` [V, L] the variants' own letters, per
        variant ``base`` [V] (float32), ``row`` [V] (the state row, 0 .. R - 1), ``letter`` [V] (0 .. 19) and ``skip`` [V] (a position
        without candidates; None or -1: none), and the wild-type table ``wt`` [L, >= 20] float32 on the device. A candidate is a
        substitution b != S_var[v, q] of a residue with S_var[v, q] < 20 at q != skip[v] (``upper``: q > skip[v]), cysteine only
        with ``include_cys``; a variant whose row or letter is out of range contributes nothing. The variants of one row must be
        contiguous within a call (checked here when ``row`` is a numpy array or a list; a row may go on in the next call).
        ``state=None`` starts a map; passing back the returned dict continues it (updated in place), and its bits do not depend on
        how the variants were cut into calls. -> dict(best, eps_lo, eps_hi: int64 [R, L] keys, all ones = none; eps_abs_sum float32
        [R, L]; count int32 [R, L]) on the device: include/tmpnn.h has the key layout, ``decode_pair_map`` reads it. L <= 2048."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 3:
            raise TmpnnError("pair_map: ddg must be a float32 [V, L, ld] tensor on the device (the tables stay there; there is no CPU path)")
        V, L, cols = (int(n) for n in ddg.shape)
        if V > 0 and L > 0 and (ddg.stride(2) != 1 or ddg.stride(1) < cols or ddg.stride(0) != L * ddg.stride(1)):
            ddg = ddg.contiguous()
        ld = int(ddg.stride(1)) if V > 0 and L > 0 else cols
        if not isinstance(wt, torch.Tensor) or not wt.is_cuda or wt.dtype != torch.float32 or wt.dim() != 2 or int(wt.shape[0]) != L:
            raise TmpnnError(f"pair_map: wt must be a float32 [{L}, >= 20] tensor on the device, the wild type's table")
        if L > 0 and (wt.stride(1) != 1 or wt.stride(0) < wt.shape[1]):
            wt = wt.contiguous()
        ld_wt = int(wt.stride(0)) if L > 0 else int(wt.shape[1])
        R = int(R)
        if R < 0:
            raise TmpnnError(f"pair_map: R={R}")
        if L > _lib.PMAP_MAX_LEN:
            raise TmpnnError(f"pair_map: L={L} residues exceed {_lib.PMAP_MAX_LEN}")
        need = self.lib.tmpnn_pair_map_workspace_bytes(V, L)
        if need == 0 or R * L > 0x7fffffff:
            raise TmpnnError(f"pair_map: sizes not served (V={V}, L={L}, R={R})")
        if isinstance(row, (np.ndarray, list, tuple)):
            check_row_runs(row, R)
        dev = self.device
        S_var, row, letter = self._i32(S_var), self._i32(row), self._i32(letter)
        skip = torch.full((V,), -1, dtype=torch.int32, device=dev) if skip is None else self._i32(skip)
        base = self._f32(base)
        if tuple(S_var.shape) != (V, L) or base.numel() != V or row.numel() != V or letter.numel() != V or skip.numel() != V:
            raise TmpnnError(f"pair_map: tables {(V, L, cols)} need S_var [V, L] and base, row, letter, skip [V]; got "
                             f"{tuple(S_var.shape)}, {base.numel()}, {row.numel()}, {letter.numel()}, {skip.numel()}")
        flags = (_lib.PMAP_INCLUDE_CYS if include_cys else 0) | (_lib.PMAP_UPPER if upper else 0)
        if state is not None:
            for name, dt in _lib.PMAP_STATE:
                t = state.get(name) if isinstance(state, dict) else None
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != getattr(torch, dt) or tuple(t.shape) != (R, L) or \
                        not t.is_contiguous():
                    raise TmpnnError(f"pair_map: state[{name!r}] must be the {dt} [{R}, {L}] device tensor an earlier call returned")
            flags |= _lib.PMAP_CONTINUE
        else:
            state = {name: torch.empty((R, L), dtype=getattr(torch, dt), device=dev) for name, dt in _lib.PMAP_STATE}
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_pair_map(_ptr(ddg), ld, _ptr(S_var), _ptr(base), _ptr(row), _ptr(letter), _ptr(skip), _ptr(wt), ld_wt, V, L, R,
                                          flags, *[_ptr(state[name]) for name, _ in _lib.PMAP_STATE], _ptr(ws), ws.numel(), _stream()),
                  "tmpnn_pair_map")
        return state

    # -- conformer ensembles -------------------------------------------------------------------------
    def ensemble_stats(self, ddg, S, members: Sequence[int], lengths: Sequence[int], cutoff: Optional[float] = None,
                       rows=None) -> Dict[str, torch.Tensor]:
        """Per-mutation statistics across the members of conformer ensembles, from a packed table that is already on the device
        (tmpnn_ensemble_stats: one launch, no workspace): ``ddg`` [T, ld >= 20] float32 (``ssm_forward``'s table of the packed
        members), ``S`` [T] the rows' own letters (>= 20 or negative: the row takes no part), and per ensemble, on the host,
        ``members`` (M) and ``lengths`` (L): ensemble e is M[e] members of L[e] rows each, the ensembles contiguous and in order, so
        sum(M L) == T. -> dict(mean, spread, lo, hi float32 and lo_member, hi_member, count, below int32, each [sum(L), 20];
        offsets [E + 1] of the ensembles' output rows; status [E], 0 for every ensemble this method describes) on the device. The
        mean is a chain of fp32 adds in ascending member order, the spread the population form around it (include/tmpnn.h has the
        contract to the operation); ``below`` counts the members at or below ``cutoff`` (None: +inf). L <= 8192.
        ``rows`` (tmpnn_ensemble_stats_rows): an int32 [sum(M L)] row map, ``align_global``'s ``out`` as it is; member m's position q
        of ensemble e then reads table row ``rows[map0[e] + m L + q]`` (map0 = the running sum of M L) and is out where that entry is
        negative or >= T. The table may then have any number of rows: members of unequal length, packed ragged."""
        if not isinstance(ddg, torch.Tensor) or not ddg.is_cuda or ddg.dtype != torch.float32 or ddg.dim() != 2:
            raise TmpnnError("ensemble_stats: ddg must be a float32 [T, ld] tensor on the device (the table stays there; there is no CPU path)")
        if ddg.shape[0] > 0 and (ddg.stride(1) != 1 or ddg.stride(0) < ddg.shape[1]):
            ddg = ddg.contiguous()
        T, ld = int(ddg.shape[0]), int(ddg.stride(0)) if ddg.shape[0] > 0 else int(ddg.shape[1])
        cut = float("inf") if cutoff is None else float(cutoff)
        if cut != cut:
            raise TmpnnError("ensemble_stats: the cutoff is NaN")
        M, L = np.asarray(members, dtype=np.int64).reshape(-1), np.asarray(lengths, dtype=np.int64).reshape(-1)
        E = int(M.size)
        if L.size != E or (M < 0).any() or (L < 0).any():
            raise TmpnnError(f"ensemble_stats: members and lengths must be {E} non-negative numbers each, one per ensemble")
        if E > _lib.ENS_MAX_E:
            raise TmpnnError(f"ensemble_stats: {E} ensembles exceed {_lib.ENS_MAX_E} per call")
        max_len = int(L.max()) if E else 0
        if max_len > _lib.ENS_MAX_LEN:
            raise TmpnnError(f"ensemble_stats: an ensemble of {max_len} residues exceeds {_lib.ENS_MAX_LEN}, the forward's own bound")
        if rows is not None:
            rows = self._i32(rows).reshape(-1)
            if int((M * L).sum()) != rows.numel():
                raise TmpnnError(f"ensemble_stats: the ensembles describe {int((M * L).sum())} map entries, rows has {rows.numel()}")
            if T > 0x7fffffff:
                raise TmpnnError(f"ensemble_stats: {T} table rows exceed 2^31 - 1")
        elif int((M * L).sum()) != T:
            raise TmpnnError(f"ensemble_stats: the ensembles describe {int((M * L).sum())} rows, the table has {T}")
        S = self._i32(S)
        if S.numel() != T:
            raise TmpnnError(f"ensemble_stats: S has {S.numel()} entries for a table of {T} rows")
        out_off = np.concatenate([[0], np.cumsum(L)])
        T_out = int(out_off[-1])
        if T_out > 0x7fffffff:
            raise TmpnnError(f"ensemble_stats: {T_out} output rows exceed 2^31 - 1")
        row0 = np.concatenate([[0], np.cumsum(M * L)])[:-1]
        dev = self.device
        desc = torch.from_numpy(np.stack([row0, M, L, out_off[:-1]], axis=1).astype(np.int32).reshape(E, 4)).to(dev)
        res = {name: torch.empty((T_out, 20), dtype=getattr(torch, dt), device=dev) for name, dt in _lib.ENS_ARRAYS}
        res["offsets"] = torch.from_numpy(out_off.astype(np.int32)).to(dev)
        res["status"] = torch.zeros(E, dtype=torch.int32, device=dev)
        if E == 0:
            return res
        if rows is not None:
            R = int(rows.numel())
            with torch.cuda.device(dev):
                check(self.lib.tmpnn_ensemble_stats_rows(_ptr(ddg) if T > 0 else None, ld, _ptr(S) if T > 0 else None, _ptr(rows) if R > 0 else None,
                                                         R, _ptr(desc), E, T, T_out, max_len, cut,
                                                         *[_ptr(res[name]) if T_out > 0 else None for name, _ in _lib.ENS_ARRAYS],
                                                         _ptr(res["status"]), _stream()), "tmpnn_ensemble_stats_rows")
            return res
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_ensemble_stats(_ptr(ddg) if T > 0 else None, ld, _ptr(S) if T > 0 else None, _ptr(desc), E, T, T_out, max_len,
                                                cut, *[_ptr(res[name]) if T_out > 0 else None for name, _ in _lib.ENS_ARRAYS],
                                                _ptr(res["status"]), _stream()), "tmpnn_ensemble_stats")
        return res

    def superpose(self, X, mask, members: Sequence[int], lengths: Sequence[int], rows=None, fit_to=0) -> Dict[str, torch.Tensor]:
        """Rigid-body superposition of the members of conformer ensembles on the C-alpha atoms (tmpnn_superpose: two launches, no
        workspace), from the packed backbone that is already on the device: ``X`` [T, 4, 3] float32 (only atom slot 1 is read),
        ``mask`` [T], and per ensemble, on the host, ``members`` (M) and ``lengths`` (L) as ``ensemble_stats`` takes them; ``rows``:
        an int32 [sum(M L)] row map, ``align_global``'s ``out`` as it is (None: the identity map, and sum(M L) == T). ``fit_to``: the
        member every other member of its ensemble is laid on, one number for all ensembles or one per ensemble.
        -> dict(n_fit [NM] int32: the columns valid in the member and in the fit target; rmsd [NM] float32; xform [NM, 12] float64:
        R row-major, then t, x' = R x + t; dev [sum(M L)] float32, indexed like the map: the distance to the fit target's atom after
        the fit, NaN outside the fit set and for members with n_fit < 3; rmsf [sum(L)] float32 and col_count [sum(L)] int32 per axis
        column over the superposed members; offsets [E + 1] of the ensembles' columns; status [E]) on the device, NM = sum(M), the
        members in order. include/tmpnn.h has the contract to the operation and the order of every sum. L <= 8192."""
        if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 3 or tuple(X.shape[1:]) != (4, 3):
            raise TmpnnError("superpose: X must be a float32 [T, 4, 3] tensor on the device (the backbone stays there; there is no CPU path)")
        X = X.contiguous()
        T = int(X.shape[0])
        M, L = np.asarray(members, dtype=np.int64).reshape(-1), np.asarray(lengths, dtype=np.int64).reshape(-1)
        E = int(M.size)
        if L.size != E or (M < 0).any() or (L < 0).any():
            raise TmpnnError(f"superpose: members and lengths must be {E} non-negative numbers each, one per ensemble")
        if E > _lib.ENS_MAX_E:
            raise TmpnnError(f"superpose: {E} ensembles exceed {_lib.ENS_MAX_E} per call")
        max_len = int(L.max()) if E else 0
        if max_len > _lib.ENS_MAX_LEN:
            raise TmpnnError(f"superpose: an ensemble of {max_len} residues exceeds {_lib.ENS_MAX_LEN}, the forward's own bound")
        fit = np.asarray(fit_to, dtype=np.int64).reshape(-1)
        if np.ndim(fit_to) == 0:
            fit = np.repeat(fit, E)
        if fit.size != E or ((M > 0) & ((fit < 0) | (fit >= M))).any():
            raise TmpnnError(f"superpose: fit_to must name a member of every ensemble (0 <= fit_to < M), one number or {E}")
        fit = np.where(M > 0, fit, 0)
        R = int((M * L).sum())
        if T > 0x7fffffff or R > 0x7fffffff:
            raise TmpnnError(f"superpose: {T} backbone rows or {R} map entries exceed 2^31 - 1")
        if rows is not None:
            rows = self._i32(rows).reshape(-1)
            if R != rows.numel():
                raise TmpnnError(f"superpose: the ensembles describe {R} map entries, rows has {rows.numel()}")
        elif R != T:
            raise TmpnnError(f"superpose: the ensembles describe {R} rows, the backbone has {T}")
        mask = self._f32(mask).reshape(-1)
        if mask.numel() != T:
            raise TmpnnError(f"superpose: mask has {mask.numel()} entries for a backbone of {T} rows")
        out_off = np.concatenate([[0], np.cumsum(L)])
        T_out, NM = int(out_off[-1]), int(M.sum())
        map0 = np.concatenate([[0], np.cumsum(M * L)])[:-1]
        mem0 = np.concatenate([[0], np.cumsum(M)])[:-1]
        dev = self.device
        desc = torch.from_numpy(np.stack([map0, M, L, out_off[:-1], mem0, fit], axis=1).astype(np.int32).reshape(E, 6)).to(dev)
        shape = dict(n_fit=(NM,), rmsd=(NM,), xform=(NM, 12), dev=(R,), rmsf=(T_out,), col_count=(T_out,))
        res = {name: torch.empty(shape[name], dtype=getattr(torch, dt), device=dev) for name, dt in _lib.SUP_ARRAYS}
        res["offsets"] = torch.from_numpy(out_off.astype(np.int32)).to(dev)
        res["status"] = torch.zeros(E, dtype=torch.int32, device=dev)
        if E == 0:
            return res
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_superpose(_ptr(X) if T > 0 else None, _ptr(mask) if T > 0 else None,
                                           _ptr(rows) if rows is not None and R > 0 else None, R, _ptr(desc), E, T, NM, T_out, max_len,
                                           *[_ptr(res[name]) if res[name].numel() > 0 else None for name, _ in _lib.SUP_ARRAYS],
                                           _ptr(res["status"]), _stream()), "tmpnn_superpose")
        return res

    # -- global alignment of letter-code sequences ----------------------------------------------------
    def align_global(self, A, B, desc, max_n: Optional[int] = None, max_m: Optional[int] = None, out: Optional[torch.Tensor] = None,
                     slots: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Global alignments of P pairs of letter-code sequences in one launch (tmpnn_align_global: the rule of
        ``datasets.global_alignment_map``, identical columns count 1, gaps are free; codes match iff equal and in [0, 20)).
        ``A``, ``B``: int32 code arrays (all axes, all members, back to back); ``desc`` [P, 6] int32 on the host = (a0, n, b0, m, out0,
        add) per pair: axis ``A[a0 : a0 + n]`` against ``B[b0 : b0 + m]``. -> dict(out int32: ``out[out0 + q] = add + j`` where axis
        position q is aligned to member position j, else -1; aligned [P]: the number of aligned columns; status [P]: 0, or -1 for a
        descriptor the device refused, whose entries are not written) on the device. ``max_n`` / ``max_m``: bounds on every n / m
        (default: the largest in ``desc``), <= 8192. ``out``: a device buffer to write into (default: one of max(out0 + n) entries,
        prefilled with -1). ``slots``: workspace slots (default: what tmpnn_align_workspace_bytes asks for P pairs); results do not
        depend on it."""
        d = np.ascontiguousarray(np.asarray(desc.cpu() if isinstance(desc, torch.Tensor) else desc, dtype=np.int64).reshape(-1, 6))
        P = int(d.shape[0])
        if (np.abs(d) > 0x7fffffff).any():
            raise TmpnnError("align_global: descriptor fields must fit int32")
        if max_n is None:
            max_n = int(d[:, 1].max()) if P else 0
        if max_m is None:
            max_m = int(d[:, 3].max()) if P else 0
        max_n, max_m = max(int(max_n), 0), max(int(max_m), 0)
        if max_n > _lib.ALIGN_MAX_LEN or max_m > _lib.ALIGN_MAX_LEN:
            raise TmpnnError(f"align_global: sequences of {max_n} and {max_m} codes exceed {_lib.ALIGN_MAX_LEN}")
        dev = self.device
        A, B = self._i32(A).reshape(-1), self._i32(B).reshape(-1)
        if out is None:
            good = (d[:, :5] >= 0).all(axis=1)
            n_out = int((d[good, 4] + d[good, 1]).max()) if good.any() else 0
            out = torch.full((n_out,), -1, dtype=torch.int32, device=dev)
        elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.int32 or not out.is_contiguous() or out.dim() != 1:
            raise TmpnnError("align_global: out must be a contiguous int32 [NO] tensor on the device")
        res = dict(out=out, aligned=torch.zeros(P, dtype=torch.int32, device=dev), status=torch.zeros(P, dtype=torch.int32, device=dev))
        if P == 0:
            return res
        need = self.lib.tmpnn_align_workspace_bytes(max_n, max_m, P if slots is None else max(int(slots), 1))
        if need == 0:
            raise TmpnnError(f"align_global: sizes not served (max_n={max_n}, max_m={max_m}, P={P})")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        desc_dev = torch.from_numpy(d.astype(np.int32)).to(dev)
        NA, NB, NO = int(A.numel()), int(B.numel()), int(out.numel())
        with torch.cuda.device(dev):
            check(self.lib.tmpnn_align_global(_ptr(A) if NA else None, NA, _ptr(B) if NB else None, NB, _ptr(desc_dev), P, max_n, max_m,
                                              _ptr(out) if NO else None, NO, _ptr(res["aligned"]), _ptr(res["status"]), _ptr(ws),
                                              ws.numel(), _stream()), "tmpnn_align_global")
        return res

    # -- many sequence variants over one backbone ----------------------------------------------------
    def encode(self, X, mask, residue_idx, chain_enc, offsets, max_len: Optional[int] = None,
               precision: Optional[str] = None) -> "EncodedBackbone":
        """The part of a forward that never reads the sequence — k-NN graph, edge features, three encoder layers — once for a
        packed batch (tmpnn_encode: the launches ``ssm_forward`` makes for that part). -> an EncodedBackbone for
        ``decode_variants``. Raises if a protein is longer than ``max_len`` (one 4-byte read-back)."""
        max_len = self._max_len(offsets, max_len)
        X, mask = self._f32(X), self._f32(mask)
        ridx, cenc, offsets = self._i32(residue_idx), self._i32(chain_enc), self._i32(offsets)
        _need_cuda(X, mask)
        T, N = X.shape[0], offsets.numel() - 1
        used = precision or self.precision
        ctx = torch.empty(max(self.lib.tmpnn_encode_bytes(T), 256), dtype=torch.uint8, device=self.device)
        ws = self._workspace(self.lib.tmpnn_encode_workspace_bytes(T))
        self._status.zero_()
        check(self.lib.tmpnn_encode(self.weights_for(used).handle, _ptr(X), _ptr(mask), _ptr(ridx), _ptr(cenc), _ptr(offsets), N, T,
                                    max_len, self.K, _ptr(ctx), ctx.numel(), _ptr(self._status), _ptr(ws), ws.numel(), _stream()),
              "tmpnn_encode")
        if T > 0 and N > 0:
            self._raise_status("tmpnn_encode")      # a RANGE bit is left to decode_variants, which sees it again and may retry
        return EncodedBackbone(ctx, mask, offsets, T, used, (X, ridx, cenc, max_len))

    def decode_variants(self, enc: "EncodedBackbone", S_variants, want_ddg: bool = True, want_hidden: bool = False,
                        want_log_probs: bool = False, max_rows: Optional[int] = None, check_status: bool = True):
        """Decoder + ddG head for V full sequences over an encoded batch: ``S_variants`` [V,T] (a variant is one sequence over the
        packed residue axis) -> dict(ddg [V,T,21], hidden [V,3,T,128], log_probs [V,T,21]); ddg[v,t,a] is relative to the variant's
        own residue S_variants[v,t]. V is decoded in chunks of at most ``max_rows`` rows (V * T; default 2**18) — a variant's
        result does not depend on the chunking. Status handling as ``ssm_forward``: a non-finite result of an f16x2 decode
        re-encodes the backbone and reruns everything at ``retry_precision`` with a warning, or raises TmpnnRangeError."""
        return self._decode("decode_variants", enc, S_variants, None, want_ddg, want_hidden, want_log_probs, max_rows, check_status)

    def decode_ordered(self, enc: "EncodedBackbone", S_variants, ranks, want_ddg: bool = False, want_hidden: bool = False,
                       want_log_probs: bool = True, max_rows: Optional[int] = None, check_status: bool = True):
        """``decode_variants`` under a decoding order per variant (tmpnn_decode_ordered, ProteinMPNN's masked decoder): ``ranks``
        [V,T] int32, residue i of variant v sees the identity and decoder state of neighbour j when ranks[v,j] < ranks[v,i] and
        only its encoder state otherwise (equal ranks: not visible; all equal: the structure-only distribution). Same dict,
        chunking and range contract as ``decode_variants``."""
        R = self._i32(ranks)
        if R.dim() != 2 or R.shape[1] != enc.T:
            raise TmpnnError(f"decode_ordered: ranks must be [V, {enc.T}], got {tuple(R.shape)}")
        return self._decode("decode_ordered", enc, S_variants, R, want_ddg, want_hidden, want_log_probs, max_rows, check_status)

    def _decode(self, what: str, enc: "EncodedBackbone", S_variants, R: Optional[torch.Tensor], want_ddg: bool, want_hidden: bool,
                want_log_probs: bool, max_rows: Optional[int], check_status: bool):
        """The body of decode_variants (R is None) and decode_ordered (R = ranks [V,T])."""
        if not (want_ddg or want_hidden or want_log_probs):
            raise TmpnnError(f"{what}: no output requested")
        S = self._i32(S_variants)
        T = enc.T
        if S.dim() != 2 or S.shape[1] != T:
            raise TmpnnError(f"{what}: S_variants must be [V, {T}], got {tuple(S.shape)}")
        if R is not None and R.shape != S.shape:
            raise TmpnnError(f"{what}: ranks {tuple(R.shape)} and S_variants {tuple(S.shape)} differ in shape")
        if S.numel() and (int(S.min()) < 0 or int(S.max()) >= VOCAB):
            raise TmpnnError(f"{what}: residue indices must lie in [0, {VOCAB})")
        V, dev = S.shape[0], self.device
        res = {}
        if want_ddg:
            res["ddg"] = torch.empty((V, T, VOCAB), dtype=torch.float32, device=dev)
        if want_hidden:
            res["hidden"] = torch.empty((V, 3, T, HID), dtype=torch.float32, device=dev)
        if want_log_probs:
            res["log_probs"] = torch.empty((V, T, VOCAB), dtype=torch.float32, device=dev)
        if V == 0 or T == 0:
            return res
        per = self._per_chunk(max_rows, T)
        sizer = self.lib.tmpnn_decode_variants_workspace_bytes if R is None else self.lib.tmpnn_decode_ordered_workspace_bytes

        def launch(e: "EncodedBackbone", w: Weights, ws: torch.Tensor, v0: int, v1: int):
            part = lambda k: _ptr(res[k][v0:v1]) if k in res else None
            if R is None:
                check(self.lib.tmpnn_decode_variants(w.handle, _ptr(e.ctx), e.ctx.numel(), _ptr(S[v0:v1]), v1 - v0, _ptr(e.mask), T,
                                                     part("ddg"), part("hidden"), part("log_probs"), _ptr(self._status), _ptr(ws),
                                                     ws.numel(), _stream()), "tmpnn_decode_variants")
            else:
                check(self.lib.tmpnn_decode_ordered(w.handle, _ptr(e.ctx), e.ctx.numel(), _ptr(S[v0:v1]), _ptr(R[v0:v1]), v1 - v0,
                                                    _ptr(e.mask), T, part("ddg"), part("hidden"), part("log_probs"),
                                                    _ptr(self._status), _ptr(ws), ws.numel(), _stream()), "tmpnn_decode_ordered")

        self._chunked(what, enc, V, per, sizer(T, min(per, V)), launch, check_status, stacklevel=3)
        return res

    # -- the chunk loop and range contract of the calls over an encoded backbone (decode_variants, decode_ordered, sample) ---------
    @staticmethod
    def _per_chunk(max_rows: Optional[int], T: int) -> int:
        """Variants / chains per launch: at most ``max_rows`` rows (default 2**18) of T residues, at least one."""
        return max(1, (int(max_rows) if max_rows is not None else 1 << 18) // T)

    def _chunked(self, what: str, enc: "EncodedBackbone", n: int, per: int, need: int, launch, check_status: bool, stacklevel: int):
        """``launch(e, w, ws, i0, i1)`` for every chunk of at most ``per`` of ``n`` items, each with the engine's status word, on
        ``enc`` and a workspace of ``need`` bytes; the OR of the chunks' words (one read-back) goes through ``range_retry``, whose
        rerun encodes the backbone again at the retry precision. ``stacklevel``: as ``warnings.warn`` counts from the caller."""
        self._chunks(what, enc, [(i0, min(n, i0 + per)) for i0 in range(0, n, per)], need, launch, check_status, stacklevel + 1)

    def _chunks(self, what: str, enc: "EncodedBackbone", chunks, need: int, launch, check_status: bool, stacklevel: int):
        """``launch(e, w, ws, *chunk)`` for every chunk (the body of ``_chunked``; the sample entries plan their own chunks)."""
        def run(precision: str) -> int:
            e = enc
            if precision != enc.precision:
                X, ridx, cenc, max_len = enc.inputs
                e = self.encode(X, enc.mask, ridx, cenc, enc.offsets, max_len=max_len, precision=precision)
            w, ws = self.weights_for(precision), self._workspace(need)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            for chunk in chunks:
                launch(e, w, ws, *chunk)
                status.bitwise_or_(self._status)
            return int(status.item()) if check_status else 0

        range_retry(run, enc.precision, self.retry_precision, what, stacklevel + 1)

    # -- autoregressive sampling over one backbone ----------------------------------------------------
    def sample(self, enc: "EncodedBackbone", order, S_fixed, free, u, temperature: float = 1.0, bias=None, allowed=None,
               max_rows: Optional[int] = None, check_status: bool = True):
        """N chains sampled autoregressively over an encoded batch in one launch per chunk (tmpnn_sample): ``order`` [N,T] (a
        permutation of 0..T-1 per chain, order[n,s] is decoded at step s), ``S_fixed`` [N,T] letters kept where ``free`` [N,T] is 0
        or the mask is 0, ``u`` [N,T] uniforms in [0,1) indexed by RESIDUE, ``bias`` / ``allowed`` [T,21] or None ->
        dict(S [N,T] int32, probs [N,T,21]); probs = softmax(logits / temperature + bias) (times allowed, renormalised) on free
        positions and exactly 0 elsewhere, and the letter is the smallest a whose fp32 running sum of probs exceeds u * total.
        N is sampled in chunks of at most ``max_rows`` rows (N * T; default 2**18) — a chain's result does not depend on the chunking.
        Range contract as ``decode_variants``: a non-finite result of an f16x2 context re-encodes the backbone and reruns the whole
        call at ``retry_precision`` with a warning, or raises TmpnnRangeError."""
        return self._sample_front("sample", enc, order, None, S_fixed, free, u, temperature, None, bias, allowed, None, None, None,
                                  max_rows, check_status)

    def sample_tied(self, enc: "EncodedBackbone", order, close, S_fixed, free, u, temperature: float = 1.0, weight=None, bias=None,
                    allowed=None, pssm_mix=None, pssm_bias=None, pssm_keep=None, max_rows: Optional[int] = None,
                    check_status: bool = True):
        """N chains sampled with TIED positions and PSSM terms in one launch per chunk (tmpnn_sample_tied; the reference's
        tied_sample, protein_mpnn_utils.py:1385-1494). ``order`` / ``S_fixed`` / ``free`` / ``u`` / ``bias`` / ``allowed`` as ``sample``;
        ``close`` [N,T] 0 / 1 with close[:, -1] == 1: a group is a maximal run of steps ending at a 1, its members are decoded one
        after the other (a later member sees the earlier ones' states without a letter), their logits are summed with ``weight``
        [N,T] (by residue; None = 1; tied_beta / len(group)) and ONE letter is drawn for the group, with every per-residue table read
        at the closing member; a group that meets a masked member takes S_fixed there and leaves probs rows of 0. ``pssm_mix`` [T]
        with ``pssm_bias`` [T,21]: probs = (1 - mix) probs + mix pssm_bias; ``pssm_keep`` [T,21]: probs = (probs keep + 0.001 probs),
        renormalised; then ``allowed``. -> dict(S int32 [N,T], probs [N,T,21]); probs is written to every member of a live group,
        fixed ones included. Chunking and the range contract as ``sample``."""
        return self._sample_front("sample_tied", enc, order, close, S_fixed, free, u, temperature, weight, bias, allowed, pssm_mix,
                                  pssm_bias, pssm_keep, max_rows, check_status)

    # -- the samplers for every protein of a packed batch over its own steps -------------------------------------------
    def sample_each(self, enc: "EncodedBackbone", order, S_fixed, free, u, temperature: float = 1.0, bias=None, allowed=None,
                    max_rows: Optional[int] = None, check_status: bool = True):
        """``sample`` for MANY backbones at once (tmpnn_sample_each): ``enc`` is a packed batch of P proteins, every argument keeps
        ``sample``'s meaning and full-batch shape, and chain n's schedule for protein b is ``order[n, t0:t1]`` (t0, t1 =
        offsets[b], offsets[b + 1]), a permutation of the packed indices t0..t1-1. A workgroup owns (protein, 16 chains) and walks
        the protein's own steps, so a launch runs P * ceil(N / 16) workgroups over max(L) steps where ``sample`` on the packed
        context runs ceil(N / 16) over T. -> dict(S [N,T] int32, probs [N,T,21]); a (protein, chain) result has the bits
        ``sample`` gives for that protein encoded alone with the segment's order shifted to local indices. A chunk is a protein
        range times a chain range of at most ``max_rows`` rows (chains * residues of the range; default 2**18; one protein and
        one chain at least), long proteins launched first; results do not depend on the chunking. Range contract as ``sample``."""
        return self._sample_front("sample_each", enc, order, None, S_fixed, free, u, temperature, None, bias, allowed, None, None, None,
                                  max_rows, check_status)

    def sample_tied_each(self, enc: "EncodedBackbone", order, close, S_fixed, free, u, temperature: float = 1.0, weight=None, bias=None,
                         allowed=None, pssm_mix=None, pssm_bias=None, pssm_keep=None, max_rows: Optional[int] = None,
                         check_status: bool = True):
        """``sample_tied`` for every protein of a packed batch over its own steps (tmpnn_sample_tied_each): arguments as
        ``sample_tied``, schedule, chunking and bits as ``sample_each``. Groups live inside one protein: every protein's last step
        must close (close[n, offsets[b + 1] - 1] == 1)."""
        return self._sample_front("sample_tied_each", enc, order, close, S_fixed, free, u, temperature, weight, bias, allowed, pssm_mix,
                                  pssm_bias, pssm_keep, max_rows, check_status)

    def _sample_front(self, what: str, enc: "EncodedBackbone", order, close, S_fixed, free, u, temperature, weight, bias, allowed,
                      pssm_mix, pssm_bias, pssm_keep, max_rows: Optional[int], check_status: bool):
        """The body of the four sample entries (``what`` names one): ``sample_args`` and ``sample_verdicts`` refuse before any launch,
        then the chunk plan, the workspace and one launch per chunk of the entry's own C function."""
        tied, each = "tied" in what, what.endswith("_each")
        T, P = enc.T, enc.offsets.numel() - 1
        rows, tabs, res = sample_args(what, T, self.device, order, close, S_fixed, free, u, temperature, weight, bias, allowed, pssm_mix,
                                      pssm_bias, pssm_keep)
        N = rows["order"].shape[0]
        if N == 0 or T == 0 or (each and P <= 0):
            return res
        _need_cuda(enc.ctx)
        # one device pass, ONE read-back: the verdicts and the offsets the chunk plan needs on the host
        offs = sample_verdicts(what, rows["order"], rows["S_fixed"], rows["close"], enc.offsets if each else None)
        chunks = plan_each_chunks(offs, N, max_rows) if each else plan_axis_chunks(T, N, max_rows)
        entry, sizer = {"sample": (self.lib.tmpnn_sample, self.lib.tmpnn_sample_workspace_bytes),
                        "sample_tied": (self.lib.tmpnn_sample_tied, self.lib.tmpnn_sample_tied_workspace_bytes),
                        "sample_each": (self.lib.tmpnn_sample_each, self.lib.tmpnn_sample_each_workspace_bytes),
                        "sample_tied_each": (self.lib.tmpnn_sample_tied_each, self.lib.tmpnn_sample_tied_each_workspace_bytes)}[what]
        need = 0
        for p0, p1, n0, n1 in chunks:
            b = sizer(offs[p1] - offs[p0], n1 - n0)
            if b == 0:
                raise TmpnnError(f"{what}: {n1 - n0} chain(s) of the {offs[p1] - offs[p0]} residues of proteins [{p0}, {p1}) exceed one "
                                 f"launch's table" if each else
                                 f"{what}: {n1 - n0} chains of {T} residues exceed one launch's table; lower max_rows")
            need = max(need, b)
        at = {}
        if each:    # the launch order of every chunk's proteins, longest first: one upload
            sched = torch.as_tensor(np.concatenate([each_schedule(offs, p0, p1) for p0, p1, _, _ in chunks]), dtype=torch.int32).to(self.device)
            pos = 0
            for p0, p1, n0, n1 in chunks:
                at[(p0, p1, n0, n1)] = pos
                pos += p1 - p0

        def launch(e: "EncodedBackbone", w: Weights, ws: torch.Tensor, p0: int, p1: int, n0: int, n1: int):
            part = {k: _ptr(None if t is None else t[n0:n1]) for k, t in rows.items()}
            args = [w.handle, _ptr(e.ctx), e.ctx.numel(), _ptr(e.mask), T]
            if each:
                s = at[(p0, p1, n0, n1)]
                args += [_ptr(e.offsets), P, p0, p1, offs[p0], offs[p1] - offs[p0], _ptr(sched[s:s + p1 - p0])]
            args += [n1 - n0, part["order"]] + ([part["close"]] if tied else [])
            args += [part["S_fixed"], part["free"], part["u"], 1.0 / float(temperature)] + ([part["weight"]] if tied else [])
            args += [_ptr(tabs[k]) for k in (SAMPLE_TABLES if tied else SAMPLE_TABLES[:2])]
            check(entry(*args, _ptr(res["S"][n0:n1]), _ptr(res["probs"][n0:n1]), _ptr(self._status), _ptr(ws), ws.numel(), _stream()),
                  f"tmpnn_{what}")

        self._chunks(what, enc, chunks, need, launch, check_status, stacklevel=3)       # a retry warning names the public entry's caller
        return res

    def capture_graph(self, X, S, mask, residue_idx, chain_enc, offsets, max_len: int, out: Optional[dict] = None, **want):
        """Capture ONE fused forward (its ~20 launches + the status memset) into a hipGraph: -> (graph, out). ``graph.replay()``
        reruns it on the captured tensors — refill X / S / ... in place for a new protein of the same length. The C-ABI
        never allocates or synchronises, so the call sequence captures as is. Removes the per-launch CPU cost that
        dominates a single small protein (20 launches for ~0.2 ms of GPU work).

        Every buffer whose address is baked into the captured launches belongs to the GRAPH, not to the engine: the
        workspace and the status word are allocated here (the engine's shared workspace is reallocated when a later call
        needs more bytes — a graph that pointed into it would replay on freed memory), and the graph keeps them, the
        inputs, the outputs and the weight handle alive. ``check_graph_status(graph)`` reads the graph's status word."""
        X, mask = self._f32(X), self._f32(mask)
        S, ridx, cenc, offsets = self._i32(S), self._i32(residue_idx), self._i32(chain_enc), self._i32(offsets)
        priv: dict = {}
        kw = dict(max_len=int(max_len), check_status=False, _private=priv, **want)
        w = self.weights_for(want.get("precision") or self.precision)
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            out = self.ssm_forward(X, S, mask, ridx, cenc, offsets, out=out, **kw)        # warm-up: buffers exist afterwards
        keep = [X, S, mask, ridx, cenc, offsets, priv["ws"], priv["status"], *out.values()]
        for t in keep:                      # allocated / first used on the side stream, replayed from others later
            t.record_stream(cur)
        cur.wait_stream(side)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.ssm_forward(X, S, mask, ridx, cenc, offsets, out=out, **kw)
        graph._tmpnn_keepalive = (keep, out, priv, w)                                      # captured pointers stay valid
        graph._tmpnn_status = priv["status"]
        return graph, out

    def check_graph_status(self, graph) -> None:
        """Raise if the last replay of a graph from ``capture_graph`` flagged a range / max_len problem (syncs)."""
        st = int(graph._tmpnn_status.item())
        if st:
            check(self.lib.tmpnn_status_error(st), "tmpnn_ssm_forward[graph]")

    def check_last_status(self) -> None:
        """Raise if the most recent ``ssm_forward(check_status=False)`` flagged a range / max_len problem (syncs)."""
        st = int(self._status.item())
        if st:
            check(self.lib.tmpnn_status_error(st), "tmpnn_ssm_forward")


# module-level gathers with the reference's signatures (protein_mpnn_utils.py:763-791)
# -- host side of the four sample entries: the checks, the chunk plans and the launch order (plain torch / numpy: they run without a GPU) --
EACH_ROWS_MAX = ((1 << 24) - 1) // 3          # chains * rows of one launch (3 * N * rows < 2**24, the chain kernel's row arithmetic)
SAMPLE_TABLES = ("bias", "allowed", "pssm_mix", "pssm_bias", "pssm_keep")     # per residue: [T,21], pssm_mix [T]


def check_row_runs(row, R: int) -> None:
    """tmpnn_pair_map's promise, checked on the host: within one call the variants of one state row are contiguous (rows outside
    [0, R) name no state row and may repeat). TmpnnError with the row and the variant at which it comes back."""
    r = np.asarray(row).reshape(-1).astype(np.int64)
    heads = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]])) if r.size else np.zeros(0, np.int64)
    heads = heads[(r[heads] >= 0) & (r[heads] < int(R))]
    seen = {}
    for v in heads.tolist():
        if int(r[v]) in seen:
            raise TmpnnError(f"pair_map: the variants of one row must be contiguous within a call: row {int(r[v])} begins at variant "
                             f"{seen[int(r[v])]} and comes back at variant {v}")
        seen[int(r[v])] = v


def decode_pair_map(state) -> Dict[str, object]:
    """The state of ``Engine.pair_map`` read: integer operations of torch where the state lives (nothing is copied), or of numpy on
    numpy arrays. -> dict(best_ddG, eps_min, eps_max: float32 [R, L], NaN where there is none — the value's own bits, a -0.0 as +0.0;
    best_a / best_b, eps_min_a / eps_min_b, eps_max_a / eps_max_b: int32, the letter of the variant and the substituted letter, -1
    where there is none; eps_abs_mean = eps_abs_sum / count in float32, NaN at count 0; count)."""
    on_torch = isinstance(state["best"], torch.Tensor)
    xp = torch if on_torch else np
    out = {}

    def read(keys, inverted):
        k = keys if on_torch else np.asarray(keys).view(np.int64)
        none = k == -1
        o = (k >> 32) & 0xffffffff
        if inverted:
            o = o ^ 0xffffffff
        bits = xp.where((o >> 31) == 1, o ^ 0x80000000, o ^ 0xffffffff)        # hits_ord undone
        bits = xp.where(none, xp.full_like(bits, 0x7fc00000), bits)
        if on_torch:
            val = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)
            return val, xp.where(none, -1, (k >> 5) & 31).to(torch.int32), xp.where(none, -1, k & 31).to(torch.int32)
        val = bits.astype(np.uint32).view(np.float32)
        return val, np.where(none, -1, (k >> 5) & 31).astype(np.int32), np.where(none, -1, k & 31).astype(np.int32)

    for name, key, inverted in (("best", "best", False), ("eps_min", "eps_lo", False), ("eps_max", "eps_hi", True)):
        val, a, b = read(state[key], inverted)
        out["best_ddG" if name == "best" else name], out[name + "_a"], out[name + "_b"] = val, a, b
    total, count = state["eps_abs_sum"], state["count"]
    if on_torch:
        mean = total / count.clamp(min=1).to(torch.float32)
        out["eps_abs_mean"] = torch.where(count == 0, torch.full_like(mean, float("nan")), mean)
    else:
        total, count = np.asarray(total, dtype=np.float32), np.asarray(count)
        mean = total / np.maximum(count, 1).astype(np.float32)
        out["eps_abs_mean"] = np.where(count == 0, np.float32("nan"), mean).astype(np.float32)
    out["count"] = count
    return out


def sample_args(what: str, T: int, dev, order, close, S_fixed, free, u, temperature, weight, bias, allowed, pssm_mix, pssm_bias, pssm_keep):
    """The arguments of the sample entry ``what`` on ``dev``, refused with the entry's name where their shapes or values cannot be
    launched -> (rows, tabs, res): the per-chain arrays [N,T] (order / close / S_fixed int32, free / u / weight float32; close only for
    the tied entries, weight may be None), the per-residue tables (SAMPLE_TABLES, float32 or None) and the allocated dict(S, probs)."""
    i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous()
    f32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
    rows = {"order": i32(order), "close": i32(close) if "tied" in what else None, "S_fixed": i32(S_fixed), "free": f32(free), "u": f32(u),
            "weight": None if weight is None else f32(weight)}
    N = rows["order"].shape[0]
    for name, t in rows.items():
        if t is not None and (t.dim() != 2 or t.shape[1] != T or t.shape[0] != N):
            raise TmpnnError(f"{what}: {name} must be [N, {T}] like order, got {tuple(t.shape)}")
    if not float(temperature) > 0.0 or not np.isfinite(float(temperature)):
        raise TmpnnError(f"{what}: temperature must be positive and finite, got {temperature!r}")
    if (pssm_mix is None) != (pssm_bias is None):
        raise TmpnnError(f"{what}: pssm_bias goes with pssm_mix (give both or neither)")
    tabs = {}
    for name, t in zip(SAMPLE_TABLES, (bias, allowed, pssm_mix, pssm_bias, pssm_keep)):
        shape = (T,) if name == "pssm_mix" else (T, VOCAB)
        tabs[name] = None if t is None else f32(t)
        if t is not None and tuple(tabs[name].shape) != shape:
            raise TmpnnError(f"{what}: {name} must be {list(shape)}, got {tuple(tabs[name].shape)}")
    res = {"S": torch.empty((N, T), dtype=torch.int32, device=dev), "probs": torch.empty((N, T, VOCAB), dtype=torch.float32, device=dev)}
    return rows, tabs, res


def sample_verdicts(what: str, order: torch.Tensor, S_fixed: torch.Tensor, close: Optional[torch.Tensor],
                    offsets: Optional[torch.Tensor]) -> List[int]:
    """``each_verdicts`` for the sample entry ``what``, read back ONCE together with the offsets and refused with the entry's name ->
    the offsets on the host. ``offsets`` None: the whole axis is one segment [0, T) (sample / sample_tied, whatever the context packs)."""
    T = order.shape[1]
    verdicts = each_verdicts(order, S_fixed, close, offsets)
    if offsets is None:
        ok, offs = verdicts.tolist(), [0, T]
    else:
        back = torch.cat([verdicts.to(torch.int64), offsets.to(device=verdicts.device, dtype=torch.int64)]).tolist()
        ok, offs = back[: verdicts.numel()], back[verdicts.numel():]
    if offs[0] != 0 or offs[-1] != T or any(b < a for a, b in zip(offs, offs[1:])):
        raise TmpnnError(f"{what}: offsets must rise from 0 to T = {T}")
    if not ok[0]:
        raise TmpnnError(f"{what}: every row of order must be a permutation of 0..{T - 1}")
    if not ok[1]:
        raise TmpnnError(f"{what}: every entry of order must stay inside the protein of its position (order[n, t0:t1] is a "
                         f"permutation of t0..t1-1)")
    if not ok[2]:
        raise TmpnnError(f"{what}: residue indices must lie in [0, {VOCAB})")
    if close is not None and not ok[3]:
        raise TmpnnError(f"{what}: close must hold 0 or 1")
    if close is not None and not ok[4]:
        raise TmpnnError(f"{what}: every protein's last step must close (close[n, offsets[b + 1] - 1] == 1): a group lives inside "
                         f"one protein" if what.endswith("_each") else
                         f"{what}: close[:, -1] must be 1 (the last step ends its group)")
    return offs


def plan_axis_chunks(T: int, N: int, max_rows: Optional[int] = None) -> List[tuple]:
    """The chunks of sample / sample_tied in ``plan_each_chunks``'s form: the one segment (0, 1) times chain ranges of at most
    ``max_rows`` rows (default 2**18), one chain at least, rising over [0, N)."""
    per = Engine._per_chunk(max_rows, T)
    return [(0, 1, n0, min(N, n0 + per)) for n0 in range(0, N, per)]


def each_verdicts(order: torch.Tensor, S_fixed: torch.Tensor, close: Optional[torch.Tensor], offsets: Optional[torch.Tensor]) -> torch.Tensor:
    """The checks of the sample entries in one pass on the arrays' device -> bool [3] (or [5] with ``close``): every row of ``order``
    [N,T] a permutation of 0..T-1; every entry inside the protein of its position (seg[order] == seg[position] — with the first,
    order[n, t0:t1] is a permutation of t0..t1-1); letters in [0, 21); close 0 / 1; every non-empty protein's last step closing (so
    no group spans two proteins). ``offsets`` None: the axis is one segment [0, T) — nothing lies outside it, its last step is T - 1."""
    N, T = order.shape
    dev = order.device
    steps = torch.arange(T, dtype=torch.int64, device=dev)
    perm = (torch.sort(order, dim=1).values == steps).all()
    if offsets is None:
        inside = torch.ones_like(perm)
    else:
        offsets = offsets.to(device=dev, dtype=torch.int64)
        seg = torch.bucketize(steps, offsets[1:].contiguous(), right=True)                      # position -> protein
        inside = (seg[order.to(torch.int64).clamp(0, max(T - 1, 0))] == seg).all()
    out = [perm, inside, ((S_fixed >= 0) & (S_fixed < VOCAB)).all()]
    if close is not None:
        last = slice(-1, None) if offsets is None else \
            (offsets[1:] - 1)[offsets[1:] > offsets[:-1]].clamp(0, max(T - 1, 0))               # the last position of every non-empty protein
        out += [((close == 0) | (close == 1)).all(), (close[:, last] == 1).all()]
    return torch.stack(out)


def plan_each_chunks(offsets: Sequence[int], N: int, max_rows: Optional[int] = None) -> List[tuple]:
    """Chunks (p0, p1, n0, n1) — a protein range times a chain range — that cover every (protein, chain) pair exactly once, with
    (n1 - n0) * rows <= min(max_rows, EACH_ROWS_MAX) for rows = offsets[p1] - offsets[p0] wherever one protein and one chain fit that;
    a protein longer than the bound still gets chunks of one chain. Greedy: as many proteins as hold all N chains, else one protein
    and as many chains as fit."""
    cap = min(int(max_rows) if max_rows is not None else 1 << 18, EACH_ROWS_MAX)
    P, chunks, p0 = len(offsets) - 1, [], 0
    while p0 < P and N > 0:
        p1 = p0 + 1
        while p1 < P and (offsets[p1 + 1] - offsets[p0]) * N <= cap:
            p1 += 1
        rows = offsets[p1] - offsets[p0]
        per = N if rows * N <= cap else max(1, cap // max(rows, 1))
        chunks += [(p0, p1, n0, min(N, n0 + per)) for n0 in range(0, N, per)]
        p0 = p1
    return chunks


def each_schedule(offsets: Sequence[int], p0: int, p1: int) -> np.ndarray:
    """The launch order of proteins [p0, p1): indices by descending length (ties in index order), so the long ones start first."""
    o = np.asarray(offsets[p0:p1 + 1], dtype=np.int64)
    return (p0 + np.argsort(-(o[1:] - o[:-1]), kind="stable")).astype(np.int32)


def gather_nodes(nodes: torch.Tensor, neighbor_idx: torch.Tensor) -> torch.Tensor:
    _need_cuda(nodes, neighbor_idx)
    lib = _lib.load()
    B, N, C_ = nodes.shape
    K = neighbor_idx.shape[2]
    src = nodes.to(torch.float32).contiguous()
    idx = neighbor_idx.to(torch.int64).contiguous()
    out = torch.empty((B, idx.shape[1], K, C_), dtype=torch.float32, device=nodes.device)
    with torch.cuda.device(nodes.device):
        check(lib.tmpnn_gather_nodes(_ptr(src), _ptr(idx), B, N, K, C_, _ptr(out), _stream()), "tmpnn_gather_nodes")
    return out.to(nodes.dtype)


def gather_edges(edges: torch.Tensor, neighbor_idx: torch.Tensor) -> torch.Tensor:
    _need_cuda(edges, neighbor_idx)
    lib = _lib.load()
    B, N, _, C_ = edges.shape
    K = neighbor_idx.shape[2]
    src = edges.to(torch.float32).contiguous()
    idx = neighbor_idx.to(torch.int64).contiguous()
    out = torch.empty((B, N, K, C_), dtype=torch.float32, device=edges.device)
    with torch.cuda.device(edges.device):
        check(lib.tmpnn_gather_edges(_ptr(src), _ptr(idx), B, N, K, C_, _ptr(out), _stream()), "tmpnn_gather_edges")
    return out.to(edges.dtype)


def cat_neighbors_nodes(h_nodes, h_neighbors, E_idx):
    return torch.cat([h_neighbors, gather_nodes(h_nodes, E_idx)], -1)
