"""The guarded-window tests (tests/test_gpu_workspace.py: ``guarded``, three prefills, exact sizes, tail guards) of the entries behind
the fused forward: the layer entries, a C-alpha handle, the weight constructors' ``packed`` buffer, the tied and per-protein samplers,
head training, fine-tuning (fused and split), the sequence loss (one protein and packed), the selection entries, the alignment and the
bootstrap. Every comparison is on bits. Per entry a comment says whether it aligns the base itself (three window offsets) or takes it
as it is (offset 0), and whether it refuses one byte less than its size or takes whatever its carve fits.

Training inputs: the weights are seeded normal draws of 0.1 standard deviation in the entry's slab layout. They are not a trained
model; the values only have to be finite and to depend on every buffer the entry carves."""
import ctypes as C

import numpy as np
import pytest
import torch

from align_inputs import pack as align_pack, small_batch
from beam_each_restatement import pack_fixture
from beam_restatement import duplicate_fixture
from bootstrap_restatement import dense_rank, fixture_rows, fixture_values
from hits_inputs import bits_table, letters, offsets_of
from test_gpu_beam_each import MIXED
from test_gpu_sample import chains
from test_gpu_tied_sample import groups_of_four, tied_chains
from test_gpu_workspace import (AS_IS, BATCHES, DEV, Buf, context, encode_case, engine, forward_case, guarded, in_window, lib, packed,
                                ptr, same_bits, sampler_outputs, stale, stream)
from variant_inputs import hits_case, pmap_case

pytestmark = pytest.mark.gpu

INF = float("inf")
_CA = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def i32(*shape):
    return torch.empty(shape, dtype=torch.int32, device=DEV)


def f32(*shape):
    return torch.empty(shape, dtype=torch.float32, device=DEV)


def normal(n, seed, scale=0.1):
    return dev((np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32))


# ---- layers: Carver(ws, true), the entry aligns the base (three offsets) and takes what its carve fits --------------------------
def layer_inputs(batch):
    eng, p = engine("f16x2"), packed(batch)
    E_idx, D_nb = eng.knn_topk(p["X"], p["mask"], p["offsets"].cpu())
    h_E = eng.edge_featurize(p["X"], p["ridx"], p["cenc"], E_idx, D_nb)
    return eng, p, E_idx, h_E, normal(p["T"] * 128, 21).view(p["T"], 128)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_enc_layer(batch):
    """h_V and h_E are updated in place: both are set back before every call, and both must have changed."""
    eng, p, E_idx, h_E0, h_V0 = layer_inputs(batch)
    T = p["T"]
    o = dict(h_V=f32(T, 128), h_E=f32(T, 48, 128))

    def prepare(w):
        o["h_V"].copy_(h_V0)
        o["h_E"].copy_(h_E0)

    def call(w):
        return eng.lib.tmpnn_enc_layer(eng.w.handle, 1, ptr(o["h_V"]), ptr(o["h_E"]), ptr(E_idx), ptr(p["mask"]), T, w["ws"].ptr, w["ws"].nbytes,
                                       stream())

    def extra(w):
        assert not same_bits(o["h_V"], h_V0) and not same_bits(o["h_E"], h_E0)
        return {}

    guarded(call, dict(ws=Buf(eng.lib.tmpnn_layer_workspace_bytes(T))), o, prepare=prepare, extra=extra)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_dec_layer(batch):
    eng, p, E_idx, h_E, h_V = layer_inputs(batch)
    T = p["T"]
    o = dict(h_V_out=f32(T, 128))

    def call(ws, nbytes):
        return eng.lib.tmpnn_dec_layer(eng.w.handle, 1, ptr(h_V), ptr(o["h_V_out"]), ptr(h_E), ptr(E_idx), ptr(p["S"]), ptr(p["mask"]), T, ws,
                                       nbytes, stream())

    in_window(call, eng.lib.tmpnn_layer_workspace_bytes(T), o)


# ---- a C-alpha handle: the frames of ca_frames live inside the layer part's P2 ------------------------------------------------------
def ca_engine():
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if "eng" not in _CA:
        _CA["eng"] = Engine(synthetic_state_dict(0, "mpnn_ca"), DEV, 48, precision="f16x2", retry_precision=None)
        assert _CA["eng"].ca_only
    return _CA["eng"]


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ca_forward(batch):
    forward_case(ca_engine(), batch, ddg=False)              # (a CA handle has no ddG head)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ca_encode(batch):
    encode_case(ca_engine(), batch)


# ---- weight images: `packed` is taken as it is (16-byte aligned: offset 0), one byte less is refused ----------------------------------
@pytest.mark.parametrize("entry,precision", [("create", None), ("create_p", "f16x2"), ("create_p", "bf16x3"), ("create_p", "fp32"),
                                             ("create_ca", "f16x2")])
def test_weight_images(entry, precision):
    """The handle is built in exactly *_packed_bytes_p bytes; the guards hold after the constructor's launches and after one fused
    forward through the handle, whose outputs are those of a handle on a roomy buffer. The handle is destroyed before its buffer."""
    L = lib()
    src = ca_engine() if entry == "create_ca" else engine(precision or "f16x2")
    tensors, p = src.w.tensors, packed("L17")
    n, T, enc = len(tensors), p["T"], None if precision is None else precision.encode()
    arr = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    need = (L.tmpnn_weights_ca_packed_bytes_p if entry == "create_ca" else L.tmpnn_weights_packed_bytes_p)(enc)
    ws = torch.zeros(L.tmpnn_workspace_bytes(T) + 4096, dtype=torch.uint8, device=DEV)
    o = dict(hidden=f32(3, T, 128), log_probs=f32(T, 21), status=i32(1))
    if entry != "create_ca":
        o["ddg"] = f32(T, 21)

    def call(w):
        handle = C.c_void_p()
        args = (C.byref(handle), arr, n, w["packed"].ptr, w["packed"].nbytes)
        if entry == "create":
            rc = L.tmpnn_weights_create(*args, stream())
        else:
            rc = (L.tmpnn_weights_create_ca if entry == "create_ca" else L.tmpnn_weights_create_p)(*args, enc, stream())
        if rc != 0:
            assert not handle.value
            return rc
        try:
            torch.cuda.synchronize()
            assert w["packed"].guards_intact()
            rc = L.tmpnn_ssm_forward(handle, ptr(p["X"]), ptr(p["S"]), ptr(p["mask"]), ptr(p["ridx"]), ptr(p["cenc"]), ptr(p["offsets"]), p["N"],
                                     T, p["max_len"], 48, ptr(o.get("ddg")), ptr(o["hidden"]), ptr(o["log_probs"]), None, ptr(o["status"]),
                                     ptr(ws), ws.numel(), stream())
            torch.cuda.synchronize()
        finally:
            L.tmpnn_weights_destroy(handle)
        return rc

    guarded(call, dict(packed=Buf(need, AS_IS, short_by=1)), o)


# ---- samplers: Carver(ws, true) behind a comparison with the sizer: three offsets, one byte less is refused -------------------------
def tied_inputs(c):
    return dict(order=dev(c["order"], torch.int32), close=dev(c["close"], torch.int32), S_fixed=dev(c["S_fixed"], torch.int32),
                free=dev(c["free"], torch.float32), u=dev(c["u"], torch.float32), weight=dev(c["weight"], torch.float32))


@pytest.mark.parametrize("precision,pssm", [("f16x2", True), ("bf16x3", False)])
def test_sample_tied(precision, pssm):
    """N = 17 chains over L17 + L40; groups of four, mirror pairs and untied chains, so groups tie positions of both proteins."""
    eng, p, ctx = engine(precision), packed("L17+L40"), context(precision, "L17+L40")
    T, N = p["T"], 17
    pairs = [[i, T - 1 - i] for i in range(0, T // 2, 3)]
    betas = np.random.default_rng(9).uniform(0.5, 1.5, T).astype(np.float32)
    c = tied_inputs(tied_chains(T, N, 31, [groups_of_four(T), pairs, []], fixed_every=6, betas=betas))
    rng = np.random.default_rng(12)
    pb = rng.random((T, 21)).astype(np.float32)
    tabs = [dev((rng.random(T) * 0.4).astype(np.float32)), dev(pb / pb.sum(-1, keepdims=True)),
            dev((rng.random((T, 21)) > 0.3).astype(np.float32))] if pssm else [None] * 3
    o = sampler_outputs(T, N)

    def call(ws, nbytes):
        return eng.lib.tmpnn_sample_tied(eng.w.handle, ptr(ctx), ctx.numel(), ptr(p["mask"]), T, N, ptr(c["order"]), ptr(c["close"]),
                                         ptr(c["S_fixed"]), ptr(c["free"]), ptr(c["u"]), 1.0, ptr(c["weight"]), None, None, *[ptr(t) for t in tabs],
                                         ptr(o["S"]), ptr(o["probs"]), ptr(o["status"]), ws, nbytes, stream())

    in_window(call, eng.lib.tmpnn_sample_tied_workspace_bytes(T, N), o, short_by=1)


RANGES = {"middle": (1, 2), "last": (2, 3)}             # of L17 + L40 + L17: rows [17, 57) and [57, 74)


def each_inputs(tied, N=17):
    """Per protein a schedule over its own rows, shifted to packed indices."""
    p = packed("L17+L40+L17")
    starts, parts = p["starts"], []
    for b in range(3):
        Lb = int(starts[b + 1] - starts[b])
        c = tied_chains(Lb, N, 60 + b, [groups_of_four(Lb), [[i, Lb - 1 - i] for i in range(0, Lb // 2, 3)], []], fixed_every=6) if tied \
            else dict(chains(Lb, N, 50 + b, fixed_every=5), close=np.ones((N, Lb), np.int32), weight=np.ones((N, Lb), np.float32))
        parts.append(dict(c, order=c["order"] + int(starts[b])))
    return p, tied_inputs({k: np.concatenate([c[k] for c in parts], axis=1) for k in parts[0]})


def each_case(precision, which, tied):
    """The scratch is sized by the range's rows and indexed with t - row0: a range that does not start at row 0. S_out and probs are
    written for the rows of the range only (``partial``): the others keep the sentinel in every run."""
    eng, ctx = engine(precision), context(precision, "L17+L40+L17")
    p, c = each_inputs(tied)
    T, N, (p0, p1) = p["T"], 17, RANGES[which]
    row0, rows = int(p["starts"][p0]), int(p["starts"][p1] - p["starts"][p0])
    assert (row0, rows) == {"middle": (17, 40), "last": (57, 17)}[which]
    o = sampler_outputs(T, N)
    head = (eng.w.handle, ptr(ctx), ctx.numel(), ptr(p["mask"]), T, ptr(p["offsets"]), 3, p0, p1, row0, rows, None, N, ptr(c["order"]))
    mid = (ptr(c["S_fixed"]), ptr(c["free"]), ptr(c["u"]), 1.0)

    def call(ws, nbytes):
        tail = (ptr(o["S"]), ptr(o["probs"]), ptr(o["status"]), ws, nbytes, stream())
        if tied:
            return eng.lib.tmpnn_sample_tied_each(*head, ptr(c["close"]), *mid, ptr(c["weight"]), None, None, None, None, None, *tail)
        return eng.lib.tmpnn_sample_each(*head, *mid, None, None, *tail)

    def extra(w):
        inside = torch.zeros(T, dtype=torch.bool, device=DEV)
        inside[row0:row0 + rows] = True
        assert not bool(stale(o["S"][:, inside].contiguous()).any()) and bool(stale(o["S"][:, ~inside].contiguous()).all())
        assert not bool(stale(o["probs"][:, inside].contiguous()).any()) and bool(stale(o["probs"][:, ~inside].contiguous()).all())
        return {}

    sizer = eng.lib.tmpnn_sample_tied_each_workspace_bytes if tied else eng.lib.tmpnn_sample_each_workspace_bytes
    in_window(call, sizer(rows, N), o, short_by=1, partial=("S", "probs"), extra=extra)


@pytest.mark.parametrize("which", list(RANGES))
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample_each(precision, which):
    each_case(precision, which, tied=False)


@pytest.mark.parametrize("which", list(RANGES))
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample_tied_each(precision, which):
    each_case(precision, which, tied=True)


# ---- head training: Carver(base, false), the base as it is (offset 0); one byte less than the size is refused -----------------------
HEADS = {"released": dict(n_final=2, lightattn=1, dims=(384, 64, 32, 21)), "bare": dict(n_final=0, lightattn=0, dims=(128, 21))}


def head_args(head):
    h = HEADS[head]
    return h["n_final"], h["lightattn"], len(h["dims"]) - 1, (C.c_int32 * len(h["dims"]))(*h["dims"])


def mutants(M, n_rows, seed):
    rng = np.random.default_rng(seed)
    return dict(rows=dev(rng.integers(0, n_rows, M), torch.int32), mut=dev(rng.integers(0, 20, M), torch.int32),
                wt=dev(rng.integers(0, 20, M), torch.int32), target=dev(rng.standard_normal(M).astype(np.float32)))


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("head", list(HEADS))
def test_head_train_step(head, M):
    """Dropout from the generator with its mask requested (LightAttention only: the bare head has no dropout site)."""
    L = lib()
    h, D0, n_feat = head_args(head), HEADS[head]["dims"][0], M + 3
    numel = L.tmpnn_head_slab_numel(*h)
    m, feat, params = mutants(M, n_feat, 3), normal(n_feat * D0, 4, 1.0).view(n_feat, D0), normal(numel, 5)
    la = HEADS[head]["lightattn"]
    o = dict(grads=f32(numel), loss=f32(1), pred=f32(M))
    if la:
        o["keep_out"] = f32(M, D0)

    def call(ws, nbytes):
        return L.tmpnn_head_train_step(ptr(feat), n_feat, ptr(m["rows"]), ptr(m["mut"]), ptr(m["wt"]), ptr(m["target"]), M, *h, 1, ptr(params),
                                       ptr(o["grads"]), numel, 0.25 if la else 0.0, None, ptr(o.get("keep_out")), 7, 3, ptr(o["loss"]),
                                       ptr(o["pred"]), ws, nbytes, stream())

    in_window(call, L.tmpnn_head_train_workspace_bytes(M, *h), o, offsets=AS_IS, short_by=1, grads=("grads",))


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("head", list(HEADS))
def test_head_eval(head, M):
    L = lib()
    h, D0, n_feat = head_args(head), HEADS[head]["dims"][0], M + 3
    numel = L.tmpnn_head_slab_numel(*h)
    m, feat, params = mutants(M, n_feat, 3), normal(n_feat * D0, 4, 1.0).view(n_feat, D0), normal(numel, 5)
    o = dict(pred=f32(M))

    def call(ws, nbytes):
        return L.tmpnn_head_eval(ptr(feat), n_feat, ptr(m["rows"]), ptr(m["mut"]), ptr(m["wt"]), M, *h, 1, ptr(params), numel, ptr(o["pred"]), ws,
                                 nbytes, stream())

    in_window(call, L.tmpnn_head_train_workspace_bytes(M, *h), o, offsets=AS_IS, short_by=1)


# ---- fine-tuning: ft_carve2's Carver(saved, false) and Carver(scratch, false): every buffer at offset 0, one byte less is refused --------
FT_CASES = [("L17", 1), ("L40", 65)]


class Finetune:
    """One protein, M mutants and a head: the arguments of the tmpnn_finetune_* entries up to the dropout settings."""

    def __init__(self, batch, M, head):
        L = lib()
        self.p, self.M, self.h, self.la, self.nf = packed(batch), M, head_args(head), HEADS[head]["lightattn"], HEADS[head]["n_final"]
        self.L, self.D0 = self.p["T"], HEADS[head]["dims"][0]
        self.K = min(48, self.L)
        self.numel = L.tmpnn_finetune_slab_numel(*self.h)
        self.params = normal(self.numel, 6)
        self.m = mutants(M, self.L, 8)
        self.model = tuple(ptr(self.p[k]) for k in ("X", "S", "mask", "ridx", "cenc")) + (self.L, ptr(self.m["rows"]), ptr(self.m["mut"]),
                                                                                         ptr(self.m["wt"]))
        self.p_head = 0.25 if self.la else 0.0
        self.sizes = (self.L, M, *self.h)

    def forward_outs(self):
        """pred and, where ProteinMPNN runs (num_final_layers > 0), the masks the generator drew, the graph; the head rows."""
        o = dict(pred=f32(self.M), rows=f32(self.M, self.D0))
        if self.nf:
            o.update(keep_out=f32(lib().tmpnn_finetune_mask_numel(self.L)), E_idx=i32(self.L, self.K))
        return o

    def forward(self, o, saved, nbytes):
        return lib().tmpnn_finetune_forward(*self.model, self.M, *self.h, 1, ptr(self.params), self.numel, 0.1, self.p_head, None,
                                            ptr(o.get("keep_out")), None, 7, 3, ptr(o["pred"]), ptr(o.get("E_idx")), ptr(o["rows"]), saved, nbytes,
                                            stream())


@pytest.mark.parametrize("batch,M", FT_CASES)
@pytest.mark.parametrize("head", list(HEADS))
def test_finetune_step(head, batch, M):
    L, f = lib(), Finetune(batch, M, head)
    o = dict(f.forward_outs(), grads=f32(f.numel), loss=f32(1))

    def call(ws, nbytes):
        return L.tmpnn_finetune_step(*f.model, ptr(f.m["target"]), M, *f.h, 1, ptr(f.params), ptr(o["grads"]), f.numel, 0.1, f.p_head, None,
                                     ptr(o.get("keep_out")), None, 7, 3, ptr(o["loss"]), ptr(o["pred"]), ptr(o.get("E_idx")), ptr(o["rows"]), ws,
                                     nbytes, stream())

    in_window(call, L.tmpnn_finetune_workspace_bytes(*f.sizes), o, offsets=AS_IS, short_by=1, grads=("grads",))


@pytest.mark.parametrize("batch,M", FT_CASES)
@pytest.mark.parametrize("head", list(HEADS))
def test_finetune_eval(head, batch, M):
    L, f = lib(), Finetune(batch, M, head)
    o = f.forward_outs()
    o.pop("keep_out", None)

    def call(ws, nbytes):
        return L.tmpnn_finetune_eval(*f.model, M, *f.h, 1, ptr(f.params), f.numel, ptr(o["pred"]), ptr(o.get("E_idx")), ptr(o["rows"]), ws, nbytes,
                                     stream())

    in_window(call, L.tmpnn_finetune_workspace_bytes(*f.sizes), o, offsets=AS_IS, short_by=1)


@pytest.mark.parametrize("batch,M", FT_CASES)
@pytest.mark.parametrize("head", list(HEADS))
def test_finetune_forward(head, batch, M):
    f = Finetune(batch, M, head)
    o = f.forward_outs()
    in_window(lambda saved, nbytes: f.forward(o, saved, nbytes), lib().tmpnn_finetune_saved_bytes(*f.sizes), o, offsets=AS_IS, short_by=1)


def backward_twice(backward, w, o, grads=("grads",)):
    """A backward over ``w["saved"]``: ``saved`` and its guards keep every byte; a second backward over the same ``saved``, with the
    scratch window refilled with another pattern, gives the same outputs. -> the first return code."""
    before = w["saved"].whole.clone()
    rc = backward(w)
    if rc != 0:
        return rc
    assert torch.equal(w["saved"].whole, before)
    first = {k: t.clone() for k, t in o.items()}
    w["scratch"].inside.fill_(0x33)
    for k, t in o.items():
        t.view(torch.uint8).fill_(0 if k in grads else 0xA5)
    assert backward(w) == 0
    assert torch.equal(w["saved"].whole, before)
    for k in o:
        assert same_bits(o[k], first[k]), k
    return rc


@pytest.mark.parametrize("batch,M", FT_CASES)
@pytest.mark.parametrize("head,form", [("released", "plain"), ("released", "x"), ("released", "head_only"), ("bare", "plain"), ("bare", "x")])
def test_finetune_backward(head, form, batch, M):
    """tmpnn_finetune_backward (also with mpnn_grads = 0: the head's part alone) and tmpnn_finetune_backward_x."""
    L, f = lib(), Finetune(batch, M, head)
    dpred, fo = normal(M, 10, 1.0), f.forward_outs()
    o = dict(grads=f32(f.numel))
    if form == "x":
        o["dX"] = f32(f.L, 4, 3)

    def prepare(w):
        assert f.forward(fo, w["saved"].ptr, w["saved"].nbytes) == 0

    def backward(w):
        head_ = (*f.model, M, *f.h, 1, ptr(f.params), f.numel, 0.1, f.p_head, None, None, 7, 3, ptr(dpred), ptr(o["grads"]))
        tail = (w["saved"].ptr, w["saved"].nbytes, w["scratch"].ptr, w["scratch"].nbytes, stream())
        if form == "x":
            return L.tmpnn_finetune_backward_x(*head_, ptr(o["dX"]), 1, *tail)
        return L.tmpnn_finetune_backward(*head_, 0 if form == "head_only" else 1, *tail)

    bufs = dict(saved=Buf(L.tmpnn_finetune_saved_bytes(*f.sizes), AS_IS, short_by=1),
                scratch=Buf(L.tmpnn_finetune_scratch_bytes(*f.sizes), AS_IS, short_by=1))
    guarded(lambda w: backward_twice(backward, w, o), bufs, o, grads=("grads",), prepare=prepare)


# ---- the sequence loss, one protein: the same carve (seq = true), the same rules ---------------------------------------------------------
SEQ_CASES = [("L17", 48), ("L40", 30)]                  # K = 17 = L; K = 30 < min(48, L): the edge-mask sites are laid out for 40


class Seqloss:
    def __init__(self, batch, k_neighbors, ranks):
        L = lib()
        self.p, self.kn = packed(batch), k_neighbors
        self.L = self.p["T"]
        self.K = min(k_neighbors, self.L)
        self.numel = L.tmpnn_seqloss_slab_numel()
        self.params = normal(self.numel, 6)
        self.ranks = dev(np.random.default_rng(11).permutation(self.L), torch.int32) if ranks else None
        self.model = tuple(ptr(self.p[k]) for k in ("X", "S", "mask", "ridx", "cenc")) + (self.L, k_neighbors, ptr(self.ranks), ptr(self.params),
                                                                                         self.numel, 0.1)

    def forward_outs(self):
        return dict(log_probs=f32(self.L, 21), keep_out=f32(lib().tmpnn_finetune_mask_numel(self.L)), E_idx=i32(self.L, self.K))

    def forward(self, o, saved, nbytes):
        return lib().tmpnn_seqloss_forward(*self.model, None, ptr(o["keep_out"]), 7, 3, ptr(o["log_probs"]), ptr(o["E_idx"]), saved, nbytes,
                                           stream())


@pytest.mark.parametrize("ranks", [True, False])
@pytest.mark.parametrize("batch,k_neighbors", SEQ_CASES)
def test_seqloss_forward(batch, k_neighbors, ranks):
    """With K < min(48, L) an edge site uses the first L K rows of its part of keep_out: the rest keeps the sentinel (``partial``)."""
    s = Seqloss(batch, k_neighbors, ranks)
    o = s.forward_outs()
    in_window(lambda saved, nbytes: s.forward(o, saved, nbytes), lib().tmpnn_seqloss_saved_bytes(s.L), o, offsets=AS_IS, short_by=1,
              partial=("keep_out",) if s.K < min(48, s.L) else ())


@pytest.mark.parametrize("x", [False, True])
@pytest.mark.parametrize("ranks", [True, False])
@pytest.mark.parametrize("batch,k_neighbors", SEQ_CASES)
def test_seqloss_backward(batch, k_neighbors, ranks, x):
    """tmpnn_seqloss_backward and tmpnn_seqloss_backward_x."""
    L, s = lib(), Seqloss(batch, k_neighbors, ranks)
    dlp, fo = normal(s.L * 21, 10, 1.0).view(s.L, 21), s.forward_outs()
    o = dict(grads=f32(s.numel))
    if x:
        o["dX"] = f32(s.L, 4, 3)

    def prepare(w):
        assert s.forward(fo, w["saved"].ptr, w["saved"].nbytes) == 0

    def backward(w):
        head_ = (*s.model, None, 7, 3, ptr(dlp), ptr(o["grads"]))
        tail = (w["saved"].ptr, w["saved"].nbytes, w["scratch"].ptr, w["scratch"].nbytes, stream())
        return L.tmpnn_seqloss_backward_x(*head_, ptr(o["dX"]), *tail) if x else L.tmpnn_seqloss_backward(*head_, *tail)

    bufs = dict(saved=Buf(L.tmpnn_seqloss_saved_bytes(s.L), AS_IS, short_by=1), scratch=Buf(L.tmpnn_seqloss_scratch_bytes(s.L), AS_IS, short_by=1))
    guarded(lambda w: backward_twice(backward, w, o), bufs, o, grads=("grads",), prepare=prepare)


# ---- the sequence loss, packed: ft_carve2 with the call's K and n_proteins ------------------------------------------------------------
BATCH_CASES = [("L17+L40", 16), ("2xL17", 48)]          # ragged at K = 16; padded: K = 17 < k_neighbors, accepted as min_len == max_len


class Seqbatch:
    def __init__(self, batch, k_neighbors):
        L = lib()
        self.p = p = packed(batch)
        self.T, self.n = p["T"], p["N"]
        lens = np.diff(p["starts"])
        self.K = min(k_neighbors, int(lens.min()))
        self.numel = L.tmpnn_seqloss_slab_numel()
        self.params = normal(self.numel, 6)
        self.ranks = dev(np.random.default_rng(11).permutation(self.T), torch.int32)
        self.model = tuple(ptr(p[k]) for k in ("X", "S", "mask", "ridx", "cenc", "offsets")) + (
            self.n, self.T, int(lens.min()), int(lens.max()), k_neighbors, ptr(self.ranks), ptr(self.params), self.numel, 0.1)
        self.sizes = (self.T, self.n, self.K)
        self.mask_bytes = 4 * L.tmpnn_seqloss_batch_mask_numel(self.T, self.K)

    def forward_outs(self):
        return dict(log_probs=f32(self.T, 21), E_idx=i32(self.T, self.K), status=i32(1))

    def forward(self, o, keep_out, saved, nbytes):
        return lib().tmpnn_seqloss_batch_forward(*self.model, None, keep_out, 7, 3, ptr(o["log_probs"]), ptr(o["E_idx"]), ptr(o["status"]), saved,
                                                 nbytes, stream())


@pytest.mark.parametrize("batch,k_neighbors", BATCH_CASES)
def test_seqloss_batch_forward(batch, k_neighbors):
    """keep_out has exactly tmpnn_seqloss_batch_mask_numel floats, every one written, and is guarded like the saved buffer (it has no
    size argument, so nothing is refused on its account)."""
    s = Seqbatch(batch, k_neighbors)
    o = s.forward_outs()
    bufs = dict(saved=Buf(lib().tmpnn_seqloss_batch_saved_bytes(*s.sizes), AS_IS, short_by=1), keep_out=Buf(s.mask_bytes, AS_IS))

    def extra(w):
        keep = w["keep_out"].inside.view(torch.float32)
        assert bool(((keep == 0) | (keep == 1)).all())
        return dict(keep_out=keep)

    guarded(lambda w: s.forward(o, w["keep_out"].ptr, w["saved"].ptr, w["saved"].nbytes), bufs, o, extra=extra)


@pytest.mark.parametrize("x", [False, True])
@pytest.mark.parametrize("batch,k_neighbors", BATCH_CASES)
def test_seqloss_batch_backward(batch, k_neighbors, x):
    """tmpnn_seqloss_batch_backward and tmpnn_seqloss_batch_backward_x."""
    L, s = lib(), Seqbatch(batch, k_neighbors)
    dlp, fo = normal(s.T * 21, 10, 1.0).view(s.T, 21), s.forward_outs()
    o = dict(grads=f32(s.numel))
    if x:
        o["dX"] = f32(s.T, 4, 3)

    def prepare(w):
        assert s.forward(fo, None, w["saved"].ptr, w["saved"].nbytes) == 0

    def backward(w):
        head_ = (*s.model, None, 7, 3, ptr(dlp), ptr(o["grads"]))
        tail = (w["saved"].ptr, w["saved"].nbytes, w["scratch"].ptr, w["scratch"].nbytes, stream())
        return L.tmpnn_seqloss_batch_backward_x(*head_, ptr(o["dX"]), *tail) if x else L.tmpnn_seqloss_batch_backward(*head_, *tail)

    bufs = dict(saved=Buf(L.tmpnn_seqloss_batch_saved_bytes(*s.sizes), AS_IS, short_by=1),
                scratch=Buf(L.tmpnn_seqloss_batch_scratch_bytes(*s.sizes), AS_IS, short_by=1))
    guarded(lambda w: backward_twice(backward, w, o), bufs, o, grads=("grads",), prepare=prepare)


# ---- selection: Carver(workspace, true), three offsets; the entries take what the carve fits: 257 bytes less (the sizer's 256 bytes of
# slack and one more) are refused on an aligned base. The 0x00 prefill is the one that matters: an all-zero key beats every candidate ----
@pytest.mark.parametrize("k", [1, 256])
def test_select_hits(k):
    """An empty protein, one of more than 256 rows (two stage-1 blocks) and two short ones; the smallest and the largest k."""
    L = lib()
    lens = [19, 0, 300, 40]
    T, P = sum(lens), len(lens)
    table, S, offs = dev(bits_table(T, 21, 71)), dev(letters(T, 72)), dev(offsets_of(lens))
    o = dict(hit_ddg=f32(P, k), hit_pos=i32(P, k), hit_aa=i32(P, k), hit_count=i32(P))

    def call(ws, nbytes):
        return L.tmpnn_select_hits(ptr(table), 21, ptr(S), ptr(offs), P, T, k, INF, 0, ptr(o["hit_ddg"]), ptr(o["hit_pos"]), ptr(o["hit_aa"]),
                                   ptr(o["hit_count"]), ws, nbytes, stream())

    count = in_window(call, L.tmpnn_hits_workspace_bytes(T, P, k), o, short_by=257)["hit_count"].tolist()
    assert count[1] == 0 and min(count[i] for i in (0, 2, 3)) >= 1


@pytest.mark.parametrize("V,Lr,k", [(5, 19, 33), (37, 300, 33), (37, 300, 256)])
def test_select_variant_hits(V, Lr, k):
    L = lib()
    c = {n: dev(a) for n, a in hits_case(V, Lr, 11).items()}
    o = dict(state=torch.empty(k, dtype=torch.int64, device=DEV), hit_ddg=f32(k), hit_tag=i32(k), hit_pos=i32(k), hit_aa=i32(k), hit_count=i32(1))

    def call(ws, nbytes):
        return L.tmpnn_select_variant_hits(ptr(c["ddg"]), 21, ptr(c["S_var"]), ptr(c["base"]), ptr(c["tag"]), ptr(c["skip"]), V, Lr, k, INF, 0,
                                           ptr(o["state"]), ptr(o["hit_ddg"]), ptr(o["hit_tag"]), ptr(o["hit_pos"]), ptr(o["hit_aa"]),
                                           ptr(o["hit_count"]), ws, nbytes, stream())

    assert int(in_window(call, L.tmpnn_variant_hits_workspace_bytes(V, Lr, k), o, short_by=257)["hit_count"].item()) >= 1


@pytest.mark.parametrize("V,Lr,rows", [(5, 19, [0, 0, 1, 1, 1]), (37, 300, [1] * 17 + [0] * 10 + [2] * 10)])
def test_pair_map(V, Lr, rows):
    """A fresh call (no CONTINUE) sets the whole state, the row that no variant names included."""
    L, R = lib(), 4
    c = {n: dev(a) for n, a in pmap_case(V, Lr, 13, specials=False).items()}
    row = dev(np.asarray(rows, np.int32))
    o = dict(best=torch.empty((R, Lr), dtype=torch.int64, device=DEV), eps_lo=torch.empty((R, Lr), dtype=torch.int64, device=DEV),
             eps_hi=torch.empty((R, Lr), dtype=torch.int64, device=DEV), eps_abs_sum=f32(R, Lr), count=i32(R, Lr))

    def call(ws, nbytes):
        return L.tmpnn_pair_map(ptr(c["ddg"]), 21, ptr(c["S_var"]), ptr(c["base"]), ptr(row), ptr(c["letter"]), ptr(c["skip"]), ptr(c["wt"]),
                                int(c["wt"].shape[1]), V, Lr, R, 0, *[ptr(o[n]) for n in ("best", "eps_lo", "eps_hi", "eps_abs_sum", "count")],
                                ws, nbytes, stream())

    assert int(in_window(call, L.tmpnn_pair_map_workspace_bytes(V, Lr), o, short_by=257)["count"].sum()) >= 1


@pytest.mark.parametrize("d,V,Lr,k", [(3, 37, 300, 32), (1, 1, 300, 256)])
def test_beam_step(d, V, Lr, k):
    L = lib()
    fx = duplicate_fixture(d, V, Lr, 5)
    c = {n: dev(fx[n]) for n in ("ddg", "S_var", "score")}
    muts = dev(fx["muts"]) if d > 1 else None
    o = dict(out_muts=i32(k, d), out_score=f32(k), out_parent=i32(k), out_S=i32(k, Lr), out_count=i32(1))

    def call(ws, nbytes):
        return L.tmpnn_beam_step(ptr(c["ddg"]), 21, ptr(c["S_var"]), ptr(c["score"]), ptr(muts), d, None, V, Lr, k, INF, 0, ptr(o["out_muts"]),
                                 ptr(o["out_score"]), ptr(o["out_parent"]), ptr(o["out_S"]), ptr(o["out_count"]), ws, nbytes, stream())

    assert int(in_window(call, L.tmpnn_beam_step_workspace_bytes(V, Lr, k, d), o, short_by=257)["out_count"].item()) >= 1


def test_beam_step_each():
    """The MIXED pack (an empty protein, one of 300 rows, one of 257) at k = 32: at max_len = 300, and at max_len = 2048, which changes
    the slots' item loops (ceil(max_len / 256) blocks per member) and must not change the result. (W itself is at its cap of
    8192 / 128 - 1 = 63 slots per protein in both: 37 members of two blocks already exceed it.)"""
    L = lib()
    d, V, k, P = 3, 37, 32, len(MIXED)
    fx = pack_fixture(d, V, MIXED, 5)
    c = {n: dev(fx[n]) for n in ("ddg", "S_var", "score", "muts", "offsets")}
    T = int(fx["offsets"][-1])
    o = dict(out_muts=i32(P, k, d), out_score=f32(P, k), out_parent=i32(P, k), out_S=i32(k, T), out_count=i32(P))
    seen = {}
    for max_len in (max(MIXED), 2048):
        def call(ws, nbytes):
            return L.tmpnn_beam_step_each(ptr(c["ddg"]), 21, ptr(c["S_var"]), ptr(c["score"]), ptr(c["muts"]), d, None, ptr(c["offsets"]), P, T, V,
                                          max_len, k, INF, 0, ptr(o["out_muts"]), ptr(o["out_score"]), ptr(o["out_parent"]), ptr(o["out_S"]),
                                          ptr(o["out_count"]), ws, nbytes, stream())

        need = L.tmpnn_beam_step_each_workspace_bytes(P, V, max_len, k, d)
        seen[max_len] = (need, in_window(call, need, o, short_by=257))
    (small, first), (large, second) = seen.values()
    assert large >= small and all(same_bits(first[n], second[n]) for n in o)
    assert first["out_count"].tolist()[2] == 0 and first["out_count"].tolist()[1] >= 1


# ---- alignment: Carver(workspace, true); the entry uses as many slots as the workspace holds, one is enough --------------------------------
@pytest.mark.parametrize("size", ["every_pair", "one_slot", "between"])
def test_align_global(size):
    """align_inputs.small_batch() (pairs up to 257 x 256) in a workspace for every pair, for one slot that serves every pair in turn (the
    smallest the header accepts: less than its slot is refused), and one that holds two slots and half of a third."""
    L = lib()
    A, B, desc, NO = align_pack([(a, b) for _, _, _, a, b in small_batch()])
    P = len(desc)
    one, slot = L.tmpnn_align_workspace_bytes(257, 257, 1), L.tmpnn_align_workspace_bytes(257, 257, 2) - L.tmpnn_align_workspace_bytes(257, 257, 1)
    assert P >= 3 and slot > 0 and L.tmpnn_align_workspace_bytes(257, 257, P) == one + (P - 1) * slot
    need = {"every_pair": one + (P - 1) * slot, "one_slot": one, "between": one + slot + slot // 2 + 4}[size]
    assert size != "between" or (need - 256) % slot
    dA, dB, dd = dev(A), dev(B), dev(desc)
    o = dict(out=i32(NO), aligned=i32(P), pair_status=i32(P))

    def call(ws, nbytes):
        return L.tmpnn_align_global(ptr(dA), len(A), ptr(dB), len(B), ptr(dd), P, 257, 257, ptr(o["out"]), NO, ptr(o["aligned"]),
                                    ptr(o["pair_status"]), ws, nbytes, stream())

    want = in_window(call, need, o, short_by=257 if size == "one_slot" else None)
    assert not bool(want["pair_status"].any()) and int(want["aligned"].max()) >= 250


# ---- bootstrap: Carver(workspace, true) in the workspace form; the LDS form takes none ---------------------------------------------------
def boot_inputs(N, B):
    values = fixture_values(N, 3)
    return dev(values), dev(dense_rank(values)), dev(fixture_rows(N, n_random=1)[:B])


def boot_outputs(B):
    return dict(metrics=torch.empty((B, 3, 5), dtype=torch.float64, device=DEV), ranks=torch.empty((B, 3, 3), dtype=torch.int64, device=DEV),
                row_status=i32(B))


@pytest.mark.parametrize("N,B", [(257, 5), (4099, 3)])
def test_bootstrap_metrics(N, B):
    """The workspace form (flags = 1). At N = 4099 the scan takes two tiles and the slots are padded to 4100 words."""
    L = lib()
    values, gid, idx = boot_inputs(N, B)
    assert idx.shape == (B, N)
    o = boot_outputs(B)

    def call(ws, nbytes):
        return L.tmpnn_bootstrap_metrics(ptr(values), ptr(gid), 4, N, ptr(idx), B, ptr(o["metrics"]), ptr(o["ranks"]), ptr(o["row_status"]), ws,
                                         nbytes, 1, stream())

    assert not bool(in_window(call, L.tmpnn_bootstrap_workspace_bytes(4, N, B, 1), o, short_by=257)["row_status"].any())


def test_bootstrap_lds_form_takes_no_workspace():
    """The sizer returns 0 for the LDS form; a null workspace of 0 bytes runs and gives the workspace form's bits."""
    L, N, B = lib(), 257, 5
    values, gid, idx = boot_inputs(N, B)
    assert L.tmpnn_bootstrap_workspace_bytes(4, N, B, 0) == 0
    got = {}
    for flags in (0, 1):
        o = boot_outputs(B)
        for t in o.values():
            t.view(torch.uint8).fill_(0xA5)
        ws = torch.zeros(L.tmpnn_bootstrap_workspace_bytes(4, N, B, 1), dtype=torch.uint8, device=DEV) if flags else None
        rc = L.tmpnn_bootstrap_metrics(ptr(values), ptr(gid), 4, N, ptr(idx), B, ptr(o["metrics"]), ptr(o["ranks"]), ptr(o["row_status"]), ptr(ws),
                                       ws.numel() if flags else 0, flags, stream())
        assert rc == 0, L.tmpnn_last_error()
        assert not bool(o["row_status"].any()) and not any(bool(stale(t).any()) for t in o.values())
        got[flags] = o
    assert all(same_bits(got[0][n], got[1][n]) for n in got[0])
