"""Every C-ABI entry that takes a caller-owned buffer, run inside exactly the bytes its *_bytes() function reports.

``COVERED`` below names every such entry of include/tmpnn.h and the test(s) that guard it; tests/test_workspace_host.py holds the
table to the header, so an entry cannot be added without a window test. The fused forward, the encoder, the two decodes, the sampler
and the generic head are tested here, everything else in tests/test_gpu_workspace_entries.py with the helper of this file.

``guarded``: every buffer of a call is a window of exactly ``need`` bytes at offset ``off`` inside an allocation of its own that is
filled with one byte pattern and ends in a tail guard of 64 KiB (an overrun by a whole row of 128 floats x 48 neighbours stays inside
memory the test owns). Entries that align the base themselves (Carver(ws, true)) get off in 0, 16, 240; entries that take the base as
it is (Carver(.., false)) get 0. Three prefills: 0xFF (a NaN as a float, "no candidate" as a selection key), 0x00 (the key that beats
every real candidate, a zero float) and 0x5A (a finite float of about 1.5e16, a plausible int). Under every prefill and offset each
output equals, bit for bit, what a roomy, aligned, zero-filled buffer gave, and every byte outside the windows still holds the
prefill. So no entry writes past the size it reports, no two arrays of a carve overlap, none reads what it has not written, and the
result does not depend on the base's alignment. That the entry ran at all: every output is filled with 0xA5 before each call, the
roomy run must leave status 0 and no 0xA5A5.. word in any output (``partial`` outputs: not only such words), and gradients, which the
entries add into a zeroed slab, must be finite and not all zero. Where the contract is "need bytes or refuse", ``short_by`` bytes less
are refused with TMPNN_E_WORKSPACE and leave every output and every byte of every buffer untouched. Whether the VALUES are right is the
business of the parity tests; this file proves that they do not depend on the bytes around or inside the buffers. The C-ABI is driven
through ``_lib`` directly: ``Engine`` would substitute its own workspace. Backbones: msk_L17 (fewer residues than neighbour slots),
msk_L40, the two packed, and L17 + L40 + L17 for the per-protein samplers."""
import ctypes as C

import numpy as np
import pytest
import torch

from masked_backbones import pack, protein

pytestmark = pytest.mark.gpu

# C entry -> the tests that run it in guarded windows ("<module>::<test>"); tests/test_workspace_host.py compares with the header
_HERE, _ENTRIES = "test_gpu_workspace", "test_gpu_workspace_entries"
COVERED = {
    "tmpnn_ssm_forward": [f"{_HERE}::test_ssm_forward", f"{_ENTRIES}::test_ca_forward"],
    "tmpnn_encode": [f"{_HERE}::test_encode", f"{_ENTRIES}::test_ca_encode"],
    "tmpnn_decode_variants": [f"{_HERE}::test_decode"],
    "tmpnn_decode_ordered": [f"{_HERE}::test_decode"],
    "tmpnn_sample": [f"{_HERE}::test_sample"],
    "tmpnn_ddg_head_generic": [f"{_HERE}::test_ddg_head_generic"],
    "tmpnn_enc_layer": [f"{_ENTRIES}::test_enc_layer"],
    "tmpnn_dec_layer": [f"{_ENTRIES}::test_dec_layer"],
    "tmpnn_weights_create": [f"{_ENTRIES}::test_weight_images"],
    "tmpnn_weights_create_p": [f"{_ENTRIES}::test_weight_images"],
    "tmpnn_weights_create_ca": [f"{_ENTRIES}::test_weight_images"],
    "tmpnn_sample_tied": [f"{_ENTRIES}::test_sample_tied"],
    "tmpnn_sample_each": [f"{_ENTRIES}::test_sample_each"],
    "tmpnn_sample_tied_each": [f"{_ENTRIES}::test_sample_tied_each"],
    "tmpnn_head_train_step": [f"{_ENTRIES}::test_head_train_step"],
    "tmpnn_head_eval": [f"{_ENTRIES}::test_head_eval"],
    "tmpnn_finetune_step": [f"{_ENTRIES}::test_finetune_step"],
    "tmpnn_finetune_eval": [f"{_ENTRIES}::test_finetune_eval"],
    "tmpnn_finetune_forward": [f"{_ENTRIES}::test_finetune_forward"],
    "tmpnn_finetune_backward": [f"{_ENTRIES}::test_finetune_backward"],
    "tmpnn_finetune_backward_x": [f"{_ENTRIES}::test_finetune_backward"],
    "tmpnn_seqloss_forward": [f"{_ENTRIES}::test_seqloss_forward"],
    "tmpnn_seqloss_backward": [f"{_ENTRIES}::test_seqloss_backward"],
    "tmpnn_seqloss_backward_x": [f"{_ENTRIES}::test_seqloss_backward"],
    "tmpnn_seqloss_batch_forward": [f"{_ENTRIES}::test_seqloss_batch_forward"],
    "tmpnn_seqloss_batch_backward": [f"{_ENTRIES}::test_seqloss_batch_backward"],
    "tmpnn_seqloss_batch_backward_x": [f"{_ENTRIES}::test_seqloss_batch_backward"],
    "tmpnn_select_hits": [f"{_ENTRIES}::test_select_hits"],
    "tmpnn_select_variant_hits": [f"{_ENTRIES}::test_select_variant_hits"],
    "tmpnn_pair_map": [f"{_ENTRIES}::test_pair_map"],
    "tmpnn_beam_step": [f"{_ENTRIES}::test_beam_step"],
    "tmpnn_beam_step_each": [f"{_ENTRIES}::test_beam_step_each"],
    "tmpnn_align_global": [f"{_ENTRIES}::test_align_global"],
    "tmpnn_bootstrap_metrics": [f"{_ENTRIES}::test_bootstrap_metrics", f"{_ENTRIES}::test_bootstrap_lds_form_takes_no_workspace"],
}

DEV = "cuda:0"
OFFSETS = (0, 16, 240)          # window offsets for an entry that aligns the base itself
AS_IS = (0,)                    # ... for an entry that takes the base as it is
PREFILLS = (0xFF, 0x00, 0x5A)
TAIL = 1 << 16                  # the tail guard; the front guard is the offset
SENTINEL = 0xA5                 # what every output holds before a call
E_WORKSPACE = -4
BATCHES = {"L17": ("msk_L17",), "L40": ("msk_L40",), "L17+L40": ("msk_L17", "msk_L40")}
PACKS = dict(BATCHES, **{"L17+L40+L17": ("msk_L17", "msk_L40", "msk_L17"), "2xL17": ("msk_L17", "msk_L17")})
_ENGINES, _PACKED, _CTX = {}, {}, {}


def engine(precision):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if precision not in _ENGINES:
        _ENGINES[precision] = Engine(synthetic_state_dict(0), DEV, 48, precision=precision, retry_precision=None)
    return _ENGINES[precision]


def lib():
    from thermompnn_amd import _lib
    return _lib.load()


def packed(batch):
    if batch not in _PACKED:
        p = pack([protein(n) for n in PACKS[batch]])
        p["offsets"] = p["offsets"].to(DEV)
        p["T"], p["N"], p["max_len"] = int(p["starts"][-1]), len(p["starts"]) - 1, int(np.diff(p["starts"]).max())
        _PACKED[batch] = p
    return _PACKED[batch]


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """One caller-owned buffer of an entry: its size, the window offsets it is tried at and, where the entry refuses a smaller one,
    by how many bytes the refused size is smaller (1: the entry compares with the size itself; 257: the entry aligns the base and takes
    what its carve fits, the sizer adds one alignment's 256 bytes of slack, so on an aligned base the carve is need - 256)."""

    def __init__(self, need, offsets=OFFSETS, short_by=None):
        assert need > 0
        self.need, self.offsets, self.short_by = int(need), tuple(offsets), short_by


class Window:
    """``need`` bytes at ``off`` inside an allocation of off + need + TAIL bytes of ``fill``; ``nbytes`` is what the entry is told
    (``room`` bytes more for the roomy reference, which has no guards); ``inside`` is the first ``need`` bytes of the window."""

    def __init__(self, need, off, fill, tail=TAIL, room=0):
        self.need, self.off, self.fill, self.nbytes = need, off, fill, need + room
        self.whole = torch.full((off + need + room + tail,), fill, dtype=torch.uint8, device=DEV)
        assert self.whole.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.whole.data_ptr() + off)
        self.inside = self.whole[off:off + need]

    def guards_intact(self):
        return bool((self.whole[:self.off] == self.fill).all()) and bool((self.whole[self.off + self.need:] == self.fill).all())

    def untouched(self):
        return bool((self.whole == self.fill).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def stale(t):
    """[numel] bool: the elements that still hold the sentinel in every byte."""
    return (t.contiguous().view(torch.uint8).reshape(-1, t.element_size()) == SENTINEL).all(dim=1)


def guarded(call, bufs, outs, zeroed=(), grads=(), partial=(), prepare=None, extra=None):
    """``call(w)`` launches the entry on the windows ``w[name]`` (``.ptr``, ``.nbytes``) of ``bufs`` {name: Buf} and returns its code.
    ``outs`` {name: tensor}: what it writes, the status word among them; each is filled with the sentinel before every call, the ones in
    ``zeroed`` (a word the entry ORs into) and ``grads`` (a slab the entry adds its non-zero entries to) with zeros. ``partial``: outputs
    that the entry's contract leaves unwritten in part. ``prepare(w)`` runs before the call (a forward that fills ``saved``), and
    ``extra(w)`` -> more tensors to compare (parts of a buffer that is itself an output). Reference first, then the windows.
    -> the reference outputs."""
    def fresh():
        for k, t in outs.items():
            assert t.is_contiguous()
            t.view(torch.uint8).fill_(0 if k in zeroed or k in grads else SENTINEL)

    def run(w, what):
        fresh()
        if prepare:
            prepare(w)
        rc = call(w)
        assert rc == 0, (what, rc, lib().tmpnn_last_error())
        got = {k: t.clone() for k, t in outs.items()}
        if extra:
            got.update({k: t.clone() for k, t in extra(w).items()})
        return got

    want = run({name: Window(b.need, 0, 0x00, tail=0, room=4096) for name, b in bufs.items()}, "roomy")
    if "status" in want:
        assert int(want["status"].item()) == 0
    for k in outs:
        if k in grads:
            assert bool(torch.isfinite(want[k]).all()) and bool((want[k] != 0).any()), k
        elif k not in zeroed:
            left = stale(want[k])
            assert not bool(left.all() if k in partial else left.any()), (k, int(left.sum()))
    for fill in PREFILLS:
        for i in range(max(len(b.offsets) for b in bufs.values())):
            w = {name: Window(b.need, b.offsets[i % len(b.offsets)], fill) for name, b in bufs.items()}
            at = (hex(fill), {name: x.off for name, x in w.items()})
            got = run(w, at)
            for k in want:
                assert same_bits(got[k], want[k]), (at, k)
            for name, x in w.items():
                assert x.guards_intact(), (at, name)
    for name, b in bufs.items():
        if b.short_by is None:
            continue
        w = {n: Window(x.need, 0, 0x5A) for n, x in bufs.items()}
        w[name].nbytes = b.need - b.short_by
        fresh()
        assert call(w) == E_WORKSPACE, (name, lib().tmpnn_last_error())
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert bool((t.view(torch.uint8) == (0 if k in zeroed or k in grads else SENTINEL)).all()), (name, k)
        for n, x in w.items():
            assert x.untouched(), (name, n)
    return want


def in_window(call, need, outs, offsets=OFFSETS, short_by=None, **kw):
    """The entries with one buffer: ``call(ws pointer, ws bytes)``."""
    return guarded(lambda w: call(w["ws"].ptr, w["ws"].nbytes), dict(ws=Buf(need, offsets, short_by)), outs, **kw)


def encode_into(precision, batch, ctx, ctx_bytes, status, ws, ws_bytes, eng=None):
    eng, p = eng or engine(precision), packed(batch)
    return eng.lib.tmpnn_encode(eng.w.handle, ptr(p["X"]), ptr(p["mask"]), ptr(p["ridx"]), ptr(p["cenc"]), ptr(p["offsets"]), p["N"], p["T"],
                                p["max_len"], 48, ctx, ctx_bytes, ptr(status), ws, ws_bytes, stream())


def context(precision, batch):
    """The encoded backbone, made once with a roomy workspace: exactly tmpnn_encode_bytes(T) bytes."""
    if (precision, batch) not in _CTX:
        eng, T = engine(precision), packed(batch)["T"]
        ctx = torch.full((eng.lib.tmpnn_encode_bytes(T),), 0xFF, dtype=torch.uint8, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.zeros(eng.lib.tmpnn_encode_workspace_bytes(T) + 4096, dtype=torch.uint8, device=DEV)
        assert encode_into(precision, batch, ptr(ctx), ctx.numel(), status, ptr(ws), ws.numel()) == 0 and int(status.item()) == 0
        _CTX[precision, batch] = ctx
    return _CTX[precision, batch]


def forward_case(eng, batch, ddg=True):
    """tmpnn_ssm_forward on a batch (aligns the base: three offsets; takes what its carve fits: refusals are test_workspace_host.py's)."""
    p = packed(batch)
    T = p["T"]
    o = dict(hidden=torch.empty((3, T, 128), device=DEV), log_probs=torch.empty((T, 21), device=DEV),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))
    if ddg:
        o["ddg"] = torch.empty((T, 21), device=DEV)

    def call(ws, nbytes):
        return eng.lib.tmpnn_ssm_forward(eng.w.handle, ptr(p["X"]), ptr(p["S"]), ptr(p["mask"]), ptr(p["ridx"]), ptr(p["cenc"]),
                                         ptr(p["offsets"]), p["N"], T, p["max_len"], 48, ptr(o.get("ddg")), ptr(o["hidden"]), ptr(o["log_probs"]),
                                         None, ptr(o["status"]), ws, nbytes, stream())

    in_window(call, eng.lib.tmpnn_workspace_bytes(T), o)


def encode_case(eng, batch):
    """tmpnn_encode: the workspace (aligned by the entry: three offsets) and the ctx, an output that the entry takes as it is (it must be
    aligned: offset 0), exactly tmpnn_encode_bytes(T) bytes in a guarded allocation of its own; one byte less is refused. The ctx's
    arrays are compared, not the 64 bytes of padding behind E_idx [T,48], which keep the prefill."""
    T = packed(batch)["T"]
    nctx, o1 = eng.lib.tmpnn_encode_bytes(T), (T * 192 + 255) & ~255
    assert nctx == o1 + T * (48 * 128 + 128 + 256) * 4
    o = dict(status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(w):
        return encode_into(None, batch, w["ctx"].ptr, w["ctx"].nbytes, o["status"], w["ws"].ptr, w["ws"].nbytes, eng=eng)

    def extra(w):
        return dict(E_idx=w["ctx"].inside[:T * 192], arrays=w["ctx"].inside[o1:])

    guarded(call, dict(ws=Buf(eng.lib.tmpnn_encode_workspace_bytes(T)), ctx=Buf(nctx, AS_IS, short_by=1)), o, extra=extra)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ssm_forward(batch):
    forward_case(engine("f16x2"), batch)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_encode(batch):
    encode_case(engine("f16x2"), batch)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("entry,precision", [("variants", "f16x2"), ("ordered", "f16x2"), ("ordered", "fp32")])
def test_decode(entry, precision, batch):
    """V = 3 variants; ordered: random ranks, and the fp32 form as well (the one reader of the remap array). Both entries align the
    base (three offsets) and compare the byte count with their sizer first: one byte less is refused."""
    eng, p, ctx = engine(precision), packed(batch), context(precision, batch)
    T, V = p["T"], 3
    rng = np.random.default_rng(3)
    S = torch.from_numpy(rng.integers(0, 21, (V, T))).to(DEV, torch.int32)
    R = torch.from_numpy(np.stack([rng.permutation(T) for _ in range(V)])).to(DEV, torch.int32)
    o = dict(ddg=torch.empty((V, T, 21), device=DEV), hidden=torch.empty((V, 3, T, 128), device=DEV),
             log_probs=torch.empty((V, T, 21), device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(ws, nbytes):
        head = (eng.w.handle, ptr(ctx), ctx.numel(), ptr(S))
        tail = (V, ptr(p["mask"]), T, ptr(o["ddg"]), ptr(o["hidden"]), ptr(o["log_probs"]), ptr(o["status"]), ws, nbytes, stream())
        if entry == "ordered":
            return eng.lib.tmpnn_decode_ordered(*head, ptr(R), *tail)
        return eng.lib.tmpnn_decode_variants(*head, *tail)

    sizer = eng.lib.tmpnn_decode_ordered_workspace_bytes if entry == "ordered" else eng.lib.tmpnn_decode_variants_workspace_bytes
    in_window(call, sizer(T, V), o, short_by=1)


def sampler_inputs(T, N, seed=5):
    rng = np.random.default_rng(seed)
    return dict(order=torch.from_numpy(np.stack([rng.permutation(T) for _ in range(N)])).to(DEV, torch.int32),
                S_fixed=torch.from_numpy(rng.integers(0, 21, (N, T))).to(DEV, torch.int32), free=torch.ones((N, T), device=DEV),
                u=torch.from_numpy(rng.random((N, T)).astype(np.float32)).to(DEV))


def sampler_outputs(T, N):
    return dict(S=torch.empty((N, T), dtype=torch.int32, device=DEV), probs=torch.empty((N, T, 21), device=DEV),
                status=torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample(precision, batch):
    """N = 17 chains: one full group of 16 and one more. Aligns the base; compares with the sizer first."""
    eng, p, ctx = engine(precision), packed(batch), context(precision, batch)
    T, N = p["T"], 17
    c, o = sampler_inputs(T, N), sampler_outputs(T, N)

    def call(ws, nbytes):
        return eng.lib.tmpnn_sample(eng.w.handle, ptr(ctx), ctx.numel(), ptr(p["mask"]), T, N, ptr(c["order"]), ptr(c["S_fixed"]), ptr(c["free"]),
                                    ptr(c["u"]), 1.0, None, None, ptr(o["S"]), ptr(o["probs"]), ptr(o["status"]), ws, nbytes, stream())

    in_window(call, eng.lib.tmpnn_sample_workspace_bytes(T, N), o, short_by=1)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ddg_head_generic(batch):
    """The released head through the generic entry, which uses the caller's base as is: offset 0 only; one byte less is refused."""
    from thermompnn_amd.weights import synthetic_state_dict
    eng, p = engine("f16x2"), packed(batch)
    T = p["T"]
    names = ["prot_mpnn.W_s.weight", "light_attention.feature_convolution.weight", "light_attention.feature_convolution.bias",
             "ddg_out.weight", "ddg_out.bias"] + [f"both_out.{i}.{wb}" for i in (1, 3, 5) for wb in ("weight", "bias")]
    sd = {k: v.to(DEV, torch.float32).contiguous() for k, v in synthetic_state_dict(0).items() if k in names}
    assert len(sd) == len(names)
    hidden = eng.ssm_forward(p["X"], p["S"], p["mask"], p["ridx"], p["cenc"], p["offsets"].cpu(), want_ddg=False, want_hidden=True)["hidden"]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    mlp_w, mlp_b = [sd[f"both_out.{i}.weight"] for i in (1, 3, 5)], [sd[f"both_out.{i}.bias"] for i in (1, 3, 5)]
    dims = (C.c_int32 * 4)(384, 64, 32, 21)
    o = dict(ddg=torch.empty((T, 21), device=DEV), z=torch.empty((T, 21), device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(ws, nbytes):               # (this entry ORs into the status word; the caller clears it: ``zeroed``)
        return eng.lib.tmpnn_ddg_head_generic(arr([hidden[2], hidden[1]]), 2, ptr(sd["prot_mpnn.W_s.weight"]), ptr(p["S"]), T,
                                              ptr(sd["light_attention.feature_convolution.weight"]),
                                              ptr(sd["light_attention.feature_convolution.bias"]), 3, arr(mlp_w), arr(mlp_b), dims,
                                              ptr(sd["ddg_out.weight"]), ptr(sd["ddg_out.bias"]), ptr(o["ddg"]), ptr(o["z"]), ws, nbytes,
                                              ptr(o["status"]), stream())

    in_window(call, eng.lib.tmpnn_head_generic_workspace_bytes(T, 2, 3, dims), o, offsets=AS_IS, short_by=1, zeroed=("status",))


def test_the_helper_sees_what_it_is_for():
    """``guarded`` on stand-in entries written with torch on the window's own allocation: a sound one passes; one byte written behind
    the window or in front of it, a scratch word read before it is written, a key slot read before it is written (all ones, "no
    candidate", under 0xFF, where the result is right by accident: it is the zero-filled reference, whose empty slots beat every key,
    that the 0xFF run disagrees with), an entry that does nothing, and one that runs on less than it reports are
    each caught."""
    need = 1024
    o = dict(value=torch.empty(4, dtype=torch.int64, device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV))
    real = torch.tensor([7, 9, 11, 13], dtype=torch.int64, device=DEV)

    def entry(fault):
        def call(w):
            ws = w["ws"]
            if ws.nbytes < need + 256 and fault != "never_refuses":         # (compares with its sizer first, as the decodes do)
                return E_WORKSPACE
            base = ws.off + (-ws.off % 256)                          # the stand-in aligns its base, as Carver(ws, true) does
            keys = ws.whole[base:base + 64].view(torch.int64)
            if fault != "unwritten_key":
                keys[4:] = -1                                        # "no candidate"
            keys[:4] = real
            o["value"].copy_(torch.where(keys[4:] == -1, keys[:4], torch.minimum(keys[:4], keys[4:])))   # a merge; all ones = none
            if fault == "unwritten_scratch":
                o["value"][0] += ws.whole[base + 128:base + 136].view(torch.int64)[0]
            if fault == "behind":
                ws.whole[ws.off + ws.need] = 1
            if fault == "in_front" and ws.off:
                ws.whole[ws.off - 1] = 1
            o["status"].zero_()
            return 0
        return (lambda w: 0) if fault == "nothing" else call

    bufs = dict(ws=Buf(need + 256, OFFSETS, short_by=1))
    assert torch.equal(guarded(entry(None), bufs, o)["value"], real)
    for fault in ("behind", "in_front", "unwritten_scratch", "unwritten_key", "nothing", "never_refuses"):
        with pytest.raises(AssertionError) as e:
            guarded(entry(fault), bufs, o)
        assert fault != "unwritten_key" or "'0xff'" in str(e.value), str(e.value)
