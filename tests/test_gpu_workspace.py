"""Every C-ABI entry that takes a caller-owned workspace, run inside exactly the bytes its *_bytes() function reports.

The allocation is need + 4096 bytes of 0xFF (NaN as a float, a huge value as an int); the entry gets the window [off, off + need) for
off in 0, 16, 240, and afterwards every output equals, bit for bit, what a roomy, aligned, zero-filled workspace gave, and every byte
outside the window is still 0xFF. So no entry writes past the size it reports, no two arrays of its carve overlap, none reads
workspace it has not written, and the result does not depend on the base's alignment. The C-ABI is driven through ``_lib`` directly:
``Engine`` would substitute its own workspace. Backbones: msk_L17 (fewer residues than neighbour slots), msk_L40, and the two packed."""
import ctypes as C

import numpy as np
import pytest
import torch

from masked_backbones import pack, protein

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSETS = (0, 16, 240)
BATCHES = {"L17": ("msk_L17",), "L40": ("msk_L40",), "L17+L40": ("msk_L17", "msk_L40")}
_ENGINES, _PACKED, _CTX = {}, {}, {}


def engine(precision):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if precision not in _ENGINES:
        _ENGINES[precision] = Engine(synthetic_state_dict(0), DEV, 48, precision=precision, retry_precision=None)
    return _ENGINES[precision]


def packed(batch):
    if batch not in _PACKED:
        p = pack([protein(n) for n in BATCHES[batch]])
        p["offsets"] = p["offsets"].to(DEV)
        p["T"], p["N"], p["max_len"] = int(p["starts"][-1]), len(p["starts"]) - 1, int(np.diff(p["starts"]).max())
        _PACKED[batch] = p
    return _PACKED[batch]


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def in_window(call, need, outputs, offsets=OFFSETS):
    """``call(ws pointer, ws bytes)`` launches the entry (and returns its code); ``outputs()`` -> fresh clones of what it wrote,
    the status word among them. Reference first, then the guarded windows."""
    assert need > 0
    roomy = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    assert roomy.data_ptr() % 256 == 0
    assert call(ptr(roomy), roomy.numel()) == 0, engine("f16x2").lib.tmpnn_last_error()
    want = outputs()
    assert int(want["status"].item()) == 0
    for off in offsets:
        buf = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 256 == 0
        rc = call(ptr(buf, off), need)
        assert rc == 0, (off, engine("f16x2").lib.tmpnn_last_error())
        got = outputs()
        for k in want:
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), (off, k)
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + need:] == 0xFF).all()), off


def encode_into(precision, batch, ctx, status, ws, ws_bytes):
    eng, p = engine(precision), packed(batch)
    return eng.lib.tmpnn_encode(eng.w.handle, ptr(p["X"]), ptr(p["mask"]), ptr(p["ridx"]), ptr(p["cenc"]), ptr(p["offsets"]), p["N"], p["T"],
                                p["max_len"], 48, ptr(ctx), ctx.numel(), ptr(status), ws, ws_bytes, stream())


def context(precision, batch):
    """The encoded backbone, made once with a roomy workspace: exactly tmpnn_encode_bytes(T) bytes."""
    if (precision, batch) not in _CTX:
        eng, T = engine(precision), packed(batch)["T"]
        ctx = torch.full((eng.lib.tmpnn_encode_bytes(T),), 0xFF, dtype=torch.uint8, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.zeros(eng.lib.tmpnn_encode_workspace_bytes(T) + 4096, dtype=torch.uint8, device=DEV)
        assert encode_into(precision, batch, ctx, status, ptr(ws), ws.numel()) == 0 and int(status.item()) == 0
        _CTX[precision, batch] = ctx
    return _CTX[precision, batch]


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ssm_forward(batch):
    eng, p = engine("f16x2"), packed(batch)
    T = p["T"]
    o = dict(ddg=torch.empty((T, 21), device=DEV), hidden=torch.empty((3, T, 128), device=DEV), log_probs=torch.empty((T, 21), device=DEV),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(ws, nbytes):
        for t in o.values():
            t.view(torch.uint8).fill_(0xFF)
        return eng.lib.tmpnn_ssm_forward(eng.w.handle, ptr(p["X"]), ptr(p["S"]), ptr(p["mask"]), ptr(p["ridx"]), ptr(p["cenc"]),
                                         ptr(p["offsets"]), p["N"], T, p["max_len"], 48, ptr(o["ddg"]), ptr(o["hidden"]), ptr(o["log_probs"]),
                                         None, ptr(o["status"]), ws, nbytes, stream())

    in_window(call, eng.lib.tmpnn_workspace_bytes(T), lambda: {k: v.clone() for k, v in o.items()})


@pytest.mark.parametrize("batch", list(BATCHES))
def test_encode(batch):
    """The ctx is an output: exactly tmpnn_encode_bytes(T) bytes inside a guarded allocation of its own (a ctx must be aligned)."""
    eng, T = engine("f16x2"), packed(batch)["T"]
    nctx = eng.lib.tmpnn_encode_bytes(T)
    guard = torch.empty(nctx + 4096, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(ws, nbytes):
        guard.fill_(0xFF)
        status.fill_(-1)
        return encode_into("f16x2", batch, guard[:nctx], status, ws, nbytes)

    def outputs():
        assert bool((guard[nctx:] == 0xFF).all())
        return dict(ctx=guard[:nctx].clone(), status=status.clone())

    in_window(call, eng.lib.tmpnn_encode_workspace_bytes(T), outputs)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("entry,precision", [("variants", "f16x2"), ("ordered", "f16x2"), ("ordered", "fp32")])
def test_decode(entry, precision, batch):
    """V = 3 variants; ordered: random ranks, and the fp32 form as well (the one reader of the remap array)."""
    eng, p, ctx = engine(precision), packed(batch), context(precision, batch)
    T, V = p["T"], 3
    rng = np.random.default_rng(3)
    S = torch.from_numpy(rng.integers(0, 21, (V, T))).to(DEV, torch.int32)
    R = torch.from_numpy(np.stack([rng.permutation(T) for _ in range(V)])).to(DEV, torch.int32)
    o = dict(ddg=torch.empty((V, T, 21), device=DEV), hidden=torch.empty((V, 3, T, 128), device=DEV),
             log_probs=torch.empty((V, T, 21), device=DEV), status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(ws, nbytes):
        for t in o.values():
            t.view(torch.uint8).fill_(0xFF)
        head = (eng.w.handle, ptr(ctx), ctx.numel(), ptr(S))
        tail = (V, ptr(p["mask"]), T, ptr(o["ddg"]), ptr(o["hidden"]), ptr(o["log_probs"]), ptr(o["status"]), ws, nbytes, stream())
        if entry == "ordered":
            return eng.lib.tmpnn_decode_ordered(*head, ptr(R), *tail)
        return eng.lib.tmpnn_decode_variants(*head, *tail)

    sizer = eng.lib.tmpnn_decode_ordered_workspace_bytes if entry == "ordered" else eng.lib.tmpnn_decode_variants_workspace_bytes
    in_window(call, sizer(T, V), lambda: {k: v.clone() for k, v in o.items()})


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
def test_sample(precision, batch):
    """N = 17 chains: one full group of 16 and one more."""
    eng, p, ctx = engine(precision), packed(batch), context(precision, batch)
    T, N = p["T"], 17
    rng = np.random.default_rng(5)
    order = torch.from_numpy(np.stack([rng.permutation(T) for _ in range(N)])).to(DEV, torch.int32)
    S_fixed = torch.from_numpy(rng.integers(0, 21, (N, T))).to(DEV, torch.int32)
    free = torch.ones((N, T), device=DEV)
    u = torch.from_numpy(rng.random((N, T)).astype(np.float32)).to(DEV)
    o = dict(S=torch.empty((N, T), dtype=torch.int32, device=DEV), probs=torch.empty((N, T, 21), device=DEV),
             status=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(ws, nbytes):
        for t in o.values():
            t.view(torch.uint8).fill_(0xFF)
        return eng.lib.tmpnn_sample(eng.w.handle, ptr(ctx), ctx.numel(), ptr(p["mask"]), T, N, ptr(order), ptr(S_fixed), ptr(free), ptr(u), 1.0,
                                    None, None, ptr(o["S"]), ptr(o["probs"]), ptr(o["status"]), ws, nbytes, stream())

    in_window(call, eng.lib.tmpnn_sample_workspace_bytes(T, N), lambda: {k: v.clone() for k, v in o.items()})


@pytest.mark.parametrize("batch", list(BATCHES))
def test_ddg_head_generic(batch):
    """The released head through the generic entry, which uses the caller's base as is: offset 0 only."""
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

    def call(ws, nbytes):
        o["ddg"].view(torch.uint8).fill_(0xFF)
        o["z"].view(torch.uint8).fill_(0xFF)
        o["status"].zero_()              # (this entry ORs into the word; the caller clears it)
        return eng.lib.tmpnn_ddg_head_generic(arr([hidden[2], hidden[1]]), 2, ptr(sd["prot_mpnn.W_s.weight"]), ptr(p["S"]), T,
                                              ptr(sd["light_attention.feature_convolution.weight"]),
                                              ptr(sd["light_attention.feature_convolution.bias"]), 3, arr(mlp_w), arr(mlp_b), dims,
                                              ptr(sd["ddg_out.weight"]), ptr(sd["ddg_out.bias"]), ptr(o["ddg"]), ptr(o["z"]), ws, nbytes,
                                              ptr(o["status"]), stream())

    in_window(call, eng.lib.tmpnn_head_generic_workspace_bytes(T, 2, 3, dims), lambda: {k: v.clone() for k, v in o.items()}, offsets=(0,))
