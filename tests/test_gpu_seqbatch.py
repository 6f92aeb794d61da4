"""The packed sequence loss on the MI355X (tmpnn_seqloss_batch_forward / _backward, model_utils.SeqBatchFunction, ProteinMPNN.packed):
every member of a ragged batch against its own single call bit for bit, n_proteins = 1 against the single entries, the batch gradient
against the float64 restatement summed over proteins, the dropout numbering over packed rows, the status word, and the module."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden
from lattice_backbones import backbone
from masked_backbones import layout_arrays
from seqloss_restatement import grads_f64, log_probs_f64
from test_gpu_finetune import numpy_site_mask
from test_gpu_seqloss import FINETUNE_TOL, Call, _batch, _module, _ranks, _sd, _split
from train_weight_cases import HOT_F64_FACTOR, check_against_golden, mpnn_weights

pytestmark = pytest.mark.gpu

RAGGED = ("msk_L40", "msk_L56_2ch", "lat32")
K_RAGGED = 30


def _arrays(name):
    if name == "lat32":                                   # the first 32 residues of the L = 49 lattice layout (some of them masked)
        g = backbone("lat_L49m")
        return tuple(np.asarray(g[k])[:32] for k in ("X", "S", "mask", "ridx", "cenc"))
    return layout_arrays(name)


class BatchCall:
    """tmpnn_seqloss_batch_forward / _backward called directly on proteins packed in the given order."""

    def __init__(self, prots, ranks, k, sd=None, min_len=None, max_len=None):
        from thermompnn_amd import _lib
        self.lib = _lib.load()
        t = lambda xs, dt: torch.cat([torch.as_tensor(np.asarray(x)) for x in xs]).to("cuda", dt).contiguous()
        self.X, self.mask = t([p[0] for p in prots], torch.float32), t([p[2] for p in prots], torch.float32)
        self.S, self.ridx, self.cenc = (t([p[i] for p in prots], torch.int32) for i in (1, 3, 4))
        self.ranks = t(ranks, torch.int32)
        self.lens = [len(p[1]) for p in prots]
        self.starts = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.offsets = torch.as_tensor(self.starts).to("cuda", torch.int32)
        self.n, self.T, self.k = len(prots), int(self.starts[-1]), k
        self.min_len = min(self.lens) if min_len is None else min_len
        self.max_len = max(self.lens) if max_len is None else max_len
        self.K = min(k, self.min_len)
        self.slab = torch.cat([v.reshape(-1).float() for v in (sd or _sd()).values()]).cuda()
        self.numel = int(self.lib.tmpnn_seqloss_slab_numel())
        self.saved = torch.empty(self.lib.tmpnn_seqloss_batch_saved_bytes(self.T, self.n, self.K), dtype=torch.uint8, device="cuda")
        self.scratch = torch.empty(self.lib.tmpnn_seqloss_batch_scratch_bytes(self.T, self.n, self.K), dtype=torch.uint8, device="cuda")
        assert self.saved.numel() > 0 and self.scratch.numel() > 0
        self.E_idx = torch.full((self.T, self.K), -1, dtype=torch.int32, device="cuda")
        self.status = torch.full((1,), 77, dtype=torch.int32, device="cuda")         # the entry zeroes it on the stream

    def _head(self):
        from thermompnn_amd.train import _ptr
        return (_ptr(self.X), _ptr(self.S), _ptr(self.mask), _ptr(self.ridx), _ptr(self.cenc), _ptr(self.offsets), self.n, self.T,
                self.min_len, self.max_len, self.k, _ptr(self.ranks), _ptr(self.slab), self.numel)

    def forward(self, p=0.0, seed=0, step=0, keep_in=None, keep_out=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        lp = torch.empty((self.T, 21), dtype=torch.float32, device="cuda")
        check(self.lib.tmpnn_seqloss_batch_forward(*self._head(), p, _ptr(keep_in), _ptr(keep_out), seed, step, _ptr(lp), _ptr(self.E_idx),
                                                   _ptr(self.status), _ptr(self.saved), self.saved.numel(), _stream()),
              "tmpnn_seqloss_batch_forward")
        return lp

    def backward(self, dlp, p=0.0, seed=0, step=0, keep_in=None):
        from thermompnn_amd._lib import check
        from thermompnn_amd.train import _ptr, _stream
        dlp = torch.as_tensor(dlp).to("cuda", torch.float32).contiguous()
        grads = torch.zeros(self.numel, dtype=torch.float32, device="cuda")
        check(self.lib.tmpnn_seqloss_batch_backward(*self._head(), p, _ptr(keep_in), seed, step, _ptr(dlp), _ptr(grads), _ptr(self.saved),
                                                    self.saved.numel(), _ptr(self.scratch), self.scratch.numel(), _stream()),
              "tmpnn_seqloss_batch_backward")
        return grads

    def mask_numel(self):
        return int(self.lib.tmpnn_seqloss_batch_mask_numel(self.T, self.K))

    def rows(self, b):
        return slice(int(self.starts[b]), int(self.starts[b + 1]))


def _member_ranks(name, kind):
    return _ranks(kind, len(_arrays(name)[1]), seed=3 + RAGGED.index(name))


_SINGLE = {}


def _single(name, kind):
    """tmpnn_seqloss_forward on the protein alone at K = 30 -> (log_probs, E_idx), computed once."""
    if (name, kind) not in _SINGLE:
        call = Call(*_arrays(name), _member_ranks(name, kind), K_RAGGED)
        _SINGLE[name, kind] = (call.forward(), call.E_idx.clone())
    return _SINGLE[name, kind]


# ---- 1. every member against its single call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["perm", "ties"])
def test_ragged_members_equal_their_single_calls_in_every_packing_order(kind):
    """log_probs rows and E_idx minus the offset of every member, bit for bit, whatever the order of the three in the pack."""
    for order in itertools.permutations(RAGGED):
        bc = BatchCall([_arrays(n) for n in order], [_member_ranks(n, kind) for n in order], K_RAGGED)
        assert bc.K == K_RAGGED and bc.T == 128
        lp = bc.forward()
        assert int(bc.status.item()) == 0
        for b, name in enumerate(order):
            want_lp, want_E = _single(name, kind)
            assert torch.equal(lp[bc.rows(b)], want_lp), (order, name)
            assert torch.equal(bc.E_idx[bc.rows(b)] - int(bc.starts[b]), want_E), (order, name)


def test_equal_length_pack_of_short_members_runs_at_the_shared_k():
    """2 x 40 rows at k_neighbors = 48: K = 40, the second member is msk_L17 padded with 23 masked tail rows."""
    X, S, mask, _, ridx, cenc = [t.cpu().numpy() for t in _batch(["msk_L40", "msk_L17"])]
    assert float(np.abs(mask[1, 17:]).max()) == 0.0
    prots = [(X[b], S[b], mask[b], ridx[b], cenc[b]) for b in range(2)]
    ranks = [_ranks("perm", 40, seed=11 + b) for b in range(2)]
    bc = BatchCall(prots, ranks, 48)
    assert bc.K == 40 and (bc.min_len, bc.max_len) == (40, 40)
    lp = bc.forward()
    assert int(bc.status.item()) == 0
    for b in range(2):
        call = Call(*prots[b], ranks[b], 48)
        assert call.Keff == 40
        assert torch.equal(lp[bc.rows(b)], call.forward()) and torch.equal(bc.E_idx[bc.rows(b)] - 40 * b, call.E_idx), b


# ---- 2. n_proteins = 1 is the single entry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["msk_L40", "msk_L56_2ch"])
def test_one_protein_batch_equals_the_single_entries_bit_for_bit(name):
    arrays = _arrays(name)
    L = len(arrays[1])
    ranks = _ranks("perm", L)
    dlp = torch.from_numpy(np.random.default_rng(4).normal(size=(L, 21)).astype(np.float32))
    bc, call = BatchCall([arrays], [ranks], 48), Call(*arrays, ranks, 48)
    assert bc.K == call.Keff and bc.mask_numel() == call.mask_numel()
    for kw in (dict(p=0.0), dict(p=0.1, seed=5, step=9)):
        lp_b, lp_s = bc.forward(**kw), call.forward(**kw)
        assert torch.equal(lp_b, lp_s) and torch.equal(bc.E_idx, call.E_idx), kw
        g_b, g_s = bc.backward(dlp, **kw), call.backward(dlp, **kw)
        assert torch.equal(g_b, g_s), kw
        assert float(g_b.abs().max()) > 0.0
    assert not torch.equal(bc.forward(p=0.1, seed=5, step=9), bc.forward())          # the drawn masks did act


# ---- 3. the batch gradient against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,seed", [("xavier", 0), ("hot", 0)])
def test_batch_gradient_matches_the_float64_restatement_summed_over_proteins(style, seed):
    """The ragged batch of test 1 under a random dL/dlog_probs on every row (masked rows carry non-zero values): every tensor of the
    batch gradient within FINETUNE_TOL x max|g| (or 1e-12 on a structural zero) of the sum over proteins of
    tests/seqloss_restatement.py in float64 on the device's graph, at the Xavier draw and at the heavy one (hot, seed 0).

    Worst error / max|g| on the first passing run (MI355X): Xavier 1.40e-6 (encoder_layers.1.norm3.weight; log_probs error 4.5e-6),
    hot 1.95e-6 (features.edge_embedding.weight; log_probs error 1.59e-5). Every run prints its own figures."""
    sd = mpnn_weights(style, seed)
    prots = [_arrays(n) for n in RAGGED]
    ranks = [_member_ranks(n, "perm") for n in RAGGED]
    bc = BatchCall(prots, ranks, K_RAGGED, sd=sd)
    lp = bc.forward()
    dlp = torch.from_numpy(np.random.default_rng(1).normal(size=(bc.T, 21)).astype(np.float32))
    dead = torch.cat([torch.as_tensor(p[2]) for p in prots]) == 0
    assert int(dead.sum()) > 0 and float(dlp[dead].abs().min()) > 0.0
    grads = _split(bc.backward(dlp))
    ref, lp_err = None, 0.0
    for b, (arr, r) in enumerate(zip(prots, ranks)):
        Ei = bc.E_idx[bc.rows(b)].cpu().numpy() - int(bc.starts[b])
        assert ((Ei >= 0) & (Ei < bc.lens[b])).all()
        ref_lp, W = log_probs_f64(sd, *arr, Ei, r, None)
        g = grads_f64(ref_lp, W, dlp[bc.rows(b)])
        lp_err = max(lp_err, float((lp[bc.rows(b)].cpu().double() - ref_lp.detach()).abs().max()))
        ref = g if ref is None else {k: ref[k] + g[k] for k in ref}
    worst = {}
    for k, gt in grads.items():
        gmax, err = float(ref[k].abs().max()), float((gt.cpu().double() - ref[k]).abs().max())
        worst[k] = err / gmax if gmax > 1e-12 else 0.0
    print(f"packed batch {style}{seed}: log_probs error {lp_err:.3g}, worst gradient error / max|g|: {max(worst.values()):.3g}",
          max(worst, key=worst.get))
    for k, gt in grads.items():
        gmax, err = float(ref[k].abs().max()), float((gt.cpu().double() - ref[k]).abs().max())
        assert err <= FINETUNE_TOL * gmax or err <= 1e-12, (k, err, gmax)
    assert float(grads["W_s.weight"].abs().max()) > 0.0 and float(grads["W_out.bias"].abs().max()) > 0.0


# ---- 4. dropout over packed rows -----------------------------------------------------------------------------------------------------
def _site_rows(s, rows, K):
    return rows * K if s < 9 and s % 3 == 2 else rows


def test_dropout_rows_are_the_packed_rows():
    """keep_out replayed as keep_in gives the same bits; the generator restated in numpy on PACKED row numbers is keep_out; each
    member's slice of every site, injected into the single entry at the same K, reproduces the member's log_probs bit for bit."""
    from thermompnn_amd.finetune import mask_offsets
    prots = [_arrays(n) for n in RAGGED]
    ranks = [_member_ranks(n, "perm") for n in RAGGED]
    bc = BatchCall(prots, ranks, K_RAGGED)
    T, K = bc.T, bc.K
    keep_out = torch.full((bc.mask_numel(),), -1.0, device="cuda")
    dlp = torch.from_numpy(np.random.default_rng(2).normal(size=(T, 21)).astype(np.float32))
    lp = bc.forward(p=0.1, seed=7, step=3, keep_out=keep_out)
    g = bc.backward(dlp, p=0.1, seed=7, step=3)
    lp2 = bc.forward(p=0.1, seed=99, step=1, keep_in=keep_out)
    assert torch.equal(lp2, lp) and torch.equal(bc.backward(dlp, p=0.1, seed=99, step=1, keep_in=keep_out), g)
    flat, sites, o = keep_out.cpu().numpy(), [], 0
    for s in range(15):
        n = _site_rows(s, T, K)
        sites.append(flat[o:o + n * 128].reshape(n, 128))
        o += n * 128
        assert np.array_equal(sites[s], numpy_site_mask(7, 3, s, n)), s
    assert o == flat.size and 0.85 < float(flat.mean()) < 0.95
    for b, (arr, r) in enumerate(zip(prots, ranks)):
        L, r0 = bc.lens[b], int(bc.starts[b])
        off = mask_offsets(L)
        single = np.zeros(off[15], np.float32)                               # the single entry lays an edge site out for min(48, L)
        for s in range(15):
            per = K if s < 9 and s % 3 == 2 else 1
            part = sites[s][r0 * per:(r0 + L) * per]
            single[off[s]:off[s] + part.size] = part.reshape(-1)
        call = Call(*arr, r, K_RAGGED)
        assert call.mask_numel() == single.size
        assert torch.equal(call.forward(p=0.1, keep_in=torch.from_numpy(single).cuda()), lp[bc.rows(b)]), RAGGED[b]


# ---- 5. the status word, reruns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len,max_len", [(40, 56), (32, 50)], ids=["shorter-than-promised", "longer-than-promised"])
def test_a_broken_length_promise_sets_the_status_bit_and_the_wrapper_raises(min_len, max_len):
    """Offsets that are valid and inside the buffers ([0, 40, 96, 128]); only [min_len, max_len] is wrong about them."""
    from thermompnn_amd import _lib
    from thermompnn_amd import model_utils as mu
    prots = [_arrays(n) for n in RAGGED]
    ranks = [_member_ranks(n, "perm") for n in RAGGED]
    bc = BatchCall(prots, ranks, K_RAGGED, min_len=min_len, max_len=max_len)
    lp = bc.forward()
    assert int(bc.status.item()) & _lib.STATUS_MAXLEN
    assert lp.shape == (128, 21)
    good = BatchCall(prots, ranks, K_RAGGED)
    good.forward()
    assert int(good.status.item()) == 0
    model = _module(k_neighbors=K_RAGGED).eval()
    params = [p for _, p in model.named_parameters()]
    packed = [[torch.as_tensor(np.asarray(p[i])) for p in prots] for i in range(5)] + [[torch.as_tensor(r) for r in ranks]]
    with pytest.raises(_lib.TmpnnError, match="max_len"):
        mu.sequence_log_probs_batch(mu.SeqPlan(), params, *packed, None, K_RAGGED, 0.0, min_len=min_len, max_len=max_len)
    out = mu.sequence_log_probs_batch(mu.SeqPlan(), params, *packed, None, K_RAGGED, 0.0)           # lists are packed, lengths read off
    assert torch.equal(out.detach(), good.forward())


def test_reruns_and_a_second_backward_keep_their_bits():
    prots = [_arrays(n) for n in RAGGED]
    ranks = [_member_ranks(n, "ties") for n in RAGGED]
    dlp = torch.from_numpy(np.random.default_rng(3).normal(size=(128, 21)).astype(np.float32))
    a, b = BatchCall(prots, ranks, K_RAGGED), BatchCall(prots, ranks, K_RAGGED)
    kw = dict(p=0.1, seed=5, step=9)
    lp_a, g_a = a.forward(**kw), a.backward(dlp, **kw)
    assert torch.equal(a.backward(dlp, **kw), g_a)                          # a second backward over the same saved buffer
    assert torch.equal(b.forward(**kw), lp_a) and torch.equal(b.backward(dlp, **kw), g_a)      # a rerun in other buffers
    assert torch.equal(a.forward(**kw), lp_a) and torch.equal(a.backward(dlp, **kw), g_a)      # ... and in the same ones


# ---- 6. the module ----------------------------------------------------------------------------------------------------------------
def test_packed_module_equals_the_loop_and_fills_every_grad():
    """eval mode, _batch(["msk_L40", "msk_L17"]): forward equal to the loop's bit for bit; the gradients of the summed smoothed loss
    within 2 x FINETUNE_TOL x max|g| of the loop's (each is within FINETUNE_TOL of float64: the triangle inequality)."""
    from thermompnn_amd import model_utils as mu
    model = _module().eval()
    X, S, mask, chain_M, ridx, cenc = _batch(["msk_L40", "msk_L17"])
    randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(9)).cuda()
    grads = {}
    for packed in (False, True):
        model.packed = packed
        model.zero_grad(set_to_none=True)
        lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
        assert lp.shape == (2, 40, 21) and lp.requires_grad
        (mu.loss_smoothed(S, lp, mask * chain_M)[0] * mask * chain_M).sum().backward()
        assert all(p.grad is not None for p in model.parameters())
        grads[packed] = ({k: p.grad.clone() for k, p in model.named_parameters()}, lp.detach())
    assert torch.equal(grads[True][1], grads[False][1])
    worst = 0.0
    for k, want in grads[False][0].items():
        gmax, err = float(want.abs().max()), float((grads[True][0][k] - want).abs().max())
        worst = max(worst, err / gmax if gmax > 1e-12 else 0.0)
        assert err <= 2 * FINETUNE_TOL * gmax or err <= 1e-12, (k, err, gmax)
    print("packed module against the loop, worst gradient distance / max|g|:", worst)
    one = model(X[:1], S[:1], mask[:1], chain_M[:1], ridx[:1], cenc[:1], randn=randn[:1])      # B = 1: the single path
    assert torch.equal(one[0].detach(), grads[False][1][0])
    with torch.no_grad():
        assert not model(X, S, mask, chain_M, ridx, cenc, randn=randn).requires_grad


# ---- 7. the imported reference on a padded batch of two ---------------------------------------------------------------------------
def test_packed_module_matches_the_reference_golden_of_a_padded_batch():
    """tests/golden/make_seqbatch_golden.py: the imported reference in float64 on msk_L40 and msk_L56_2ch padded to 56, k_neighbors
    48, under its own recorded draw. The packed module call is held to the lines of
    test_log_probs_loss_and_gradients_match_the_reference_golden: log_probs within max(1e-5, 2.5 x the reference's own float32
    distance), every gradient of the summed smoothed loss within 1e-4 x max|g|. The fixture's graph lists, among the masked residues
    tied at a row's D_max, the lowest indices (the script says how); the device's graph must be that graph on every live row."""
    from thermompnn_amd import model_utils as mu
    g = load_golden("seqbatch_L40_L56")
    assert list(g["members"]) == ["msk_L40", "msk_L56_2ch"]
    X, S, mask, chain_M, ridx, cenc = _batch(["msk_L40", "msk_L56_2ch"])
    assert X.shape[:2] == (2, 56)
    randn = torch.from_numpy(g["randn"]).cuda()
    host = [t.cpu().numpy() for t in (X, S, mask, ridx, cenc)]
    from thermompnn_amd.protein_mpnn_utils import decoding_ranks
    ranks = decoding_ranks(chain_M * mask, randn).cpu().numpy()
    order = g["decoding_order"]
    assert all(np.array_equal(ranks[b][order[b]], np.arange(56)) for b in range(2))
    bc = BatchCall([tuple(a[b] for a in host) for b in range(2)], [ranks[b] for b in range(2)], 48)
    bc.forward()
    live = mask.cpu().numpy().reshape(-1) > 0
    E_dev = (bc.E_idx.cpu().numpy() - np.repeat(bc.starts[:2], 56)[:, None])
    assert np.array_equal(E_dev[live], g["E_idx"].reshape(112, 48)[live]), "the device's k-NN graph differs from the reference's"
    model = _module().eval()
    model.packed = True
    lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
    line = max(1e-5, HOT_F64_FACTOR * float(g["eval_log_probs_d32"]))
    err = float(np.abs(lp.detach().cpu().numpy() - g["eval_log_probs"]).max())
    loss = mu.loss_smoothed(S, lp, mask * chain_M)[1]
    print("packed module against the reference: log_probs", err, "line", line, "loss", float(loss.detach()), float(g["eval_loss"]))
    assert err <= line
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is not None for v in grads.values())
    worst = check_against_golden(g, "eval", {k: v.cpu() for k, v in grads.items()}, 1e-4)
    print("packed module against the reference: worst gradient distance / max|g|:", worst)
