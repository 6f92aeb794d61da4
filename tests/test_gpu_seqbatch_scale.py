"""The packed sequence loss (tmpnn_seqloss_batch_forward / _backward, ProteinMPNN.packed) past the sizes of test_gpu_seqbatch.py, on
the branches that file never takes: 260 members in one pack (sq_segments_kernel's second trip, binary searches over 260 segments,
ft_csr_scan_kernel with 13 bins per thread), more than 16 384 edge rows (ft_wgrad's FT_MAX_PARTS blocks of more than 64 rows with empty
last blocks, ft_class_sum's 64 blocks) under the order-masked decoder, a ragged pack at K = 48, row counts off every tile size
(T = 85, K = 17, boundaries at odd rows), offsets that do not ascend (the even split of sq_segments_kernel), and the module on a
padded batch of five. The reference throughout is the float64 restatement tests/seqloss_restatement.py, evaluated per member on the
device's own graph and summed over the members.

NOT covered here, so that the gap stays visible: T near the 65 536 rows the header allows, and L above 16 384 (where ft_parts and
ft_cparts cap on NODE rows). `saved` is 0.8 MB per residue at K = 48, which makes neither a seconds-long test nor a cheap float64
reference. The C-alpha flavour has no training entries."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from lattice_backbones import backbone
from masked_backbones import layout_arrays
from seqloss_restatement import grads_f64, log_probs_f64
from test_gpu_finetune import numpy_site_mask
from test_gpu_seqbatch import BatchCall, _arrays
from test_gpu_seqloss import FINETUNE_TOL, SCALE, Call, _batch, _module, _ranks, _split
from tiny_backbones import many_short, tiny_member
from train_weight_cases import HOT_F64_FACTOR, mpnn_weights

pytestmark = pytest.mark.gpu

_WEIGHTS = {}


def _weights(style, seed):
    if (style, seed) not in _WEIGHTS:
        _WEIGHTS[style, seed] = mpnn_weights(style, seed)
    return _WEIGHTS[style, seed]


class Singles:
    """tmpnn_seqloss_forward on many proteins through ONE Call per length, its input tensors refilled for each protein: the weight
    slab is uploaded once per length, not once per protein."""

    def __init__(self, k, sd):
        self.k, self.sd, self.calls = k, sd, {}

    def call(self, arrays, ranks):
        L = len(arrays[1])
        if L not in self.calls:
            self.calls[L] = Call(*arrays, ranks, self.k, sd=self.sd)
        c = self.calls[L]
        for dst, src in zip((c.X, c.S, c.mask, c.ridx, c.cenc, c.ranks), (*arrays, ranks)):
            dst.copy_(torch.as_tensor(np.asarray(src)))
        return c


def _summed_reference(bc, sd, prots, ranks, dlp, lp, mults=None, fp32=False):
    """The float64 restatement of every member on the device's graph (E_idx minus the member's offset) -> (its gradients summed over
    the members, the largest |device log_probs - float64|, and with ``fp32`` what the SAME restatement in float32 is away from
    float64: (log_probs distance, {name: gradient distance}), which is what entitles a hot draw to a line of its own)."""
    E_dev, lp_dev = bc.E_idx.cpu().numpy(), lp.cpu().double()
    ref, ref32, lp_err, lp32 = None, None, 0.0, 0.0
    for b, (arr, r) in enumerate(zip(prots, ranks)):
        rows = bc.rows(b)
        Ei = E_dev[rows] - int(bc.starts[b])
        assert ((Ei >= 0) & (Ei < bc.lens[b])).all(), b
        m = None if mults is None else mults[b]
        ref_lp, W = log_probs_f64(sd, *arr, Ei, r, m)
        g = grads_f64(ref_lp, W, dlp[rows])
        ref_lp = ref_lp.detach()
        lp_err = max(lp_err, float((lp_dev[rows] - ref_lp).abs().max()))
        ref = g if ref is None else {k: ref[k] + g[k] for k in ref}
        if fp32:
            lp_s, W_s = log_probs_f64(sd, *arr, Ei, r, m, dtype=torch.float32)
            g_s = grads_f64(lp_s, W_s, dlp[rows])
            lp32 = max(lp32, float((lp_s.detach().double() - ref_lp).abs().max()))
            ref32 = {k: v.double() for k, v in g_s.items()} if ref32 is None else {k: ref32[k] + g_s[k].double() for k in ref32}
    d32 = {k: float((ref32[k] - ref[k]).abs().max()) for k in ref} if fp32 else None
    return ref, lp_err, (lp32, d32)


def _check_gradients(tag, grads, ref, lp_err, lp_line=1e-5, d32=None):
    """Prints the worst figures, then: log_probs within ``lp_line``; every tensor within FINETUNE_TOL x max|g| (or 1e-12 on a structural
    zero), a hot draw within max(that, HOT_F64_FACTOR x the float32 restatement's own distance ``d32``)."""
    worst = {}
    for k, gt in grads.items():
        gmax, err = float(ref[k].abs().max()), float((gt.cpu().double() - ref[k]).abs().max())
        worst[k] = err / gmax if gmax > 1e-12 else 0.0
    name = max(worst, key=worst.get)
    print(f"{tag}: log_probs error {lp_err:.3g} (line {lp_line:.3g}), worst gradient error / max|g|: {worst[name]:.3g} {name}")
    assert lp_err <= lp_line, (lp_err, lp_line)
    for k, gt in grads.items():
        gmax, err = float(ref[k].abs().max()), float((gt.cpu().double() - ref[k]).abs().max())
        line = FINETUNE_TOL * gmax if d32 is None else max(FINETUNE_TOL * gmax, HOT_F64_FACTOR * d32[k])
        assert err <= line or err <= 1e-12, (k, err, gmax)
    assert float(grads["W_s.weight"].abs().max()) > 0.0 and float(grads["W_out.bias"].abs().max()) > 0.0


def _dlp(T, seed, prots):
    """A random dL/dlog_probs on every row; the masked rows carry non-zero values."""
    dlp = torch.from_numpy(np.random.default_rng(seed).normal(size=(T, 21)).astype(np.float32))
    dead = torch.cat([torch.as_tensor(np.asarray(p[2])) for p in prots]) == 0
    assert int(dead.sum()) > 0 and float(dlp[dead].abs().min()) > 0.0
    return dlp


def _sites(flat, T, K):
    """The batch's flat keep_out -> its 15 sites [rows, 128] (T rows a node site, T K an edge site, no tail)."""
    out, o = [], 0
    for s in range(15):
        n = T * K if s < 9 and s % 3 == 2 else T
        out.append(flat[o:o + n * 128].reshape(n, 128))
        o += n * 128
    assert o == flat.size
    return out


def _member_sites(sites, bc, b):
    """Member b's rows of every site (packed rows r0 .. r0 + L of a node site, r0 K .. (r0 + L) K of an edge site)."""
    r0, r1 = int(bc.starts[b]), int(bc.starts[b + 1])
    per = [bc.K if s < 9 and s % 3 == 2 else 1 for s in range(15)]
    return [sites[s][r0 * per[s]:r1 * per[s]] for s in range(15)]


# ---- 1. 260 short proteins: n > 256, E > 16 384, odd boundaries -----------------------------------------------------------------------
K_SHORT = 8
_PACK = {}


def _pack260():
    """The pack, its BatchCall and its log_probs / E_idx without dropout, made once. Every test runs its own forward before a backward:
    another test may have refilled ``saved`` in between."""
    if not _PACK:
        sd = _weights("xavier", 0)
        prots = many_short()
        ranks = [_ranks("perm", len(p[1]), seed=3 + b) for b, p in enumerate(prots)]
        bc = BatchCall(prots, ranks, K_SHORT, sd=sd)
        assert (bc.n, bc.T, bc.K, bc.min_len, bc.max_len) == (260, 3120, 8, 8, 16) and sum(L % 2 for L in bc.lens) == 116
        # the branches this pack is for: sq_segments_kernel's loops take a second trip, ft_parts / ft_cparts are capped on the edge
        # rows, ft_csr_scan_kernel sums several bins per thread, member boundaries sit at odd rows
        assert bc.n > 256 and bc.T * bc.K > 16384 and bc.T > 256 and any(int(s) % 2 for s in bc.starts[1:-1])
        lp = bc.forward()
        assert int(bc.status.item()) == 0
        _PACK.update(sd=sd, prots=prots, ranks=ranks, bc=bc, lp=lp.clone(), E_idx=bc.E_idx.clone(), dlp=_dlp(bc.T, 1, prots))
    return _PACK


def test_all_260_members_equal_their_single_calls():
    """log_probs rows and E_idx minus the offset of each of the 260 members, bit for bit tmpnn_seqloss_forward on it alone at K = 8."""
    p = _pack260()
    bc, singles = p["bc"], Singles(K_SHORT, p["sd"])
    for b in range(bc.n):
        call = singles.call(p["prots"][b], p["ranks"][b])
        assert call.Keff == K_SHORT
        assert torch.equal(p["lp"][bc.rows(b)], call.forward()), b
        assert torch.equal(p["E_idx"][bc.rows(b)] - int(bc.starts[b]), call.E_idx), b


def test_260_member_gradient_matches_the_float64_restatement_summed_over_members():
    """T = 3 120 packed rows, E = 24 960 edge rows: ft_wgrad runs FT_MAX_PARTS = 256 blocks of 100 rows over the edge rows (the last
    six are empty) with the decoder's order-masked segments, ft_class_sum its 64 blocks of 390. Random dL/dlog_probs on every row,
    masked rows included. Every tensor within FINETUNE_TOL x max|g| (or 1e-12 on a structural zero) of the float64 restatement summed
    over the 260 members on the device's graph, log_probs within 1e-5: the project's lines, which the restatement in float32 meets
    on these members with 1.5e-6 x max|g| (encoder_layers.0.norm1.weight) and 4.2e-6 (CPU, on an argsort k-NN graph).

    First passing run (MI355X): worst gradient error / max|g| 1.86e-6 (encoder_layers.0.norm1.weight), log_probs error 4.36e-6. Every
    run prints its own figures."""
    p = _pack260()
    bc = p["bc"]
    lp = bc.forward()
    assert torch.equal(lp, p["lp"])
    grads = _split(bc.backward(p["dlp"]))
    ref, lp_err, _ = _summed_reference(bc, p["sd"], p["prots"], p["ranks"], p["dlp"], lp)
    _check_gradients("260 members", grads, ref, lp_err)


def test_260_member_reruns_and_a_second_backward_keep_their_bits():
    p = _pack260()
    bc = p["bc"]
    assert torch.equal(bc.forward(), p["lp"])
    g = bc.backward(p["dlp"])
    assert torch.equal(bc.backward(p["dlp"]), g)                             # a second backward over the same saved buffer
    fresh = BatchCall(p["prots"], p["ranks"], K_SHORT, sd=p["sd"])
    assert torch.equal(fresh.forward(), p["lp"]) and torch.equal(fresh.E_idx, p["E_idx"])
    assert torch.equal(fresh.backward(p["dlp"]), g)                          # a rerun in other buffers
    assert float(g.abs().max()) > 0.0


# ---- 2. dropout numbering over 3 120 packed rows --------------------------------------------------------------------------------------
def test_dropout_rows_are_numbered_over_3120_packed_rows():
    """keep_out of the 260-member pack: its size, the documented generator on PACKED rows at a node site, an edge site (row = i K + k)
    and the last site, the keep rate, the replay under another key, and three members' slices of all 15 sites injected into the
    single entry (which lays an edge site out for min(48, L) neighbours: the K = 8 rows go to the start of each part)."""
    from thermompnn_amd.finetune import mask_offsets
    p = _pack260()
    bc = p["bc"]
    T, K = bc.T, bc.K
    assert bc.mask_numel() == (12 * T + 3 * T * K) * 128
    keep_out = torch.full((bc.mask_numel(),), -1.0, device="cuda")
    lp = bc.forward(p=0.1, seed=7, step=3, keep_out=keep_out)
    g = bc.backward(p["dlp"], p=0.1, seed=7, step=3)
    assert not torch.equal(lp, p["lp"])                                      # the drawn masks did act
    assert torch.equal(bc.forward(p=0.1, seed=99, step=1, keep_in=keep_out), lp)
    assert torch.equal(bc.backward(p["dlp"], p=0.1, seed=99, step=1, keep_in=keep_out), g)
    flat = keep_out.cpu().numpy()
    assert set(np.unique(flat).tolist()) <= {0.0, 1.0} and 0.85 < float(flat.mean()) < 0.95
    sites = _sites(flat, T, K)
    for s in (0, 5, 14):
        assert np.array_equal(sites[s], numpy_site_mask(7, 3, s, sites[s].shape[0])), s
    singles = Singles(K_SHORT, p["sd"])
    beyond = next(b for b in range(bc.n) if bc.starts[b] > 256 and bc.lens[b] % 2)
    for b in (0, beyond, bc.n - 1):
        off = mask_offsets(bc.lens[b])
        single = np.zeros(off[15], np.float32)
        for s, part in enumerate(_member_sites(sites, bc, b)):
            single[off[s]:off[s] + part.size] = part.reshape(-1)
        call = singles.call(p["prots"][b], p["ranks"][b])
        assert call.mask_numel() == single.size
        assert torch.equal(call.forward(p=0.1, keep_in=torch.from_numpy(single).cuda()), lp[bc.rows(b)]), b


# ---- 3. a ragged pack at k_neighbors = 48 with E > 16 384 -----------------------------------------------------------------------------
def _chain(chains):
    from thermompnn_amd.pdb_io import alt_parse_PDB, tied_featurize
    pdb = alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), chains)
    f = tied_featurize([pdb[0]], "cpu", None, None, None, None, None, None, ca_only=False)
    return tuple(t.numpy() for t in (f[0][0], f[1][0], f[2][0], f[12][0], f[5][0]))     # X, S, mask, residue_idx, chain_enc


def _ragged48():
    g = backbone("lat_L49m")
    return [_chain(["A"]), _arrays("msk_L56_2ch"), _chain(["B"]), tuple(np.asarray(g[k]) for k in ("X", "S", "mask", "ridx", "cenc"))]


@pytest.mark.parametrize("style,seed", [("xavier", 0), ("hot", 0)])
def test_ragged_pack_at_k48_past_the_row_block_cap(style, seed):
    """2OCJ chain A, msk_L56_2ch, 2OCJ chain B, lat_L49m: 493 rows, boundaries at 194, 250 and 444, K = 48, E = 23 664 (256 weight-
    gradient blocks of 96 rows, the last nine empty), with a two-chain member, masked members and one of L = K + 1. Every member's
    log_probs and E_idx are its single call's bit for bit; the batch gradient is held to FINETUNE_TOL x max|g| and log_probs to 1e-5
    against the float64 restatement summed over the members, at the hot draw to max(that line, HOT_F64_FACTOR x the float32
    restatement's own distance from float64 on this case), computed here from the restatement alone (for orientation, on an argsort
    k-NN graph: log_probs 2.8e-6 / 1.42e-5, gradients 1.3e-6 / 1.9e-6 x max|g| at Xavier / hot).

    First passing run (MI355X): Xavier 1.57e-6 x max|g| (features.norm_edges.weight), log_probs error 2.77e-6; hot 2.34e-6 x max|g|
    (encoder_layers.1.norm1.weight), log_probs error 1.75e-5 against a line of 3.04e-5 (the float32 restatement: 1.22e-5). Every run
    prints its own figures."""
    sd = _weights(style, seed)
    prots = _ragged48()
    ranks = [_ranks("perm", len(p[1]), seed=3 + b) for b, p in enumerate(prots)]
    bc = BatchCall(prots, ranks, 48, sd=sd)
    assert bc.lens == [194, 56, 194, 49] and list(bc.starts) == [0, 194, 250, 444, 493] and bc.K == 48
    assert bc.T * bc.K == 23664 > 16384 and bc.T > 256
    lp = bc.forward()
    assert int(bc.status.item()) == 0
    for b, (arr, r) in enumerate(zip(prots, ranks)):
        call = Call(*arr, r, 48, sd=sd)
        assert torch.equal(lp[bc.rows(b)], call.forward()), b
        assert torch.equal(bc.E_idx[bc.rows(b)] - int(bc.starts[b]), call.E_idx), b
    dlp = _dlp(bc.T, 1, prots)
    grads = _split(bc.backward(dlp))
    hot = style == "hot"
    ref, lp_err, (lp32, d32) = _summed_reference(bc, sd, prots, ranks, dlp, lp, fp32=hot)
    if hot:
        print(f"ragged K = 48 {style}{seed}: the float32 restatement is {lp32:.3g} (log_probs) from float64")
    _check_gradients(f"ragged K = 48 {style}{seed}", grads, ref, lp_err, max(1e-5, HOT_F64_FACTOR * lp32) if hot else 1e-5, d32)


def test_one_protein_of_388_residues_past_the_row_block_cap():
    """2OCJ chains A + B alone (L = 388, two chains, E = 18 624) through tmpnn_seqloss_forward / _backward under a random order: the
    order-masked decoder's backward past the 16 384-row cap in the n = 1 form, held to 1e-5 and FINETUNE_TOL x max|g| against the
    float64 restatement (the restatement in float32: 2.3e-6 and 1.6e-6 x max|g|).

    First passing run (MI355X): worst gradient error / max|g| 1.12e-6 (encoder_layers.2.W1.bias), log_probs error 3.09e-6. Every run
    prints its own figures."""
    sd = _weights("xavier", 0)
    arrays = _chain(["A", "B"])
    L = len(arrays[1])
    assert L == 388 and L * 48 > 16384 and len(set(arrays[4].tolist())) == 2
    ranks = _ranks("perm", L)
    call = Call(*arrays, ranks, 48, sd=sd)
    lp = call.forward()
    dlp = torch.from_numpy(np.random.default_rng(1).normal(size=(L, 21)).astype(np.float32))
    grads = _split(call.backward(dlp))
    Ei = call.E_idx.cpu().numpy()
    assert ((Ei >= 0) & (Ei < L)).all()
    ref_lp, W = log_probs_f64(sd, *arrays, Ei, ranks, None)
    ref = grads_f64(ref_lp, W, dlp)
    _check_gradients("2OCJ_AB alone", grads, ref, float((lp.cpu().double() - ref_lp.detach()).abs().max()))


# ---- 4. row counts off every tile size ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "p0.1"])
def test_five_members_of_17_rows_off_every_tile_size(dropout):
    """msk_L17 and four synthetic backbones of 17 residues (two with a masked residue) at k_neighbors = 48: K = 17, T = 85, member
    boundaries at 17, 34, 51 and 68, edge rows i 17 + k - nothing is a multiple of the 16-row tiles or of ft_wgrad's groups of 4.
    Every member's log_probs and E_idx are its single call's bit for bit (without dropout); the batch gradient within FINETUNE_TOL x
    max|g| and log_probs within 1e-5 of the float64 restatement summed over the members, which with dropout takes the drawn masks
    (keep_out) x SCALE.

    First passing run (MI355X): without dropout 9.53e-7 x max|g| (features.embeddings.linear.weight), log_probs error 3.82e-6; with
    dropout 1.02e-6 x max|g| (encoder_layers.1.dense.W_in.bias), log_probs error 3.63e-6. Every run prints its own figures."""
    sd = _weights("xavier", 0)
    prots = [_arrays("msk_L17"), tiny_member(17, 21), tiny_member(17, 22, masked=5), tiny_member(17, 23), tiny_member(17, 24, masked=16)]
    ranks = [_ranks("perm", 17, seed=3 + b) for b in range(5)]
    bc = BatchCall(prots, ranks, 48, sd=sd)
    assert (bc.K, bc.T, bc.min_len, bc.max_len) == (17, 85, 17, 17) and list(bc.starts) == [0, 17, 34, 51, 68, 85]
    kw = dict(p=0.1, seed=7, step=3) if dropout else {}
    keep_out = torch.full((bc.mask_numel(),), -1.0, device="cuda") if dropout else None
    lp = bc.forward(keep_out=keep_out, **kw)
    assert int(bc.status.item()) == 0
    mults = None
    if dropout:
        flat = keep_out.cpu().numpy()
        assert set(np.unique(flat).tolist()) <= {0.0, 1.0}
        sites = _sites(flat, bc.T, bc.K)
        for s in range(15):
            assert np.array_equal(sites[s], numpy_site_mask(7, 3, s, sites[s].shape[0])), s
        mults = [[m * SCALE for m in _member_sites(sites, bc, b)] for b in range(5)]
    else:
        for b, (arr, r) in enumerate(zip(prots, ranks)):
            call = Call(*arr, r, 48, sd=sd)
            assert call.Keff == 17
            assert torch.equal(lp[bc.rows(b)], call.forward()), b
            assert torch.equal(bc.E_idx[bc.rows(b)] - 17 * b, call.E_idx), b
    dlp = _dlp(bc.T, 1, prots)
    grads = _split(bc.backward(dlp, **kw))
    ref, lp_err, _ = _summed_reference(bc, sd, prots, ranks, dlp, lp, mults=mults)
    _check_gradients(f"5 x 17 rows, dropout {int(dropout)}", grads, ref, lp_err)


# ---- 5. offsets that do not ascend: the status bit, no lingering state ----------------------------------------------------------------
@pytest.mark.parametrize("offsets", [[0, 96, 40, 128], [8, 40, 96, 128], [0, 40, 96, 120]],
                         ids=["descending", "first-not-0", "last-not-T"])
def test_offsets_that_do_not_ascend_set_the_status_bit_and_leave_no_state(offsets):
    """msk_L40, msk_L56_2ch, lat32 at k_neighbors = 16 under the true [min_len, max_len] = [32, 56] and offsets whose values all lie in
    [0, T] but break the promise: sq_segments_kernel falls back to the even split [0, 56, 112, 128] (every segment still holds K = 16
    rows), the entry returns 0 with TMPNN_STATUS_MAXLEN, the wrapper raises, and the next call with the right offsets in the SAME
    saved / scratch buffers gives the bits of a call in fresh ones."""
    from thermompnn_amd import _lib
    from thermompnn_amd import model_utils as mu
    names = ("msk_L40", "msk_L56_2ch", "lat32")
    prots = [_arrays(n) for n in names]
    ranks = [_ranks("perm", len(p[1]), seed=3 + b) for b, p in enumerate(prots)]
    bc = BatchCall(prots, ranks, 16)
    assert (bc.T, bc.K, bc.min_len, bc.max_len) == (128, 16, 32, 56) and all(0 <= o <= bc.T for o in offsets)
    right = bc.offsets
    bc.offsets = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    lp = bc.forward()                                                        # (_lib.check raises on any return code but 0)
    assert int(bc.status.item()) & _lib.STATUS_MAXLEN
    assert lp.shape == (128, 21)
    model = _module(k_neighbors=16).eval()
    params = [p for _, p in model.named_parameters()]
    packed = [torch.cat([torch.as_tensor(np.asarray(p[i])) for p in prots]) for i in range(5)] + [torch.cat([torch.as_tensor(r) for r in ranks])]
    with pytest.raises(_lib.TmpnnError, match="max_len"):
        mu.sequence_log_probs_batch(mu.SeqPlan(), params, *packed, offsets, 16, 0.0, min_len=32, max_len=56)
    dlp = torch.from_numpy(np.random.default_rng(5).normal(size=(128, 21)).astype(np.float32))
    bc.offsets = right
    lp = bc.forward()
    assert int(bc.status.item()) == 0
    g = bc.backward(dlp)
    fresh = BatchCall(prots, ranks, 16)
    assert torch.equal(fresh.forward(), lp) and int(fresh.status.item()) == 0
    assert torch.equal(fresh.backward(dlp), g) and float(g.abs().max()) > 0.0
    out = mu.sequence_log_probs_batch(mu.SeqPlan(), params, *packed, [int(s) for s in bc.starts], 16, 0.0, min_len=32, max_len=56)
    assert torch.equal(out.detach(), lp)


# ---- 6. the module on a padded batch of five ------------------------------------------------------------------------------------------
def test_packed_module_equals_the_loop_on_a_padded_batch_of_five():
    """eval mode, five layouts of 17, 56, 40, 47 and 49 residues padded to 56: the packed forward is the loop's bit for bit, every
    gradient of the summed smoothed loss within 2 x FINETUNE_TOL x max|g| of the loop's (the rule of
    test_packed_module_equals_the_loop_and_fills_every_grad)."""
    from thermompnn_amd import model_utils as mu
    model = _module().eval()
    names = ["msk_L17", "msk_L56_2ch", "msk_L40", "msk_L47", "msk_L49"]
    X, S, mask, chain_M, ridx, cenc = _batch(names)
    assert X.shape[:2] == (5, 56) and [len(layout_arrays(n)[1]) for n in names] == [17, 56, 40, 47, 49]
    randn = torch.randn(chain_M.shape, generator=torch.Generator().manual_seed(9)).cuda()
    grads = {}
    for packed in (False, True):
        model.packed = packed
        model.zero_grad(set_to_none=True)
        lp = model(X, S, mask, chain_M, ridx, cenc, randn=randn)
        assert lp.shape == (5, 56, 21) and lp.requires_grad
        (mu.loss_smoothed(S, lp, mask * chain_M)[0] * mask * chain_M).sum().backward()
        assert all(p.grad is not None for p in model.parameters())
        grads[packed] = ({k: p.grad.clone() for k, p in model.named_parameters()}, lp.detach())
    assert torch.equal(grads[True][1], grads[False][1])
    worst = 0.0
    for k, want in grads[False][0].items():
        gmax, err = float(want.abs().max()), float((grads[True][0][k] - want).abs().max())
        worst = max(worst, err / gmax if gmax > 1e-12 else 0.0)
        assert err <= 2 * FINETUNE_TOL * gmax or err <= 1e-12, (k, err, gmax)
    assert float(grads[True][0]["W_s.weight"].abs().max()) > 0.0
    print("packed module of five against the loop, worst gradient distance / max|g|:", worst)
