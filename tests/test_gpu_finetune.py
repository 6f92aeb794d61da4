"""Fine-tuning of ProteinMPNN with the head on the MI355X: every gradient against a float64 torch.autograd restatement, the eval-mode
rows against the inference engine, the dropout generator, determinism, AdamW, learning and finetune(cfg) end to end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from masked_backbones import LAYOUTS, write_layout
from train_weight_cases import FINETUNE_WEIGHT_CASES, ft_id

pytestmark = pytest.mark.gpu
AA20 = "ACDEFGHIKLMNPQRSTVWY"
RELEASED = dict(hidden_dims=[64, 32], num_final_layers=2, lightattn=True)
GOLD64 = 0x9E3779B97F4A7C15
SITE_MUL = 0xD6E8FEB86659FD93


def _model(tmp_path, head=None, subtract=True, seed=0, style="xavier"):
    from thermompnn_amd import weights
    from thermompnn_amd.train import Config
    from thermompnn_amd.transfer_model import TransferModel
    head = head or RELEASED
    sd = weights.synthetic_state_dict(seed, style=style, head=head)
    vdir = os.path.join(str(tmp_path), "vanilla_model_weights")
    os.makedirs(vdir, exist_ok=True)
    weights.save_vanilla_checkpoint(os.path.join(vdir, "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    cfg = Config.wrap(dict(model=dict(hidden_dims=list(head["hidden_dims"]), subtract_mut=subtract, num_final_layers=head["num_final_layers"],
                                      freeze_weights=False, load_pretrained=True, lightattn=head["lightattn"]),
                           platform=dict(thermompnn_dir=str(tmp_path))))
    model = TransferModel(cfg)
    model.load_state_dict(sd)
    return model.cuda()


def _pdb(case, tmp_path):
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    if case == "2OCJ_A":
        return alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A"])
    if case == "2OCJ_AB":
        return alt_parse_PDB(os.path.join(GOLDEN, "2OCJ.pdb"), ["A", "B"])
    if case == "2OCJ_A_gap":                       # residue 120 without N (position 24), 150-152 removed (positions 54-56 are '-')
        return alt_parse_PDB(os.path.join(GOLDEN, "2OCJ_gap_chainA.pdb"), ["A"])
    if case in LAYOUTS:
        return alt_parse_PDB(write_layout(case, tmp_path), ["A"])
    L = int(case.split("_L")[1])
    X, seq = synthetic_backbone(L, 5)
    path = os.path.join(str(tmp_path), f"{case}.pdb")
    with open(path, "w") as fh:
        fh.write(backbone_pdb_text(X, seq))
    return alt_parse_PDB(path, ["A"])


def _mutants(pdb, n, seed=0, with_none=True, at=()):
    """n mutants on residues that have a letter ('-' has no wild type), the first quarter on one residue, then one on each of ``at``."""
    from thermompnn_amd.datasets import Mutation
    seq = pdb[0]["seq"]
    rng = np.random.default_rng(seed)
    letters = np.array([i for i, c in enumerate(seq) if c != "-"])
    pos = letters[rng.integers(0, len(letters), n)]
    pos[: n // 4] = pos[0]                          # several mutants share a residue
    pos[n // 4: n // 4 + len(at)] = at
    out = []
    for i, p in enumerate(pos):
        t = None if with_none and i % 17 == 5 else torch.tensor([float(rng.normal())])
        out.append(Mutation(int(p), seq[p], AA20[int(rng.integers(0, 20))], t, "x"))
    return out


def _mix(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def numpy_site_mask(seed, step, site, rows, p=0.1):
    """The documented generator of csrc/tmpnn_finetune.hip, restated: keep = (mix(ks ^ (row << 32 | col)) >> 40) >= round(p 2^24)."""
    with np.errstate(over="ignore"):
        k2 = _mix(_mix(np.uint64(seed) ^ np.uint64(GOLD64)) + np.uint64(step))
        ks = _mix(k2 ^ (np.uint64(SITE_MUL) * np.uint64(site + 1)))
    r = np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(32)
    c = np.arange(128, dtype=np.uint64)[None, :]
    h = _mix(ks ^ (r | c))
    return ((h >> np.uint64(40)) >= np.uint64(round(p * 2 ** 24))).astype(np.float32)


def numpy_head_mask(seed, step, M, D, p=0.25):
    with np.errstate(over="ignore"):
        k2 = _mix(_mix(np.uint64(seed) ^ np.uint64(GOLD64)) + np.uint64(step))
    h = _mix(k2 ^ ((np.arange(M, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(D, dtype=np.uint64)[None, :]))
    return ((h >> np.uint64(40)) >= np.uint64(round(p * 2 ** 24))).astype(np.float32)


def _split_masks(flat, L):
    from thermompnn_amd.finetune import mask_offsets
    off = mask_offsets(L)
    return [flat[off[s]:off[s + 1]].reshape(-1, 128) for s in range(15)]


def restate(sd, names, prot, E_idx, site_mult, head_mult, nf, lightattn, subtract, dtype=torch.float64, upstream=None):
    """float64 torch.autograd restatement of the training forward + loss (oracle layer functions, dropout multipliers given).
    ``dtype`` = torch.float32 evaluates the same mathematics at the device's precision (what fp32 alone costs, test_train_weights_host.py).
    ``upstream`` [M] replaces the loss by sum(pred * upstream): an arbitrary dL/dpred.
    -> (loss, {name: grad}, rows)"""
    from oracle import thermompnn_oracle as O
    W = {k: v.detach().cpu().to(dtype).clone().requires_grad_(k in names) for k, v in sd.items()}
    mp, hd = O.split_weights(W)
    L = prot.L
    K = E_idx.shape[1]
    X = prot.X.cpu().to(dtype)[None]
    mask = prot.mask.cpu().to(dtype)[None]
    ridx, cenc, S = (t.cpu().long()[None] for t in (prot.ridx, prot.cenc, prot.S))
    Ei = torch.from_numpy(E_idx).long()[None]
    atoms = O.backbone_atoms(X)
    D_nb, _ = O.knn(atoms[O.CA], mask, K, Ei)
    blocks = [O.rbf(D_nb)]
    for a, b in O.PAIR_ORDER[1:]:
        D_ab = torch.sqrt(((atoms[a][:, :, None, :] - atoms[b][:, None, :, :]) ** 2).sum(-1) + 1e-6)
        blocks.append(O.rbf(O.gather_edges(D_ab[..., None], Ei)[..., 0]))
    d = O.positional_index(ridx, cenc, Ei)
    E_pos = F.linear(F.one_hot(d, 66).to(dtype), mp["features.embeddings.linear.weight"], mp["features.embeddings.linear.bias"])
    E = F.linear(torch.cat([E_pos] + blocks, -1), mp["features.edge_embedding.weight"])
    hE = O.linear(O.layer_norm(E, mp, "features.norm_edges"), mp, "W_e")
    hV = torch.zeros(1, L, 128, dtype=dtype)
    ma = mask.unsqueeze(-1) * O.gather_nodes(mask.unsqueeze(-1), Ei).squeeze(-1)
    m = [torch.from_numpy(x).to(dtype).view(1, L, -1, 128).squeeze(2) if x.shape[0] == L else torch.from_numpy(x).to(dtype).view(1, L, K, 128)
         for x in site_mult]
    for l in range(3):
        p = f"encoder_layers.{l}"
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), O.cat_neighbors_nodes(hV, hE, Ei)], -1)
        msg = ma.unsqueeze(-1) * O.message(hEV, mp, p)
        hV = O.layer_norm(hV + m[3 * l] * (msg.sum(-2) / 30.0), mp, p + ".norm1")
        hV = O.layer_norm(hV + m[3 * l + 1] * O.ffn(hV, mp, p + ".dense"), mp, p + ".norm2")
        hV = mask.unsqueeze(-1) * hV
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), O.cat_neighbors_nodes(hV, hE, Ei)], -1)
        hE = O.layer_norm(hE + m[3 * l + 2] * O.message(hEV, mp, p, ("W11", "W12", "W13")), mp, p + ".norm3")
    hS = F.embedding(S, mp["W_s.weight"])
    hES = O.cat_neighbors_nodes(hS, hE, Ei)
    hidden = []
    for l in range(3):
        p = f"decoder_layers.{l}"
        hESV = mask.view(1, L, 1, 1) * O.cat_neighbors_nodes(hV, hES, Ei)
        hEV = torch.cat([hV.unsqueeze(-2).expand(-1, -1, K, -1), hESV], -1)
        hV1 = O.layer_norm(hV + m[9 + 2 * l] * (O.message(hEV, mp, p).sum(-2) / 30.0), mp, p + ".norm1")
        hV = mask.unsqueeze(-1) * O.layer_norm(hV1 + m[10 + 2 * l] * O.ffn(hV1, mp, p + ".dense"), mp, p + ".norm2")
        hidden.append(hV)
    hidden = hidden[::-1]
    pos = prot.pos.cpu().long()
    rows = torch.cat([hidden[k][0][pos] for k in range(nf)] + [hS[0][pos]], -1)
    y = rows
    if lightattn:
        y = F.linear(rows, hd["light_attention.feature_convolution.weight"][:, :, 4], hd["light_attention.feature_convolution.bias"])
        if head_mult is not None:
            y = y * torch.from_numpy(head_mult).to(dtype)
    z = y
    for i in range(sum(1 for k in hd if k.startswith("both_out.") and k.endswith(".weight"))):   # [ReLU, Linear] x n (any depth)
        z = O.linear(F.relu(z), hd, f"both_out.{2 * i + 1}")
    zz = z * hd["ddg_out.weight"].view(()) + hd["ddg_out.bias"].view(())
    mut, wt = prot.mut.cpu().long(), prot.wt.cpu().long()
    pred = zz.gather(1, mut[:, None])[:, 0] - (zz.gather(1, wt[:, None])[:, 0] if subtract else 0.0)
    loss = ((pred - prot.target.cpu().to(dtype)) ** 2).mean() if upstream is None else (pred * torch.as_tensor(upstream).cpu().to(dtype)).sum()
    loss.backward()
    grads = {k: (W[k].grad if W[k].grad is not None else torch.zeros_like(W[k])) for k in names}
    return float(loss.detach()), grads, rows.detach()


CASES = [("2OCJ_A", RELEASED, True, True), ("2OCJ_AB", RELEASED, True, False), ("syn_L32", RELEASED, True, True),
         ("syn_L32", dict(hidden_dims=[64, 32], num_final_layers=0, lightattn=True), True, True),
         ("syn_L40", dict(hidden_dims=[48], num_final_layers=1, lightattn=False), True, True),
         ("syn_L32", dict(hidden_dims=[32], num_final_layers=3, lightattn=True), False, True)]
NF0 = dict(hidden_dims=[64, 32], num_final_layers=0, lightattn=True)
# masked residues (mask 0 with a letter, and '-' gaps), chains shorter than a 16-row tile or off the multiples of 4 / 16, K = 48 < L from
# L = 49 on, and ~1900 labelled mutants crowded onto two residues (long mutant-CSR bins, the head core's 16 parts of > 64 rows)
EDGE_CASES = [("2OCJ_A_gap", RELEASED, True, True), ("msk_L40", RELEASED, False, True), ("msk_L40", NF0, True, True),
              ("msk_L56", RELEASED, True, True), ("syn_L2", RELEASED, True, True), ("syn_L3", RELEASED, False, True),
              ("syn_L5", dict(hidden_dims=[48], num_final_layers=1, lightattn=False), True, True), ("syn_L17", NF0, True, True),
              ("syn_L17", RELEASED, True, True), ("syn_L47", dict(hidden_dims=[32], num_final_layers=3, lightattn=True), True, True),
              ("syn_L49", RELEASED, True, True), ("many_L24", RELEASED, True, True)]
# mutants placed on masked residues (a missing N line: mask 0, the letter kept) and next to the gaps
AT = {"2OCJ_A_gap": (24, 24, 53, 57), "msk_L40": (0, 12, 30, 39, 23), "msk_L56": (0, 9, 41, 55, 33)}
GAPPED = ("2OCJ_A_gap", "msk_L40", "msk_L56")


def _case_mutants(case, pdb, n=40, seed=0):
    from thermompnn_amd.datasets import Mutation
    if not case.startswith("many_"):
        return _mutants(pdb, n, seed, at=AT.get(case, ()))
    seq = pdb[0]["seq"]
    rng = np.random.default_rng(seed)
    n = 2000
    pos = np.where(rng.random(n) < 0.9, np.where(rng.random(n) < 0.5, 3, 17), rng.integers(0, len(seq), n))
    return [Mutation(int(p), seq[p], AA20[int(rng.integers(0, 20))], None if i % 17 == 5 else torch.tensor([float(rng.normal())]), "x")
            for i, p in enumerate(pos)]


def _case_id(c):
    return f"{c[0]}-nf{c[1]['num_final_layers']}-la{int(c[1]['lightattn'])}-s{int(c[2])}-d{int(c[3])}"


@pytest.mark.parametrize("case,head,subtract,dropout", CASES + EDGE_CASES,
                         ids=[f"{c[0]}-nf{c[1]['num_final_layers']}-la{int(c[1]['lightattn'])}-d{int(c[3])}" for c in CASES]
                         + [_case_id(c) for c in EDGE_CASES])
def test_every_gradient_matches_a_float64_restatement(tmp_path, case, head, subtract, dropout):
    _every_gradient_matches(tmp_path, case, head, subtract, dropout)


@pytest.mark.parametrize("case,head,subtract,dropout,style,seed", FINETUNE_WEIGHT_CASES, ids=[ft_id(c) for c in FINETUNE_WEIGHT_CASES])
def test_every_gradient_matches_a_float64_restatement_on_heavy_weight_draws(tmp_path, case, head, subtract, dropout, style, seed):
    """The body and every line of test_every_gradient_matches_a_float64_restatement away from the Xavier draw of seed 0: "hot"
    weights (matrices x 3, biases x 5, LayerNorm gamma in [-2, 2]: losses of 1e3 .. 1e4, ReLU heads with dead units, LightAttention
    rows of 1e2), "wide" weights (matrices x 8: losses to 8e7) and a second Xavier seed, mutants on masked residues as before.
    The lines are unchanged because the restatement in float32 alone meets each with a factor of 2.5 to spare on every one of these
    cases (tests/test_train_weights_host.py: gradients 4.7e-7 .. 1.2e-5 of max|g|, loss 2.1e-8 .. 5.1e-7 relative, rows to 3.5e-6).

    First passing run (MI355X), in the order of FINETUNE_WEIGHT_CASES - worst device gradient error / max|g| (the restatement's own
    float32 figure from the host test), loss relative error, rows error: 5.27e-6 (4.92e-6), 5.4e-7, 6.4e-6; 3.42e-6 (2.42e-6), 2.9e-7,
    4.4e-6; wide 1.70e-5 (7.19e-6), 2.6e-7, 4.5e-6; msk_L56 4.69e-6 (3.90e-6), 8.9e-7, 3.9e-6; no hidden states 4.08e-7 (4.68e-7),
    2.1e-8, 0; syn_L17 wide 6.25e-6 (1.21e-5), 5.6e-7, 4.6e-6; xavier 1 2.06e-6 (1.32e-6), 3.6e-7, 2.1e-6. Every run prints its own."""
    _every_gradient_matches(tmp_path, case, head, subtract, dropout, style, seed)


def _every_gradient_matches(tmp_path, case, head, subtract, dropout, style="xavier", seed=0):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path, head, subtract, seed, style)
    tr = MPNNTrainer(model, seed=7)
    pdb = _pdb(case, tmp_path)
    prot = tr.prepare([(pdb, _case_mutants(case, pdb))])[0]
    L, K = prot.L, min(48, prot.L)
    nf, la = head["num_final_layers"], head["lightattn"]
    E_idx = torch.empty((L, K), dtype=torch.int32, device="cuda")
    D0 = 128 * nf + 128
    rows = torch.empty((prot.M, D0), dtype=torch.float32, device="cuda")
    keep_out = torch.empty(tr.mask_numel(L), dtype=torch.float32, device="cuda") if dropout and nf else None
    hkeep = numpy_head_mask(7, 3, prot.M, D0) if dropout and la else None
    loss = tr.forward_backward(prot, keep_out=keep_out, head_keep_in=None if hkeep is None else torch.from_numpy(hkeep).cuda(),
                               p_mpnn=0.1 if dropout else 0.0, p_head=0.25 if hkeep is not None else 0.0, step=3,
                               E_idx_out=E_idx if nf else None, rows_out=rows)
    torch.cuda.synchronize()
    if nf:
        Ei = E_idx.cpu().numpy()
        assert ((Ei >= 0) & (Ei < L)).all()
        _check_neighbour_sets(prot, Ei)
    else:
        from oracle import thermompnn_oracle as O
        X = prot.X.cpu().double()[None]
        Ei = O.knn(O.backbone_atoms(X)[O.CA], prot.mask.cpu().double()[None], K)[1][0].numpy()
    scale = 1.0 / (1.0 - round(0.1 * 2 ** 24) / 2 ** 24)
    if keep_out is not None:
        site_mult = [x * scale for x in _split_masks(keep_out.cpu().numpy(), L)]
    else:
        site_mult = [np.ones((L * (K if s < 9 and s % 3 == 2 else 1), 128), np.float32) for s in range(15)]
    head_mult = None if hkeep is None else hkeep / 0.75
    ref_loss, ref, ref_rows = restate(model.state_dict(), list(tr.shapes), prot, Ei, site_mult, head_mult, nf, la, subtract)
    figures = {k: float((tr.tensor(k, "grad").cpu().double() - r).abs().max()) / float(r.abs().max()) for k, r in ref.items()
               if float(r.abs().max()) > 1e-12}
    print(case, style, seed, f"loss {ref_loss:.4g} rel. error {abs(float(loss) - ref_loss) / max(abs(ref_loss), 1e-3):.3g}, rows error "
          f"{float((rows.cpu().double() - ref_rows).abs().max()):.3g}, worst gradient error / max|g|:", max(figures.values()),
          max(figures, key=figures.get))
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(abs(ref_loss), 1e-3), (float(loss), ref_loss)
    assert torch.allclose(rows.cpu().double(), ref_rows, atol=1e-4, rtol=0)
    for k in tr.shapes:
        g, r = tr.tensor(k, "grad").cpu().double(), ref[k]
        gmax = float(r.abs().max())
        err = float((g - r).abs().max())
        assert err <= 1e-4 * gmax or err <= 1e-12, (k, err, gmax)      # 1e-12: a structural zero the float64 side rounds to ~1e-17
    if case in GAPPED and nf:
        assert int((prot.S == 20).sum()) > 0 and float(prot.mask.min()) == 0.0
        mask = prot.mask.cpu().numpy()
        reached = bool((mask[Ei[mask > 0]] == 0).any())
        g20 = float(ref["prot_mpnn.W_s.weight"][20].abs().max())
        if case == "2OCJ_A_gap":            # 194 residues, 4 masked: no masked residue is among an unmasked row's 48 nearest
            assert not reached and g20 == 0.0
            assert float(tr.tensor("prot_mpnn.W_s.weight", "grad")[20].abs().max()) == 0.0
        else:                               # masked j feed unmasked rows through h_E_ij and h_S_j (W_s[20] at a '-' position)
            assert reached and g20 > 0.0
    if case.startswith("many_"):
        assert prot.M > 1024 and int((prot.pos == 3).sum()) > 400 and int((prot.pos == 17).sum()) > 400


def _check_neighbour_sets(prot, Ei):
    """The device's k-NN on the unmasked rows equals the oracle's, up to exact ties at the K-th adjusted distance (the device takes
    the lower index; torch.topk leaves tie order unspecified). A masked row's candidates all sit at distance 0: the device
    lists 0 .. K-1 (test_gpu_knn_exact.py), torch.topk whatever it likes, and the row reaches nothing, so it is not compared here."""
    from oracle import thermompnn_oracle as O
    from test_gpu_parity import topk_rows_differing
    X, mask = prot.X.cpu()[None], prot.mask.cpu()[None]
    D_adj = O.adjusted_distances(X[:, :, 1], mask)[0].numpy()
    ref = O.knn(X[:, :, 1], mask, Ei.shape[1])[1][0].numpy()
    live = np.flatnonzero(prot.mask.cpu().numpy() > 0)
    topk_rows_differing(Ei, ref, D_adj, live)
    masked = set(np.flatnonzero(prot.mask.cpu().numpy() == 0).tolist())
    if prot.L > Ei.shape[1] and masked and len(live) < Ei.shape[1]:
        # fewer unmasked residues than K: every unmasked row's top K holds masked neighbours, at its D_max
        for i in live:
            nb = [j for j in Ei[i] if j in masked]
            assert nb and all(D_adj[i, j] == D_adj[i].max() for j in nb), i


def test_eval_rows_match_the_engine_and_predictions_match_transfer_model(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    tr = MPNNTrainer(model)
    pdb = _pdb("2OCJ_A", tmp_path)
    muts = _mutants(pdb, 50, with_none=False)
    prot = tr.prepare([(pdb, muts)])[0]
    rows = torch.empty((prot.M, 384), dtype=torch.float32, device="cuda")
    pred = tr.predict_one(prot, rows_out=rows)
    eng = model.engine()
    offs = torch.tensor([0, prot.L], dtype=torch.int32)
    res = eng.ssm_forward(prot.X, prot.S, prot.mask, prot.ridx, prot.cenc, offs, max_len=prot.L, want_ddg=False, want_hidden=True,
                          precision="fp32")
    hid = res["hidden"]
    feat = torch.cat([hid[2], hid[1], eng.seq_embed(prot.S)], dim=1)[prot.pos.long()]
    assert float((rows - feat).abs().max()) <= 1e-5 * max(1.0, float(feat.abs().max()))
    model.precision = "fp32"
    ref = model(pdb, muts)[0]
    ref = torch.stack([r["ddG"][0] for r in ref]).float().cuda()
    assert float((pred - ref).abs().max()) <= 1e-4


def test_in_kernel_dropout_masks_equal_the_numpy_restatement(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    tr = MPNNTrainer(_model(tmp_path), seed=11)
    pdb = _pdb("syn_L64", tmp_path)
    prot = tr.prepare([(pdb, _mutants(pdb, 8))])[0]
    L, K = prot.L, min(48, prot.L)
    keep_out = torch.empty(tr.mask_numel(L), dtype=torch.float32, device="cuda")
    tr.forward_backward(prot, keep_out=keep_out, step=5)
    got = _split_masks(keep_out.cpu().numpy(), L)
    total = kept = 0
    for s in range(15):
        rows = L * K if s < 9 and s % 3 == 2 else L
        want = numpy_site_mask(11, 5, s, rows)
        assert np.array_equal(got[s], want), s
        total += want.size
        kept += want.sum()
    big = numpy_site_mask(11, 5, 2, 8000)                         # >= 10^6 draws of the same generator
    assert big.size >= 10 ** 6 and abs(big.mean() - 0.9) <= 0.002
    assert total >= 10 ** 6 and abs(kept / total - 0.9) <= 0.002    # the kernel's own masks


@pytest.mark.parametrize("head", [RELEASED, dict(hidden_dims=[64, 32], num_final_layers=0, lightattn=True)], ids=["nf2", "nf0"])
def test_three_steps_are_bit_reproducible_and_leave_untouched_tensors_alone(tmp_path, head):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path, head)
    pdb = _pdb("syn_L48", tmp_path)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        tr = MPNNTrainer(model, seed=3, mpnn_learn_rate=1e-3)
        prot = tr.prepare([(pdb, _mutants(pdb, 30))])[0]
        tr.begin_epoch(1)                                       # the loss buffer grows past its size and keeps what it holds
        losses = []
        for _ in range(3):
            tr.grad.zero_()
            tr.step(prot)
            losses.append(tr.epoch_losses()[-1])
        assert np.array_equal(tr.epoch_losses(), np.array(losses, np.float32))
        torch.cuda.synchronize()
        runs.append((tr.slab.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), np.array(losses)))
        tr.write_back()
        sd = model.state_dict()
        assert torch.equal(sd["prot_mpnn.W_out.weight"], start["prot_mpnn.W_out.weight"])
        assert torch.equal(sd["prot_mpnn.W_out.bias"], start["prot_mpnn.W_out.bias"])
        changed = [k for k in sd if not torch.equal(sd[k], start[k])]
        assert "prot_mpnn.W_s.weight" in changed
        if head["num_final_layers"] == 0:
            assert all(not k.startswith("prot_mpnn.") or k == "prot_mpnn.W_s.weight" for k in changed), changed
        else:
            assert "prot_mpnn.encoder_layers.0.W1.weight" in changed and "prot_mpnn.features.embeddings.linear.weight" in changed
        model.load_state_dict(start)
    for a, b in zip(runs[0], runs[1]):
        assert (torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b))


def test_fused_adamw_on_the_finetune_slab_matches_torch(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    tr = MPNNTrainer(model, learn_rate=2e-3, mpnn_learn_rate=3e-4)
    assert tr.lrs["prot_mpnn"] == 3e-4 and tr.lrs["both_out"] == 2e-3
    gen = torch.Generator().manual_seed(0)
    names = list(tr.shapes)
    ref = {k: tr.tensor(k).detach().cpu().clone().requires_grad_(True) for k in names}
    groups = {}
    for k in names:
        groups.setdefault("prot_mpnn" if k.startswith("prot_mpnn.") else k.split(".")[0], []).append(ref[k])
    opt = torch.optim.AdamW([{"params": v, "lr": tr.lrs[g]} for g, v in groups.items()], lr=2e-3)
    for step in range(3):
        grads = {k: torch.randn(ref[k].shape, generator=gen) for k in names}
        for k in names:        # the structurally zero regions of the head (as tmpnn_finetune_step leaves them)
            if k.startswith("light_attention.attention_convolution") or k == "ddg_out.bias":
                grads[k].zero_()
            elif k == "light_attention.feature_convolution.weight":
                g = torch.zeros_like(grads[k])
                g[:, :, 4] = grads[k][:, :, 4]
                grads[k] = g
        for k in names:
            tr.tensor(k, "grad").copy_(grads[k].cuda())
            ref[k].grad = grads[k].clone()
        tr.adamw()
        opt.step()
    for k in names:
        got, want = tr.tensor(k).cpu(), ref[k].detach()
        assert torch.allclose(got, want, atol=1e-6, rtol=1e-5), k


def test_training_loss_falls_over_twenty_steps_without_dropout(tmp_path):
    from thermompnn_amd.finetune import MPNNTrainer
    model = _model(tmp_path)
    tr = MPNNTrainer(model, seed=1, learn_rate=1e-3, mpnn_learn_rate=1e-4, p_mpnn=0.0, p_head=0.0)
    pdb = _pdb("syn_L56", tmp_path)
    prot = tr.prepare([(pdb, _mutants(pdb, 60, with_none=False))])[0]
    tr.begin_epoch(20)
    for _ in range(20):
        tr.step(prot)
    losses = tr.epoch_losses()
    assert losses[-1] < 0.5 * losses[0], losses


def _write_megascale(tmp_path, n_prot=3):
    import pickle
    from thermompnn_amd.synthetic import backbone_pdb_text, synthetic_backbone
    pdbs = tmp_path / "pdbs"
    pdbs.mkdir()
    rng = np.random.default_rng(0)
    names = []
    with open(tmp_path / "mega.csv", "w") as fh:
        fh.write("name,ddG_ML,mut_type,WT_name,aa_seq,dG_ML,extra\n")
        for p in range(n_prot):
            L = 40 + 8 * p
            X, seq = synthetic_backbone(L, p)
            name = f"prot{p}|A.pdb"
            names.append(name)
            (pdbs / f"prot{p}:A.pdb").write_text(backbone_pdb_text(X, seq))
            fh.write(f"x,0.0,wt,{name},{seq},1.0,z\n")
            for _ in range(12):
                i = int(rng.integers(0, L))
                a = AA20[int(rng.integers(0, 20))]
                if a == seq[i]:
                    continue
                fh.write(f"x,{rng.normal():.3f},{seq[i]}{i + 1}{a},{name},{seq[:i] + a + seq[i + 1:]},1.0,z\n")
    with open(tmp_path / "splits.pkl", "wb") as fh:
        pickle.dump({"train": names, "val": names, "test": []}, fh)
    return pdbs


def test_finetune_end_to_end_writes_a_checkpoint_that_reloads(tmp_path):
    from thermompnn_amd import weights
    from thermompnn_amd.finetune import finetune
    from thermompnn_amd.thermompnn_benchmarking import get_trained_model
    from thermompnn_amd.train import Config
    pdbs = _write_megascale(tmp_path)
    sd = weights.synthetic_state_dict(0)
    vdir = tmp_path / "vanilla_model_weights"
    vdir.mkdir()
    weights.save_vanilla_checkpoint(str(vdir / "v_48_020.pt"), weights.split_transfer_state_dict(sd)[0], 48)
    cfg = Config.wrap(dict(datasets=["megascale"], platform=dict(thermompnn_dir=str(tmp_path)),
                           data_loc=dict(megascale_csv=str(tmp_path / "mega.csv"), megascale_splits=str(tmp_path / "splits.pkl"),
                                         megascale_pdbs=str(pdbs)),
                           training=dict(learn_rate=1e-3, mpnn_learn_rate=1e-4, epochs=2, checkpoint_dir=str(tmp_path / "ck")),
                           model=dict(hidden_dims=[64, 32], subtract_mut=True, num_final_layers=2, freeze_weights=False,
                                      load_pretrained=True, lightattn=True)))
    res = finetune(cfg, log=lambda s: None)
    assert len(res["history"]) == 2 and res["best_checkpoint"] and os.path.exists(res["best_checkpoint"])
    ck = torch.load(res["best_checkpoint"], map_location="cpu", weights_only=True)["state_dict"]
    moved = [k for k, v in sd.items() if k.startswith("prot_mpnn.") and not k.startswith("prot_mpnn.W_out")
             and not torch.equal(ck["model." + k].float(), v.float())]
    assert len(moved) > 100
    model = get_trained_model(res["best_checkpoint"], cfg, override_custom=True).cuda()
    tr = res["trainer"]
    from thermompnn_amd.pdb_io import alt_parse_PDB
    pdb = alt_parse_PDB(str(pdbs / "prot0:A.pdb"), ["A"])
    muts = _mutants(pdb, 20, with_none=False)
    best = torch.load(res["best_checkpoint"], map_location="cpu", weights_only=True)["state_dict"]
    for k in tr.shapes:                                           # the trainer at the best epoch's weights
        tr.tensor(k).copy_(best["model." + k].cuda())
    pred = tr.predict_one(tr.prepare([(pdb, muts)])[0]).cpu()
    model.precision = "fp32"
    table = model.ssm_table(pdb).cpu()
    from thermompnn_amd.datasets import ALPHABET
    want = torch.tensor([float(table[m.position, ALPHABET.index(m.mutation)]) for m in muts])
    assert float((pred - want).abs().max()) <= 1e-4


def _golden_sample_index(name, n, k=2048):
    """tests/golden/make_finetune_golden.py: sample_index."""
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + n)
    return np.sort(rng.choice(n, k, replace=False)), rng.choice([-1.0, 1.0], n)


@pytest.mark.parametrize("golden,src", [("finetune_2OCJ_A", "2OCJ.pdb"), ("finetune_2OCJ_A_gap", "2OCJ_gap_chainA.pdb"),
                                        ("finetune_2OCJ_A_hot", "2OCJ.pdb")], ids=["2OCJ_A", "2OCJ_A_gap", "2OCJ_A_hot"])
def test_loss_and_gradients_match_the_reference_golden(tmp_path, golden, src):
    """The imported reference in float64 (tests/golden/make_finetune_golden.py), all-ones and generator-drawn dropout masks. On the
    gapped chain the reference also settles how mask_attend / mask_bw enter the gradients (the kernel and restate() share one reading).

    2OCJ_A_hot is 2OCJ_A from the heavy weight draw (hot, seed 2; the drawn masks only; loss 8682). The fixture records the imported
    reference's own float32 distance from its float64 result: loss 1.4e-7 relative, worst gradient 3.3e-6 of max|g|; both are inside
    the unchanged lines (1e-6 relative, 1e-4 x max|g|) divided by 2.5, so the lines hold as they are. First passing run (MI355X):
    loss 2.6e-8 relative."""
    from conftest import load_golden
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.finetune import MPNNTrainer
    from thermompnn_amd.pdb_io import alt_parse_PDB
    g = load_golden(golden)
    pdb = alt_parse_PDB(os.path.join(GOLDEN, src), ["A"])
    muts = [Mutation(int(p), AA20[w], AA20[m], None if np.isnan(t) else torch.tensor([float(t)]), "2OCJ")
            for p, w, m, t in zip(g["positions"], g["wildtype"], g["mutation"], g["targets"])]
    style = str(g["weight_style"]) if "weight_style" in g else "xavier"
    tr = MPNNTrainer(_model(tmp_path, seed=int(g["weight_seed"]), style=style), seed=int(g["seed"]))
    prot = tr.prepare([(pdb, muts)])[0]
    L, K = prot.L, min(48, prot.L)
    assert prot.M == int(np.isfinite(g["targets"]).sum())
    if golden.endswith("_gap"):
        assert 24 in g["positions"] and float(prot.mask[24]) == 0.0 and pdb[0]["seq"][54:57] == "---"
    drawn = np.concatenate([numpy_site_mask(int(g["seed"]), int(g["step"]), s, L * K if s < 9 and s % 3 == 2 else L).reshape(-1)
                            for s in range(15)])
    for tag in [t for t in ("ones", "drawn") if f"{t}_loss" in g]:
        tr.grad.zero_()
        E_idx = torch.empty((L, K), dtype=torch.int32, device="cuda")
        kw = dict(keep_in=torch.from_numpy(drawn).cuda(), p_mpnn=0.1) if tag == "drawn" else dict(p_mpnn=0.0)
        loss = tr.forward_backward(prot, p_head=0.0, step=int(g["step"]), E_idx_out=E_idx, **kw)
        live = prot.mask.cpu().numpy() > 0           # a masked row's order in the REFERENCE's graph is torch.topk's choice; it does not reach the loss
        assert np.array_equal(E_idx.cpu().numpy()[live], g["E_idx"][live]), "the device's k-NN graph differs from the reference's"
        ref_loss = float(g[f"{tag}_loss"])
        print(golden, tag, "loss", float(loss), "reference", ref_loss, "relative error", abs(float(loss) - ref_loss) / abs(ref_loss))
        assert abs(float(loss) - ref_loss) <= 1e-6 * abs(ref_loss), (tag, float(loss), ref_loss)
        for name in tr.shapes:
            dev = tr.tensor(name, "grad").reshape(-1).double().cpu().numpy()
            if f"{tag}|{name}|full" in g:
                ref = g[f"{tag}|{name}|full"].astype(np.float64)
                gmax = float(np.abs(ref).max())
                assert float(np.abs(dev - ref).max()) <= 1e-4 * gmax or float(np.abs(dev - ref).max()) <= 1e-12, (tag, name)
            else:
                idx, sign = _golden_sample_index(name, dev.size)
                gmax = float(g[f"{tag}|{name}|absmax"])
                assert abs(float(np.abs(dev).max()) - gmax) <= 1e-4 * gmax, (tag, name)
                assert float(np.abs(dev[idx] - g[f"{tag}|{name}|val"]).max()) <= 1e-4 * gmax, (tag, name)
                sumsq = float(g[f"{tag}|{name}|sumsq"])
                assert abs(float((dev * dev).sum()) - sumsq) <= 1e-4 * sumsq + 1e-20, (tag, name)
                assert abs(float((dev * sign).sum()) - float(g[f"{tag}|{name}|dot"])) <= 1e-4 * np.sqrt(dev.size * sumsq) + 1e-12, (tag, name)
