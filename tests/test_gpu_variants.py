"""Many sequence variants over one encoded backbone (Engine.encode + Engine.decode_variants, tmpnn_variants.hip) on the GPU:
parity against the CPU oracle evaluated on the SUBSTITUTED sequence, batch invariance, fp32 bit-identity with the fused forward,
a large scan against replicated fused forwards, range handling and the ISA record of the new kernel."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import HOT_F64_FACTOR, REPO, is_hot, load_golden, weights_for_case

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for decoder states and log-probabilities
TOL_DDG = 1e-4            # kcal/mol
MOVES = 1e-2              # a variant's table must differ from the wild type's by more than this somewhere
_ENGINES = {}
_ORACLE = {}


def engine_for(g, precision):
    from thermompnn_amd.engine import Engine
    key = (int(g["weight_seed"]), str(g["weight_style"]) if "weight_style" in g else "xavier", precision)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(weights_for_case(g), "cuda:0", 48, precision=precision, retry_precision=None)
    return _ENGINES[key]


def packed(g, dev="cuda:0"):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    L = len(g["S"])
    return dict(X=t(g["X"], torch.float32), S=t(g["S"], torch.int32), mask=t(g["mask"], torch.float32),
                ridx=t(g["residue_idx"], torch.int32), cenc=t(g["chain_enc"], torch.int32),
                offsets=torch.tensor([0, L], dtype=torch.int32, device=dev), L=L)


def encode(eng, p):
    return eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])


def variants_of(g):
    """name -> sequence: wild type, one substitution, two adjacent ones, a fully redrawn sequence and (where the structure has
    one) a substitution at a residue whose mask is 0."""
    S = g["S"].astype(np.int64)
    L, rng = len(S), np.random.default_rng(7)
    live = np.nonzero(g["mask"] > 0)[0]
    out = {"wild_type": S.copy()}
    one = S.copy()
    p = int(live[len(live) // 2])
    one[p] = (one[p] + 3) % 20
    out["one_substitution"] = one
    two = S.copy()
    q = int(live[len(live) // 3])
    for k in (q, q + 1):
        two[k] = (two[k] + 7) % 20
    out["two_adjacent"] = two
    out["redrawn"] = rng.integers(0, 20, L)
    dead = np.nonzero(g["mask"] == 0)[0]
    if len(dead):
        md = S.copy()
        md[dead[0]] = (md[dead[0]] + 5) % 20
        out["masked_residue"] = md
    return out


def oracle_on(g, S, E_idx, f64=False):
    """The oracle's trace for sequence S on the device's neighbour graph (slot by slot), in fp32 or evaluated in float64. Keyed by
    the sequence too: conftest.oracle_trace_f64 is not, and would hand back the wild type's."""
    from oracle import thermompnn_oracle as orc
    key = (int(g["weight_seed"]), str(g.get("weight_style", "xavier")), g["X"].tobytes()[:4096], S.tobytes(), E_idx.tobytes(), f64)
    if key in _ORACLE:
        return _ORACLE[key]
    t = torch.from_numpy
    dt = torch.float64 if f64 else torch.float32
    orig_float, orig_default = torch.Tensor.float, torch.get_default_dtype()
    if f64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
        torch.set_default_dtype(torch.float64)
    try:
        W = {k: v.to(dt) for k, v in weights_for_case(g).items()}
        X, mask = t(g["X"]).to(dt)[None], t(g["mask"]).to(dt)[None]
        ridx, cenc = t(g["residue_idx"].astype(np.int64))[None], t(g["chain_enc"].astype(np.int64))[None]
        tr = {}
        with torch.no_grad():
            orc.ssm_table(W, X, t(S.astype(np.int64))[None], mask, torch.ones_like(mask), ridx, cenc, 48, trace=tr,
                          E_idx_override=t(np.ascontiguousarray(E_idx).astype(np.int64))[None])
    finally:
        torch.Tensor.float = orig_float
        torch.set_default_dtype(orig_default)
    _ORACLE[key] = {k: v[0].numpy() for k, v in tr.items()}
    return _ORACLE[key]


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("case", ["syn_L32", "2OCJ_A", "2OCJ_A_gap", "2OCJ_AB", "2OCJ_A_w1", "2OCJ_A_hot"])
def test_variants_match_the_oracle_on_the_substituted_sequence(case, precision):
    g = load_golden(case)
    eng = engine_for(g, precision)
    p = packed(g)
    enc = encode(eng, p)
    Keff = min(48, p["L"])
    ei = enc.E_idx.cpu().numpy()[:, :Keff]
    names, seqs = zip(*variants_of(g).items())
    res = eng.decode_variants(enc, np.stack(seqs), want_hidden=True, want_log_probs=True)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    wt_table = oracle_on(g, seqs[0], ei)["ddg"]
    for v, (name, S) in enumerate(zip(names, seqs)):
        tr = oracle_on(g, S, ei)
        pairs = [("ddg", got["ddg"][v], tr["ddg"], TOL_DDG), ("log_probs", got["log_probs"][v], tr["log_probs"], TOL_INTERMEDIATE)]
        pairs += [(f"hV_dec{l + 1}", got["hidden"][v, l], tr[f"hV_dec{l + 1}"], TOL_INTERMEDIATE) for l in range(3)]
        t64 = oracle_on(g, S, ei, f64=True) if is_hot(g) else None
        for what, a, b, tol in pairs:
            if t64 is not None:
                truth = t64[what].astype(np.float64)
                ref_err = float(np.abs(b.astype(np.float64) - truth).max())
                hip_err = float(np.abs(a.astype(np.float64) - truth).max())
                print(f"{case}/{precision}/{name}/{what}: |hip - f64| {hip_err:.3e}, |oracle fp32 - f64| {ref_err:.3e}")
                assert hip_err <= HOT_F64_FACTOR * ref_err, (case, precision, name, what, hip_err, ref_err)
            else:
                err = float(np.abs(a.astype(np.float64) - b).max())
                print(f"{case}/{precision}/{name}/{what}: {err:.3e} (line {tol:g})")
                assert err <= tol, (case, precision, name, what, err)
        if name != "wild_type":      # a decoder that ignored S_var would return the wild type's table
            assert float(np.abs(tr["ddg"] - wt_table).max()) > MOVES and float(np.abs(got["ddg"][v] - got["ddg"][0]).max()) > MOVES, name
        assert (got["ddg"][v][np.arange(len(S)), S] == 0).all()            # relative to the variant's own residue


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3", "fp32"])
def test_a_variant_has_the_same_bits_in_any_batch(precision):
    g = load_golden("2OCJ_A_gap")
    eng = engine_for(g, precision)
    enc = encode(eng, packed(g))
    rng = np.random.default_rng(3)
    S = g["S"].astype(np.int64)
    mine = S.copy()
    mine[[5, 40, 41]] = [(S[5] + 1) % 20, (S[40] + 2) % 20, (S[41] + 9) % 20]
    others = rng.integers(0, 21, (36, len(S)))
    want = dict(want_hidden=True, want_log_probs=True)
    alone = eng.decode_variants(enc, mine[None], **want)
    first = eng.decode_variants(enc, np.concatenate([mine[None], others]), **want)
    last = eng.decode_variants(enc, np.concatenate([others, mine[None]]), **want)
    chunked = eng.decode_variants(enc, np.concatenate([others, mine[None]]), max_rows=len(S), **want)
    for k in ("ddg", "hidden", "log_probs"):
        assert torch.equal(first[k][0], alone[k][0]), k
        assert torch.equal(last[k][36], alone[k][0]), k
        assert torch.equal(chunked[k], last[k]), k


def test_fp32_wild_type_variant_is_the_fused_forward_bit_for_bit():
    names = ["syn_L32", "2OCJ_A_gap", "2OCJ_AB"]
    gs = [load_golden(n) for n in names]
    eng = engine_for(gs[0], "fp32")
    want = dict(want_hidden=True, want_log_probs=True)
    p = packed(gs[1])
    batches = [(p["X"], p["S"], p["mask"], p["ridx"], p["cenc"], p["offsets"])]
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(g[k]) for g in gs])).to("cuda:0", dt)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(g["S"]) for g in gs])]), dtype=torch.int32)
    batches.append((cat("X", torch.float32), cat("S", torch.int32), cat("mask", torch.float32), cat("residue_idx", torch.int32),
                    cat("chain_enc", torch.int32), offsets))
    for X, S, mask, ridx, cenc, off in batches:
        ref = eng.ssm_forward(X, S, mask, ridx, cenc, off, **want)
        enc = eng.encode(X, mask, ridx, cenc, off)
        other = (S + 1) % 20
        res = eng.decode_variants(enc, torch.stack([other, S]), **want)
        assert torch.equal(res["ddg"][1], ref["ddg"]) and torch.equal(res["log_probs"][1], ref["log_probs"])
        assert torch.equal(res["hidden"][1], ref["hidden"])
        ref2 = eng.ssm_forward(X, other, mask, ridx, cenc, off, **want)       # and any other sequence
        assert torch.equal(res["ddg"][0], ref2["ddg"]) and torch.equal(res["hidden"][0], ref2["hidden"])


def test_scan_of_256_variants_against_replicated_fused_forwards(tmp_path):
    """syn_L256, f16x2, V = 256 random single and double substitutions against ssm_forward on the V replicated copies (batches of
    64). Both sides are held to 1e-4 of the same truth, so they may differ by the sum of the two tolerances: 2e-4 (derived, not
    measured). The worst difference is printed and written to variants_vs_fused.json in the directory TMPNN_EVIDENCE_DIR names
    (default: the test's temporary directory), from where a measurement run keeps it."""
    g = load_golden("syn_L256")
    eng = engine_for(g, "f16x2")
    p = packed(g)
    L, V, rng = p["L"], 256, np.random.default_rng(11)
    S = np.tile(g["S"].astype(np.int64), (V, 1))
    for v in range(V):
        for pos in rng.choice(L, 1 + v % 2, replace=False):
            S[v, pos] = (S[v, pos] + rng.integers(1, 20)) % 20
    got = eng.decode_variants(encode(eng, p), S)["ddg"]
    worst = 0.0
    for v0 in range(0, V, 64):
        n = 64
        rep = lambda t: t.repeat(n, *([1] * (t.dim() - 1)))
        off = torch.arange(n + 1, dtype=torch.int32) * L
        ref = eng.ssm_forward(rep(p["X"]), torch.from_numpy(S[v0:v0 + n].reshape(-1)).int(), rep(p["mask"]), rep(p["ridx"]), rep(p["cenc"]),
                              off, max_len=L)["ddg"].view(n, L, 21)
        worst = max(worst, float((got[v0:v0 + n] - ref).abs().max()))
    out = os.environ.get("TMPNN_EVIDENCE_DIR") or str(tmp_path)
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "variants_vs_fused.json"), "w") as fh:
            json.dump({"case": "syn_L256", "precision": "f16x2", "variants": V, "worst_abs_ddg_difference": worst, "bound": 2e-4}, fh)
    except OSError:
        pass
    print(f"worst |decode_variants - replicated ssm_forward| over {V} variants: {worst:.3e}")
    assert worst <= 2e-4


def test_range_overflow_raises_or_retries(synthetic_weights):
    """Weights scaled as test_gpu_parity.test_range_overflow_is_detected_and_retried scales them: the f16x2 decode raises without a
    retry precision; with one it warns and returns the bf16x3 result, bit for bit what a direct bf16x3 call gives."""
    import warnings
    from thermompnn_amd._lib import TmpnnRangeError
    from thermompnn_amd.engine import Engine
    W = {k: v.clone() for k, v in synthetic_weights.items()}
    W["prot_mpnn.features.edge_embedding.weight"] = W["prot_mpnn.features.edge_embedding.weight"] * 1e6
    g = load_golden("syn_L32")
    p = packed(g)
    S = np.stack([g["S"], (g["S"] + 4) % 20]).astype(np.int64)
    direct = Engine(W, "cuda:0", 48, precision="bf16x3", retry_precision=None)
    want = direct.decode_variants(encode(direct, p), S)["ddg"]
    assert bool(torch.isfinite(want).all())
    strict = Engine(W, "cuda:0", 48, precision="f16x2", retry_precision=None)
    with pytest.raises(TmpnnRangeError):
        strict.decode_variants(encode(strict, p), S)
    eng = Engine(W, "cuda:0", 48, precision="f16x2")
    enc = encode(eng, p)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = eng.decode_variants(enc, S)["ddg"]
    assert any("bf16x3" in str(w.message) for w in rec)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_isa_record_lists_the_variant_kernel_without_scratch():
    import glob
    import bench
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_isa_counts.json")), reverse=True)
    d = next(x for x in (json.load(open(f)) for f in files) if x.get("source_stamp") == bench.kernel_source_stamp())
    mine = {n: e for n, e in d["kernels"].items() if "var_msg8_kernel" in n}
    assert any("SplitH2" in n for n in mine) and any("SplitBF3" in n for n in mine), sorted(mine)
    for n, e in mine.items():
        assert int(e.get("scratch_bytes") or 0) == 0, f"{n} spills {e['scratch_bytes']} bytes of scratch"


# ---- TransferModel.variant_tables, double_mutant_table, the command line ------------------------------
class AD(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _model(tmp_path, sd, **head):
    from thermompnn_amd import weights
    from thermompnn_amd.transfer_model import TransferModel
    os.makedirs(tmp_path / "vanilla_model_weights", exist_ok=True)
    weights.save_vanilla_checkpoint(tmp_path / "vanilla_model_weights" / "v_48_020.pt", weights.split_transfer_state_dict(sd)[0], 48)
    cfg = AD(model=AD(subtract_mut=True, freeze_weights=True, load_pretrained=True, **head), platform=AD(thermompnn_dir=str(tmp_path)))
    model = TransferModel(cfg)
    assert not model.load_state_dict(sd).missing_keys
    return model.eval().cuda()


def _substituted(pdb, subs):
    """The parsed structure with its sequence text changed at {position: letter} (chain A only structures)."""
    entry = dict(pdb[0])
    seq = list(entry["seq"])
    for pos, aa in subs.items():
        seq[pos] = aa
    entry["seq"] = entry["seq_chain_A"] = "".join(seq)
    return [entry]


def test_variant_tables_released_head_against_the_oracle(tmp_path, synthetic_weights):
    from oracle import thermompnn_oracle as orc
    from thermompnn_amd.datasets import ALPHABET, Mutation
    from thermompnn_amd.pdb_io import alt_parse_PDB
    model = _model(tmp_path, synthetic_weights, hidden_dims=[64, 32], num_final_layers=2, lightattn=True)
    pdb = alt_parse_PDB(os.path.join(REPO, "tests", "golden", "2OCJ.pdb"), "A")
    seq = pdb[0]["seq"]
    new = "W" if seq[30] != "W" else "A"
    with torch.no_grad():
        got = model.variant_tables(pdb, [seq, [Mutation(30, seq[30], new)]]).cpu().numpy()
    g = load_golden("2OCJ_A")
    t = torch.from_numpy
    S = g["S"].astype(np.int64).copy()
    S[30] = ALPHABET.index(new)
    X, mask = t(g["X"])[None], t(g["mask"])[None]
    with torch.no_grad():
        want = orc.ssm_table(synthetic_weights, X, t(S)[None], mask, torch.ones_like(mask), t(g["residue_idx"].astype(np.int64))[None],
                             t(g["chain_enc"].astype(np.int64))[None], 48)[0].numpy()
    assert got.shape == (2, len(seq), 21)
    assert np.abs(got[1] - want).max() <= TOL_DDG and np.abs(got[0][:, :20] - g["ddg"]).max() <= TOL_DDG
    assert np.abs(got[1] - got[0]).max() > MOVES
    # subtract_mut = False: the un-subtracted head output, as ssm_table gives it for the substituted structure
    model.subtract_mut = False
    with torch.no_grad():
        raw = model.variant_tables(pdb, [[Mutation(30, seq[30], new)]])[0]
        ref = model.ssm_table(_substituted(pdb, {30: new}))
    assert float((raw - ref).abs().max()) <= 2e-4 and float((raw.cpu() - torch.from_numpy(got[1])).abs().max()) > MOVES


def test_variant_tables_with_a_non_default_head(tmp_path):
    """2OCJ_A_headA's configuration runs the generic head over the V L rows. The CPU oracle has the released head only, so the
    reference here is the model's own ssm_table (fused forward + generic head, itself pinned to the imported reference's vectors
    by test_gpu_e2e) on the structure with the substituted sequence: both within 1e-4 of the truth, so 2e-4 apart at most."""
    from thermompnn_amd import weights
    from thermompnn_amd.datasets import Mutation
    from thermompnn_amd.pdb_io import alt_parse_PDB
    g = load_golden("2OCJ_A_headA")
    head = dict(hidden_dims=[int(x) for x in g["hidden_dims"]], num_final_layers=int(g["num_final_layers"]), lightattn=bool(g["lightattn"]))
    model = _model(tmp_path, weights.synthetic_state_dict(int(g["weight_seed"]), head=head), **head)
    assert model.generic_head
    pdb = alt_parse_PDB(os.path.join(REPO, "tests", "golden", "2OCJ.pdb"), "A")
    seq = pdb[0]["seq"]
    subs = {12: "W" if seq[12] != "W" else "A", 13: "G" if seq[13] != "G" else "A"}
    with torch.no_grad():
        got = model.variant_tables(pdb, [seq, [Mutation(p, seq[p], a) for p, a in subs.items()]])
        ref = model.ssm_table(_substituted(pdb, subs))
    assert np.abs(got[0].cpu().numpy()[:, :20] - g["ddg"]).max() <= TOL_DDG
    assert float((got[1] - ref).abs().max()) <= 2e-4 and float((got[1] - got[0]).abs().max()) > MOVES


def test_double_mutant_table_is_two_forwards(tmp_path, synthetic_weights):
    from thermompnn_amd.datasets import ALPHABET, Mutation
    from thermompnn_amd.pdb_io import alt_parse_PDB
    from thermompnn_amd.variant_scan import double_mutant_table
    model = _model(tmp_path, synthetic_weights, hidden_dims=[64, 32], num_final_layers=2, lightattn=True)
    pdb = alt_parse_PDB(os.path.join(REPO, "tests", "golden", "2OCJ.pdb"), "A")
    seq = pdb[0]["seq"]
    positions = [20, 77]
    with torch.no_grad():
        dm = double_mutant_table(model, pdb, positions=positions, chunk=16)
    assert dm.shape == (2, 20, len(seq), 20) and dm.is_cuda
    rng = np.random.default_rng(5)
    for _ in range(6):
        k, a, q, b = int(rng.integers(2)), int(rng.integers(20)), int(rng.integers(len(seq))), int(rng.integers(20))
        p = positions[k]
        if ALPHABET[a] == seq[p] or q == p:
            continue
        bg = _substituted(pdb, {p: ALPHABET[a]})
        with torch.no_grad():
            first = model(pdb, [Mutation(p, seq[p], ALPHABET[a])])[0][0]["ddG"].item()
            second = model(bg, [Mutation(q, bg[0]["seq"][q], ALPHABET[b])])[0][0]["ddG"].item()
        assert abs(dm[k, a, q, b].item() - (first + second)) <= 2e-4, (p, a, q, b)


def test_command_line_writes_the_variant_tables(tmp_path):
    from thermompnn_amd import variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.pdb_io import alt_parse_PDB
    path = os.path.join(REPO, "tests", "golden", "2OCJ.pdb")
    pdb = alt_parse_PDB(path, "A")
    seq = pdb[0]["seq"]
    lines = [f"{seq[9]}10W,{seq[10]}11G", seq, f"{seq[0]}1A"]
    (tmp_path / "variants.txt").write_text("# three variants\n" + "\n".join(lines) + "\n")
    out = tmp_path / "tables.npz"
    assert variant_scan.main([path, "--chain", "A", "--variants", str(tmp_path / "variants.txt"), "--out", str(out),
                              "--synthetic_weights", "0"]) == 0
    with np.load(out) as z:
        tables, names, wt = z["tables"], [str(s) for s in z["variants"]], str(z["wild_type"])
    assert wt == seq and names[1] == seq and names[0][9:11] == "WG" and names[2][0] == "A" and tables.shape == (3, len(seq), 21)
    model = load_model(None, ".", 0)
    with torch.no_grad():
        want = model.variant_tables(pdb, [variant_scan.parse_variant_line(l) for l in lines]).cpu().numpy()
    np.testing.assert_array_equal(tables, want)
