"""Masked neighbours in unmasked rows and short chains (j < 0 slots), in every form of the inference forward: the layouts of
tests/masked_backbones.py (fewer than 48 unmasked residues each, so every unmasked row lists masked residues; checked on the host by
test_masked_forms_host.py) through the single operators, the fused forward at its three launch bands and the variant decoder, in
fp32, bf16x3 and f16x2, against the CPU oracle on the device's own neighbour graph (torch.topk leaves open which masked residue wins
the D_max tie; the device takes the lower index, DESIGN.md "Ties", pinned by test_gpu_knn_exact.py). No row is left out: ddG, log-probabilities and node states on all rows, per-edge tensors on unmasked rows,
decoder states of masked rows exactly 0. The worst error per (precision, quantity) goes to masked_forms_worst.json in the directory
TMPNN_EVIDENCE_DIR names (default: a temporary directory)."""
import json
import os

import numpy as np
import pytest
import torch

from masked_backbones import LAYOUTS, SEEN, checked_graph, filler, layout_arrays, oracle_trace, pack, protein, variants_of

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for per-edge tensors, node states and log-probabilities
TOL_DDG = 1e-4            # kcal/mol
MOVES = 1e-2              # a substituted masked neighbour must move some unmasked row's ddG by more than this (test_gpu_variants.MOVES)
NAMES = sorted(LAYOUTS)
PRECISIONS = ["fp32", "bf16x3", "f16x2"]
_ENGINES = {}
_SINGLE = {}              # (layout, precision) -> decode_variants of the layout alone
WORST = {}                # "precision/quantity" -> worst |hip - oracle| seen in this session


def engine(precision, K=48):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if (precision, K) not in _ENGINES:
        _ENGINES[precision, K] = Engine(synthetic_state_dict(0), "cuda:0", K, precision=precision, retry_precision=None)
    return _ENGINES[precision, K]


def close(got, want, tol, prec, what):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max()) if np.size(want) else 0.0
    WORST[f"{prec}/{what}"] = max(WORST.get(f"{prec}/{what}", 0.0), err)
    print(f"{prec}/{what}: {err:.3e} (line {tol:g})")
    assert err <= tol, (prec, what, err)


@pytest.fixture(scope="module", autouse=True)
def _evidence(tmp_path_factory):
    yield
    out = os.environ.get("TMPNN_EVIDENCE_DIR") or str(tmp_path_factory.mktemp("masked_forms"))
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.3e}")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "masked_forms_worst.json"), "w") as fh:
            json.dump({"lines": {"intermediate": TOL_INTERMEDIATE, "ddg": TOL_DDG}, "worst_abs_error": WORST}, fh, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- a. the single operators ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_stagewise_vs_oracle(name, precision):
    eng = engine(precision)
    g = protein(name)
    p = pack([g])
    L, valid = len(g["S"]), g["mask"] > 0
    E_idx, D_nb = eng.knn_topk(p["X"], p["mask"], p["offsets"])
    dn = D_nb.cpu().numpy()
    ei, D_adj = checked_graph(name, E_idx.cpu().numpy())
    Keff = ei.shape[1]
    np.testing.assert_allclose(dn[valid, :Keff], np.take_along_axis(D_adj, ei.astype(np.int64), 1)[valid], atol=1e-6, rtol=3e-7)
    assert (np.diff(dn[:, :Keff], axis=1) >= 0).all()                       # ascending like torch.topk
    tr = oracle_trace(name, E_idx=ei)                                       # everything downstream on the SAME graph, slot by slot
    assert np.array_equal(tr["E_idx"], ei)

    h_E, E = eng.edge_featurize(p["X"], p["ridx"], p["cenc"], E_idx, D_nb, want_E=True)
    close(E.cpu().numpy()[valid, :Keff], tr["E"][valid], TOL_INTERMEDIATE, precision, "E")
    close(h_E.cpu().numpy()[valid, :Keff], tr["h_E0"][valid], TOL_INTERMEDIATE, precision, "h_E0")
    assert (h_E.cpu().numpy()[:, Keff:] == 0).all()

    h_V = torch.zeros((L, 128), device="cuda:0")
    for l in range(3):
        eng.enc_layer(l, h_V, h_E, E_idx, p["mask"])
        close(h_V.cpu().numpy(), tr[f"hV_enc{l + 1}"], TOL_INTERMEDIATE, precision, f"hV_enc{l + 1}")
    close(h_E.cpu().numpy()[valid, :Keff], tr["h_E_final"][valid], TOL_INTERMEDIATE, precision, "h_E_final")

    hs = []
    for l in range(3):
        h_V = eng.dec_layer(l, h_V, h_E, E_idx, p["S"], p["mask"])
        hs.append(h_V)
        close(h_V.cpu().numpy(), tr[f"hV_dec{l + 1}"], TOL_INTERMEDIATE, precision, f"hV_dec{l + 1}")
        assert (h_V.cpu().numpy()[~valid] == 0).all()
    np.testing.assert_array_equal(eng.seq_embed(p["S"]).cpu().numpy(), tr["h_S"])
    close(eng.log_probs(hs[2]).cpu().numpy(), tr["log_probs"], TOL_INTERMEDIATE, precision, "log_probs")
    ddg, z = eng.ddg_head(hs[2], hs[1], p["S"], want_z=True)
    close(z.cpu().numpy(), tr["z"], TOL_INTERMEDIATE, precision, "z")
    close(ddg.cpu().numpy(), tr["ddg"], TOL_DDG, precision, "ddg")


# ---- b. the fused forward at its three launch bands -----------------------------------------------------
def fused(eng, prots):
    b = pack(prots)
    r = eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], want_hidden=True, want_log_probs=True,
                        want_E_idx=True)
    return {k: v.cpu().numpy() for k, v in r.items()}, b["starts"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_forward_alone_and_in_both_ragged_bands(precision):
    """A layout alone (T <= CUs: k-NN inside the featurizer launch and the fused edge + message form in f16x2), in a ragged batch with
    CUs < T < 16 CUs (8-wavefront message pass) and in one with T = 16 CUs + r, once inside the first 16 CUs rows (f16x2: the
    wavefront-per-residue message pass) and once in the tail (its 8-wavefront remainder): the same bits everywhere, and the oracle's
    numbers."""
    eng = engine(precision)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lay, fill = [protein(n) for n in NAMES], filler()
    n_lay = sum(len(g["S"]) for g in lay)
    alone = {}
    for name, g in zip(NAMES, lay):
        assert len(g["S"]) <= cus
        r, _ = fused(eng, [g])
        alone[name] = r
        ei, _ = checked_graph(name, r["E_idx"])
        tr = oracle_trace(name, E_idx=ei)
        valid = g["mask"] > 0
        tag = precision + "/fused"
        for l in range(3):
            close(r["hidden"][l], tr[f"hV_dec{l + 1}"], TOL_INTERMEDIATE, tag, f"hV_dec{l + 1}")
        assert (r["hidden"][:, ~valid] == 0).all()
        close(r["log_probs"], tr["log_probs"], TOL_INTERMEDIATE, tag, "log_probs")
        close(r["ddg"], tr["ddg"], TOL_DDG, tag, "ddg")
        assert (r["ddg"][np.arange(len(valid)), g["S"]] == 0).all()

    # middle band: every layout, a filler between any two
    mid = [x for g in lay for x in (g, fill)] + [fill] * max(0, (cus + 64 - n_lay) // 64 - len(lay))
    # large band: [layouts][fillers up to the first protein boundary at or beyond 16 CUs][layouts]; r = T - 16 CUs is
    # (n_lay + 64 n1 - 16 CUs) + n_lay < 64 + 2 n_lay and = 2 n_lay = 6 (mod 8)
    n1 = -(-(16 * cus - n_lay) // 64)
    big = lay + [fill] * n1 + lay
    head, tail = list(range(len(lay))), [len(lay) + n1 + k for k in range(len(lay))]
    for prots, where in ((mid, list(zip(NAMES, range(0, 2 * len(lay), 2)))), (big, list(zip(NAMES, head)) + list(zip(NAMES, tail)))):
        T = sum(len(g["S"]) for g in prots)
        if prots is mid:
            assert cus < T < 16 * cus
        else:
            assert 9 <= T - 16 * cus <= 2047 and (T - 16 * cus) % 8 != 0
        r, starts = fused(eng, prots)
        for name, k in where:
            s, e = int(starts[k]), int(starts[k + 1])
            if prots is big:
                assert e <= 16 * cus if k in head else s >= 16 * cus
            a = alone[name]
            blk = r["E_idx"][s:e]
            assert ((blk == -1) | ((blk >= s) & (blk < e))).all()            # neighbours never cross proteins
            np.testing.assert_array_equal(np.where(blk < 0, -1, blk - s), a["E_idx"], err_msg=f"{name} E_idx rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(r["ddg"][s:e], a["ddg"], err_msg=f"{name} ddg rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(r["hidden"][:, s:e], a["hidden"], err_msg=f"{name} hidden rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(r["log_probs"][s:e], a["log_probs"], err_msg=f"{name} log_probs rows {s}:{e} of T={T}")


# ---- c. the variant decoder ----------------------------------------------------------------------------
def check_variants(name, eng, got, ei, tag):
    """decode_variants of variants_of(name) (arrays [V, ...]) against the oracle on each substituted sequence, on the graph ei."""
    g = protein(name)
    valid, n = g["mask"] > 0, len(g["S"])
    items = list(variants_of(name).items())
    wt = oracle_trace(name, items[0][1], E_idx=ei)["ddg"]
    for v, (vname, S) in enumerate(items):
        tr = oracle_trace(name, S, E_idx=ei)
        for l in range(3):
            close(got["hidden"][v, l], tr[f"hV_dec{l + 1}"], TOL_INTERMEDIATE, tag, f"hV_dec{l + 1}")
        assert (got["hidden"][v][:, ~valid] == 0).all(), vname
        close(got["log_probs"][v], tr["log_probs"], TOL_INTERMEDIATE, tag, "log_probs")
        close(got["ddg"][v], tr["ddg"], TOL_DDG, tag, "ddg")
        assert (got["ddg"][v][np.arange(n), S] == 0).all()                  # relative to the variant's own residue
        if vname in ("seen_masked_substitution", "unmasked_substitution"):
            # the substituted letter reaches UNMASKED rows (at a masked residue: only as a neighbour the decoder keeps), on both sides
            ref_move = float(np.abs(tr["ddg"] - wt)[valid].max())
            dev_move = float(np.abs(got["ddg"][v] - got["ddg"][0])[valid].max())
            print(f"{tag}/{name}/{vname}: unmasked rows move by {ref_move:.4e} (oracle), {dev_move:.4e} (device)")
            assert ref_move > MOVES and dev_move > MOVES, (name, vname, ref_move, dev_move)


def decode_alone(name, precision):
    if (name, precision) not in _SINGLE:
        eng = engine(precision)
        p = pack([protein(name)])
        enc = eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])
        res = eng.decode_variants(enc, np.stack(list(variants_of(name).values())), want_hidden=True, want_log_probs=True)
        _SINGLE[name, precision] = ({k: v.cpu().numpy() for k, v in res.items()}, enc.E_idx.cpu().numpy())
    return _SINGLE[name, precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_variants_vs_oracle_on_the_substituted_sequence(name, precision):
    """msk_L40's seen-residue move is 1.008e-2 on the oracle (masked_backbones.SEEN): the device's own error has to stay below
    7.8e-5 kcal/mol there, inside the 1e-4 line the same test holds it to."""
    got, E_idx = decode_alone(name, precision)
    seen = SEEN[name][0]
    ei, _ = checked_graph(name, E_idx)
    assert any(seen in ei[i] for i in np.nonzero(protein(name)["mask"] > 0)[0])
    check_variants(name, engine(precision), got, ei, precision + "/variants")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_variants_over_a_context_of_all_layouts_have_the_single_protein_bits(precision):
    eng = engine(precision)
    p = pack([protein(n) for n in NAMES])
    enc = eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])
    S = np.concatenate([np.stack(list(variants_of(n).values())) for n in NAMES], axis=1)
    res = {k: v.cpu().numpy() for k, v in eng.decode_variants(enc, S, want_hidden=True, want_log_probs=True).items()}
    ei = enc.E_idx.cpu().numpy()
    for k, name in enumerate(NAMES):
        s, e = int(p["starts"][k]), int(p["starts"][k + 1])
        one, one_ei = decode_alone(name, precision)
        np.testing.assert_array_equal(np.where(ei[s:e] < 0, -1, ei[s:e] - s), one_ei, err_msg=name)
        np.testing.assert_array_equal(res["ddg"][:, s:e], one["ddg"], err_msg=name)
        np.testing.assert_array_equal(res["hidden"][:, :, s:e], one["hidden"], err_msg=name)
        np.testing.assert_array_equal(res["log_probs"][:, s:e], one["log_probs"], err_msg=name)


def test_variants_with_30_neighbours():
    name, eng = "msk_L56", engine("f16x2", 30)
    p = pack([protein(name)])
    enc = eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"])
    res = eng.decode_variants(enc, np.stack(list(variants_of(name).values())), want_hidden=True, want_log_probs=True)
    X, _, mask, _, _ = layout_arrays(name)
    ei = enc.E_idx.cpu().numpy()
    assert (ei[:, 30:] == -1).all() and (ei[:, :30] >= 0).all()
    from oracle import thermompnn_oracle as orc
    D_adj = orc.adjusted_distances(torch.from_numpy(X)[None, :, 1], torch.from_numpy(mask)[None])[0].numpy()
    for i in np.nonzero(mask > 0)[0]:                                       # 46 unmasked residues: no masked neighbour among 30
        assert (D_adj[i, ei[i, :30]] <= np.sort(D_adj[i])[29]).all() and len(set(ei[i, :30].tolist())) == 30
    got = {k: v.cpu().numpy() for k, v in res.items()}
    g = protein(name)
    valid = g["mask"] > 0
    for v, (vname, S) in enumerate(variants_of(name).items()):
        tr = oracle_trace(name, S, E_idx=np.ascontiguousarray(ei[:, :30]))
        for l in range(3):
            close(got["hidden"][v, l], tr[f"hV_dec{l + 1}"], TOL_INTERMEDIATE, "f16x2/variants_K30", f"hV_dec{l + 1}")
        assert (got["hidden"][v][:, ~valid] == 0).all()
        close(got["log_probs"][v], tr["log_probs"], TOL_INTERMEDIATE, "f16x2/variants_K30", "log_probs")
        close(got["ddg"][v], tr["ddg"], TOL_DDG, "f16x2/variants_K30", "ddg")
