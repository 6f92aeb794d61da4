"""Order-masked decoding (Engine.decode_ordered, ProteinMPNN.conditional_probs / unconditional_probs) on the forms the golden
structures do not reach: the masked layouts of tests/masked_backbones.py, where an unmasked row lists masked residues (a visible one
contributes its sequence term and a zero decoder state, an invisible one its encoder state: the reference masks by the row), one
visible slot at a time (which bit of the visibility word steers which gather), K = 30, a packed context of several proteins, the
variant chunk of a workgroup, and the ddG head on order-masked states. fp32, bf16x3 and f16x2 against the torch restatement
(tests/ordered_restatement.py, pinned to the imported reference on masked layouts by test_ordered_host.py) on the device's own
neighbour graph. No row is left out: hidden, log_probs and ddg on all rows, decoder states of masked rows exactly 0. The worst error
per precision/test/quantity and the smallest margins go to ordered_forms_worst.json in the directory TMPNN_EVIDENCE_DIR names
(default: a temporary directory)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from masked_backbones import LAYOUTS, SEEN, checked_graph, filler, pack, protein, variants_of
from ordered_restatement import conditional_ranks, ordered_decode

pytestmark = pytest.mark.gpu

TOL_INTERMEDIATE = 1e-5   # abs; the project's line for decoder states and log-probabilities
TOL_DDG = 1e-4            # kcal/mol
ORDER_MOVES = 1e-3        # 100 x the line: what a visible neighbour must move
SLOTS_APART = 1e-4        # 10 x the line: two different visible slots in the first decoder state of the row
NAMES = sorted(LAYOUTS)
PRECISIONS = ["fp32", "bf16x3", "f16x2"]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
_ENGINES, _MODELS, _RESTATED, _ALONE = {}, {}, {}, {}
WORST = {}                # "precision/test/quantity" -> worst |hip - restatement| seen in this session
MARGINS = {}              # "test/kind" -> smallest move / pairwise distance seen on the device's graphs (restatement and device)


def engine(precision, K=48):
    from thermompnn_amd.engine import Engine
    from thermompnn_amd.weights import synthetic_state_dict
    if (precision, K) not in _ENGINES:
        _ENGINES[precision, K] = Engine(synthetic_state_dict(0), "cuda:0", K, precision=precision, retry_precision=None)
    return _ENGINES[precision, K]


def weights():
    from thermompnn_amd.weights import synthetic_state_dict
    return synthetic_state_dict(0)


def structure(name):
    """-> (pack()'s protein dict, the restatement's fixture dict) of a masked layout, the filler ("filler") or a golden case."""
    if name in LAYOUTS:
        p = protein(name)
    elif name == "filler":
        p = filler()
    else:
        g = load_golden(name)
        p = dict(X=g["X"], S=g["S"].astype(np.int64), mask=g["mask"], ridx=g["residue_idx"].astype(np.int64),
                 cenc=g["chain_enc"].astype(np.int64))
    return p, dict(X=p["X"], S=p["S"], mask=p["mask"], residue_idx=p["ridx"], chain_enc=p["cenc"])


def sequences_of(name):
    """variants_of(name) for a layout; for an unmasked structure the same five kinds with ``seen`` = its middle residue."""
    if name in LAYOUTS:
        return variants_of(name), SEEN[name][0]
    S = structure(name)[0]["S"]
    L, seen = len(S), len(S) // 2
    out = {"wild_type": S.copy()}
    for key, pos, letter in (("unmasked_substitution", L // 3, (S[L // 3] + 3) % 20), ("seen_masked_substitution", seen, (S[seen] + 7) % 20),
                             ("gap_and_letter_swapped", L // 4, 20)):
        out[key] = S.copy()
        out[key][pos] = letter
    out["redrawn"] = np.random.default_rng(7).integers(0, 21, L)
    return out, seen


def int32_spread(L, rng):
    """A permutation's ranks spread over the whole int32 range: L distinct values, INT32_MIN and INT32_MAX among them."""
    vals = np.round(np.linspace(I32_MIN, I32_MAX, L)).astype(np.int64) if L > 1 else np.array([I32_MIN], np.int64)
    assert len(set(vals.tolist())) == L and (L < 2 or (vals[0] == I32_MIN and vals[-1] == I32_MAX and (vals < 0).any()))
    return vals[rng.permutation(L)]


def ranks_of(mask, seen):
    """name -> rank [L] int64: the eight orders of this file."""
    L, rng = len(mask), np.random.default_rng(17)
    seen_first = np.ones(L, np.int64)
    seen_first[seen] = 0
    return {"left_to_right": np.arange(L), "reversed": np.arange(L)[::-1].copy(), "permutation": rng.permutation(L),
            "all_equal": np.zeros(L, np.int64), "two_level": (np.arange(L) >= L // 2).astype(np.int64),
            "masked_first": (mask > 0).astype(np.int64),      # every masked residue is visible to every unmasked one
            "seen_first": seen_first, "int32_range": int32_spread(L, rng)}


# (rank, sequence): V = 16. Pairs 0..5 carry the conditions that keep the comparison from passing vacuously.
PAIRS = [("all_equal", "wild_type"), ("all_equal", "seen_masked_substitution"), ("masked_first", "wild_type"),
         ("masked_first", "seen_masked_substitution"), ("seen_first", "wild_type"), ("seen_first", "seen_masked_substitution"),
         ("left_to_right", "unmasked_substitution"), ("left_to_right", "redrawn"), ("reversed", "gap_and_letter_swapped"),
         ("reversed", "wild_type"), ("permutation", "redrawn"), ("permutation", "seen_masked_substitution"),
         ("two_level", "gap_and_letter_swapped"), ("two_level", "unmasked_substitution"), ("int32_range", "redrawn"),
         ("int32_range", "wild_type")]


def paired(name):
    """-> (sequences [16, L], ranks [16, L]) of PAIRS for a structure."""
    p, _ = structure(name)
    seqs, seen = sequences_of(name)
    ranks = ranks_of(p["mask"], seen)
    return np.stack([seqs[s] for _, s in PAIRS]).astype(np.int64), np.stack([ranks[r] for r, _ in PAIRS]).astype(np.int64)


def restated(name, seqs, ranks, ei):
    """ordered_decode of a structure on the graph ei, cached (the three precisions share the device's graph); callers leave the
    arrays unchanged."""
    key = (name, seqs.tobytes(), ranks.tobytes(), np.ascontiguousarray(ei).astype(np.int64).tobytes())
    if key not in _RESTATED:
        _RESTATED[key] = ordered_decode(weights(), structure(name)[1], seqs, ranks, ei)
    return _RESTATED[key]


def encode(eng, prots):
    p = pack(prots)
    return eng.encode(p["X"], p["mask"], p["ridx"], p["cenc"], p["offsets"]), p


def decode(eng, enc, seqs, ranks, **kw):
    res = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True, want_log_probs=True, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def close(got, want, tol, tag, what):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max()) if np.size(want) else 0.0
    WORST[f"{tag}/{what}"] = max(WORST.get(f"{tag}/{what}", 0.0), err)
    print(f"{tag}/{what}: {err:.3e} (line {tol:g})")
    assert err <= tol, (tag, what, err)


def margin(key, value, bar):
    MARGINS[key] = min(MARGINS.get(key, np.inf), float(value))
    print(f"{key}: {value:.3e} (bar {bar:g})")
    assert value > bar, (key, value, bar)


def within_the_lines(got, ref, seqs, mask, tag):
    """Every variant, every row: hidden and log_probs at 1e-5, ddg at 1e-4, masked rows' states exactly 0, ddg 0 at the own letter."""
    V, L = seqs.shape
    assert got["hidden"].shape == (V, 3, L, 128) and got["log_probs"].shape == (V, L, 21) and got["ddg"].shape == (V, L, 21)
    close(got["hidden"], ref["hidden"], TOL_INTERMEDIATE, tag, "hidden")
    close(got["log_probs"], ref["log_probs"], TOL_INTERMEDIATE, tag, "log_probs")
    close(got["ddg"], ref["ddg"], TOL_DDG, tag, "ddg")
    assert (got["hidden"][:, :, mask == 0] == 0).all()
    assert (got["ddg"][np.arange(V)[:, None], np.arange(L), seqs] == 0).all()


@pytest.fixture(scope="module", autouse=True)
def _evidence(tmp_path_factory):
    yield
    out = os.environ.get("TMPNN_EVIDENCE_DIR") or str(tmp_path_factory.mktemp("ordered_forms"))
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.3e}")
    for k in sorted(MARGINS):
        print(f"smallest {k}: {MARGINS[k]:.3e}")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ordered_forms_worst.json"), "w") as fh:
            json.dump({"lines": {"intermediate": TOL_INTERMEDIATE, "ddg": TOL_DDG, "order_moves": ORDER_MOVES, "slots_apart": SLOTS_APART},
                       "worst_abs_error": WORST, "smallest_margin": MARGINS}, fh, indent=1, sort_keys=True)
    except OSError:
        pass


def orders_move(ref, got, live, tag):
    """PAIRS 0..5 on the unmasked rows ``live``: masked-first against all-equal, the seen residue's letter under seen-first, and
    no letter at all under the all-equal order — on the restatement and on the device."""
    for who, r in (("restatement", ref), ("device", got)):
        margin(f"{tag}/masked_first_vs_all_equal/{who}", np.abs(r["log_probs"][2] - r["log_probs"][0])[live].max(), ORDER_MOVES)
        margin(f"{tag}/seen_first_letter/{who}", np.abs(r["log_probs"][5] - r["log_probs"][4])[live].max(), ORDER_MOVES)
        assert np.array_equal(r["hidden"][0], r["hidden"][1]) and np.array_equal(r["log_probs"][0], r["log_probs"][1]), who


# ---- a. every masked layout under orders ------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_masked_layouts_under_orders(name, precision):
    eng = engine(precision)
    p, _ = structure(name)
    enc, _ = encode(eng, [p])
    ei, _ = checked_graph(name, enc.E_idx.cpu().numpy())        # every unmasked row lists a masked residue
    live = p["mask"] > 0
    assert any(SEEN[name][0] in ei[i] for i in np.nonzero(live)[0])
    seqs, ranks = paired(name)
    res = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True, want_log_probs=True)
    assert torch.equal(res["hidden"][0], res["hidden"][1]) and torch.equal(res["log_probs"][0], res["log_probs"][1])
    got = {k: v.cpu().numpy() for k, v in res.items()}
    ref = restated(name, seqs, ranks, ei)
    within_the_lines(got, ref, seqs, p["mask"], f"{precision}/orders")
    orders_move(ref, got, live, "orders")


# ---- b. one visible slot at a time ------------------------------------------------------------------------
def one_slot_ranks(ei, i):
    """[49, L]: variant k < 48 makes the residue in slot k of row i the only one of rank 0 (all others 1); variant 48: all equal."""
    L = ei.shape[0]
    ranks = np.ones((49, L), np.int64)
    ranks[np.arange(48), ei[i]] = 0
    return ranks


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["msk_L49", "msk_L56", "msk_L56_2ch"])
def test_one_visible_slot_at_a_time(name, precision):
    """Row i* under 48 orders that each make one of its slots visible: every slot moves the row, every two slots move it apart (a
    gather steered by another slot's bit cannot land inside the line), and the self slot leaves it where the all-equal order has it.
    With n unmasked residues (45 in msk_L49, 46 in msk_L56 / msk_L56_2ch) slots 0..n-2 of these rows hold the nearer unmasked
    residues and slots n-1..47 the row's D_max tie — the farthest unmasked residue and the masked ones, lowest index first — so at
    least 48 - n of those last slots (3 resp. 2) hold masked residues: visible, they add their sequence term; invisible, nothing
    but the edge."""
    eng = engine(precision)
    p, _ = structure(name)
    enc, _ = encode(eng, [p])
    ei, _ = checked_graph(name, enc.E_idx.cpu().numpy())
    L, live = len(p["S"]), np.nonzero(p["mask"] > 0)[0]
    assert ei.shape == (L, 48)
    seqs = np.tile(p["S"], (49, 1))
    for i in (int(live[0]), int(live[len(live) // 2]), int(live[-1])):
        n = len(live)           # slots n-1..47: the tie at D_max among the farthest unmasked residue and every masked one
        assert ei[i, 0] == i and (p["mask"][ei[i, :n - 1]] == 1).all() and (p["mask"][ei[i, n - 1:]] == 0).sum() >= 48 - n >= 2
        ranks = one_slot_ranks(ei, i)
        res = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True, want_log_probs=True)
        for k in ("hidden", "log_probs", "ddg"):                  # the self slot: row i* sees nobody, as under the all-equal order
            row = res[k][:, :, i] if k == "hidden" else res[k][:, i]
            assert torch.equal(row[0], row[48]), (name, i, k)
        got = {k: v.cpu().numpy() for k, v in res.items()}
        ref = restated(name, seqs, ranks, ei)
        within_the_lines(got, ref, seqs, p["mask"], f"{precision}/one_slot")
        for who, r in (("restatement", ref), ("device", got)):
            move = np.abs(r["log_probs"][1:48, i] - r["log_probs"][48, i]).max(1)
            print(f"{name}/i*={i}/{who}: slot moves {np.array2string(move, precision=2)}")
            margin(f"one_slot/move/{who}", move.min(), ORDER_MOVES)
            margin(f"one_slot/move_slots_31_32_47/{who}", move[[30, 31, 46]].min(), ORDER_MOVES)
            first = r["hidden"][:48, 0, i].astype(np.float64)         # the first decoder state of row i*, one per visible slot
            apart = np.abs(first[:, None] - first[None]).max(-1) + np.diag(np.full(48, np.inf))
            margin(f"one_slot/pairwise/{who}", apart.min(), SLOTS_APART)


# ---- c. K = 30 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["msk_L56", "syn_L32"])
def test_30_neighbours_under_orders(name, precision):
    """K = 30: slots 30..47 are empty and their visibility bits dead. The same call gives the same bits after an engine with
    K = 48 has decoded more variants on the device (no stale visibility word, no stale slot-V row in a shared workspace)."""
    from oracle import thermompnn_oracle as orc
    eng = engine(precision, 30)
    p, _ = structure(name)
    enc, _ = encode(eng, [p])
    full = enc.E_idx.cpu().numpy()
    L = len(p["S"])
    assert full.shape == (L, 48) and (full[:, 30:] == -1).all() and (full[:, :30] >= 0).all() and (full[:, :30] < L).all()
    ei = np.ascontiguousarray(full[:, :30])
    D_adj = orc.adjusted_distances(torch.from_numpy(p["X"])[None, :, 1], torch.from_numpy(p["mask"])[None])[0].numpy()
    for i in np.nonzero(p["mask"] > 0)[0]:
        assert (D_adj[i, ei[i]] <= np.sort(D_adj[i])[29]).all() and len(set(ei[i].tolist())) == 30, f"row {i}"
    seqs, ranks = paired(name)
    first = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True, want_log_probs=True)
    got = {k: v.cpu().numpy() for k, v in first.items()}
    ref = restated(name, seqs, ranks, ei)
    within_the_lines(got, ref, seqs, p["mask"], f"{precision}/K30")
    for who, r in (("restatement", ref), ("device", got)):
        margin(f"K30/reversed_vs_all_equal/{who}", np.abs(r["log_probs"][9] - r["log_probs"][0]).max(), ORDER_MOVES)
        assert np.array_equal(r["hidden"][0], r["hidden"][1]) and np.array_equal(r["log_probs"][0], r["log_probs"][1]), who
    wide = engine(precision, 48)
    enc48, _ = encode(wide, [p])
    rng = np.random.default_rng(5)
    decode(wide, enc48, rng.integers(0, 21, (24, L)), np.stack([rng.permutation(L)[::-1] for _ in range(24)]))
    again = eng.decode_ordered(enc, seqs, ranks, want_ddg=True, want_hidden=True, want_log_probs=True)
    for k in first:
        assert torch.equal(first[k], again[k]), k


# ---- d. a context of several proteins -----------------------------------------------------------------------
def context_inputs(names):
    """9 variants over a packed context: per protein the five kinds of sequences_of and four redrawn ones, and ONE permutation of
    the whole packed axis per variant as ranks (values of different proteins interleave). -> (seqs [9, T], ranks [9, T])."""
    rng = np.random.default_rng(23)
    seqs = []
    for n in names:
        five = np.stack(list(sequences_of(n)[0].values()))
        seqs.append(np.concatenate([five, rng.integers(0, 21, (4, five.shape[1]))]))
    seqs = np.concatenate(seqs, axis=1).astype(np.int64)
    return seqs, np.stack([rng.permutation(seqs.shape[1]) for _ in range(9)]).astype(np.int64)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_context_of_all_layouts_has_the_single_protein_bits(precision):
    """All seven layouts, an L = 64 filler between any two, as one packed batch, at T < 4 CUs (the variant axis is cut into chunks)
    and padded to T >= 4 CUs + 9, T % 8 != 0 (all variants of a residue in one workgroup; fp32: its large-launch message kernel).
    Every protein's rows, the fillers' and with them the last rows of the packed axis included, have the bits of its decode alone
    under the same rank values, and in the first batch those are within the lines."""
    eng = engine(precision)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    small = [x for n in NAMES for x in (n, "filler")][:-1]
    T0 = sum(len(structure(n)[0]["S"]) for n in small)
    pad = -(-(4 * cus + 9 - T0) // 64)
    assert T0 < 4 * cus and pad > 0
    assert T0 % 2 == 1      # 651 rows: whole 64-row fillers keep T odd, so T % 8 != 0 on a part of any CU count
    for names in (small, small + ["filler"] * pad):
        enc, p = encode(eng, [structure(n)[0] for n in names])
        T = int(p["starts"][-1])
        assert (T < 4 * cus) if names is small else (T >= 4 * cus + 9 and T % 8 != 0)
        seqs, ranks = context_inputs(names)
        got = decode(eng, enc, seqs, ranks)
        ei = enc.E_idx.cpu().numpy()
        for k, name in enumerate(names):
            s, e = int(p["starts"][k]), int(p["starts"][k + 1])
            own = ranks[:, s:e]
            if (name, precision) not in _ALONE:
                _ALONE[name, precision] = encode(eng, [structure(name)[0]])[0]
            enc1 = _ALONE[name, precision]
            one_ei = enc1.E_idx.cpu().numpy()
            one = decode(eng, enc1, seqs[:, s:e], own)
            np.testing.assert_array_equal(np.where(ei[s:e] < 0, -1, ei[s:e] - s), one_ei, err_msg=f"{name} E_idx rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(got["ddg"][:, s:e], one["ddg"], err_msg=f"{name} ddg rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(got["hidden"][:, :, s:e], one["hidden"], err_msg=f"{name} hidden rows {s}:{e} of T={T}")
            np.testing.assert_array_equal(got["log_probs"][:, s:e], one["log_probs"], err_msg=f"{name} log_probs rows {s}:{e} of T={T}")
            if names is small:                                    # the interleaved rank values decode as the restatement reads them
                Keff = min(48, e - s)
                ref = restated(name, seqs[:, s:e], own, one_ei[:, :Keff])
                within_the_lines(one, ref, seqs[:, s:e], structure(name)[0]["mask"], f"{precision}/context")


# ---- e. variant count and chunking --------------------------------------------------------------------------
def chunks_of(V, T, cus):
    """The launcher's documented rule (launch_variant_msg): as many workgroups per residue as fill the chip four times over, but not
    under 8 variants each. -> (variants per workgroup, workgroups per residue, variants of the last one)."""
    want = -(-4 * cus // T)
    vc = max(-(-V // want), min(V, 8))
    n = -(-V // vc)
    return vc, n, V - (n - 1) * vc


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["syn_L32", "2OCJ_A_gap"])
def test_variant_count_and_chunking(name, precision):
    """A variant's numbers depend neither on V, nor on its slot in a workgroup's chunk, nor on max_rows: prefixes of one set of 33
    (sequence, rank) pairs against the one V = 33 call, bit for bit; that call against the restatement."""
    eng = engine(precision)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p, _ = structure(name)
    enc, _ = encode(eng, [p])
    L = len(p["S"])
    ei = enc.E_idx.cpu().numpy()[:, :min(48, L)]
    assert (ei >= 0).all()
    rng = np.random.default_rng(29)
    seqs = np.concatenate([p["S"][None], rng.integers(0, 21, (32, L))]).astype(np.int64)
    seqs[:, p["S"] == 20] = 20
    ranks = np.stack([rng.permutation(L) for _ in range(30)] + [np.zeros(L, np.int64), np.arange(L), int32_spread(L, rng)]).astype(np.int64)
    sweep = [1, 2, 7, 8, 9, 16, 17, 33]
    if not any(chunks_of(V, L, cus)[2] == 1 and chunks_of(V, L, cus)[1] > 1 for V in sweep):
        sweep += [V for V in range(2, 34) if chunks_of(V, L, cus)[2] == 1 and chunks_of(V, L, cus)[1] > 1][:1]
    if not any(chunks_of(V, L, cus)[1] >= 2 for V in sweep):
        sweep += [V for V in range(2, 34) if chunks_of(V, L, cus)[1] >= 2][:1]
    rule = {V: chunks_of(V, L, cus) for V in sweep}
    print(f"{name}: T={L}, CUs={cus}, (VC, chunks, last) per V: {rule}")
    assert any(n > 1 and last == 1 for _, n, last in rule.values()), "no call whose last workgroup gets exactly one variant"
    assert any(V < 8 for V in rule) and any(n >= 2 for _, n, _ in rule.values())
    want = dict(want_ddg=True, want_hidden=True, want_log_probs=True)
    full = eng.decode_ordered(enc, seqs, ranks, **want)
    for V in sweep:
        part = eng.decode_ordered(enc, seqs[:V], ranks[:V], **want)
        for k in full:
            assert torch.equal(part[k], full[k][:V]), (name, V, k)
    for rows in (L, 9 * L):
        part = eng.decode_ordered(enc, seqs, ranks, max_rows=rows, **want)
        for k in full:
            assert torch.equal(part[k], full[k]), (name, rows, k)
    within_the_lines({k: v.cpu().numpy() for k, v in full.items()}, restated(name, seqs, ranks, ei), seqs, p["mask"], f"{precision}/chunking")


# ---- f. the ProteinMPNN API on masked layouts -----------------------------------------------------------------
def model_for(precision):
    from thermompnn_amd import weights as wts
    from thermompnn_amd.protein_mpnn_utils import ProteinMPNN
    if precision not in _MODELS:
        m = ProteinMPNN(21, 128, 128, 128, k_neighbors=48, augment_eps=0.0)
        m.load_state_dict(wts.split_transfer_state_dict(wts.synthetic_state_dict(0))[0])
        m.precision, m.retry_precision = precision, None
        _MODELS[precision] = m.eval().cuda()
    return _MODELS[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["msk_L17", "msk_L40", "msk_L56_2ch"])
def test_probs_api_on_masked_layouts(name, precision):
    """conditional_probs (with and without backbone_only) and unconditional_probs against the restatement under conditional_ranks
    on the graph Engine.encode gives for the same inputs, with chain_M all ones and with a partial chain_M that covers masked
    residues too: rows outside chain_M * mask exactly 0, looped rows of the partial call with the bits of the all-ones call."""
    m = model_for(precision)
    p, g = structure(name)
    L, live = len(p["S"]), p["mask"] > 0
    b = {k: v[None] for k, v in pack([p]).items() if k in ("X", "S", "mask", "ridx", "cenc")}
    b["S"], b["ridx"], b["cenc"] = b["S"].long(), b["ridx"].long(), b["cenc"].long()
    enc, _ = encode(m.engine(), [p])
    ei, _ = checked_graph(name, enc.E_idx.cpu().numpy())
    randn_np = load_golden("ordered_" + name)["randn"]
    randn = torch.from_numpy(randn_np).cuda()
    pick = np.zeros(L, bool)
    pick[1::3] = True
    pick[~live] = True                                            # masked residues inside the selection are still not looped over
    pick[np.nonzero(live)[0][0]] = False
    S = p["S"].astype(np.int64)
    unc_ref = restated(name, S[None], np.zeros((1, L), np.int64), ei)["log_probs"][0]
    idx = np.nonzero(live)[0]
    cond_ref = restated(name, np.tile(S, (len(idx), 1)), np.stack([conditional_ranks(randn_np, int(i), L) for i in idx]), ei)["log_probs"]
    cond_full = np.zeros((L, 21), np.float32)
    cond_full[idx] = cond_ref[np.arange(len(idx)), idx]
    first = int(idx[len(idx) // 2])                                  # backbone_only through its own ranks: the position first
    bb_ref = restated(name, S[None], conditional_ranks(randn_np, first, L, True)[None], ei)["log_probs"][0, first]
    assert float(np.abs(bb_ref - unc_ref[first]).max()) <= 1e-6      # ... sees nobody: the all-equal decode's row
    margin("api/cond_vs_uncond/restatement", np.abs(cond_full - unc_ref)[live].max(), ORDER_MOVES)
    tag = f"{precision}/api"
    with torch.no_grad():
        unc = m.unconditional_probs(b["X"], b["mask"], b["ridx"], b["cenc"])
        assert unc.shape == (1, L, 21)
        close(unc[0].cpu().numpy(), unc_ref, TOL_INTERMEDIATE, tag, "uncond")
        full = {}
        for chain, looped in ((np.ones(L, bool), live), (pick, pick & live)):
            assert 0 < looped.sum() and (chain is not pick or (looped.sum() < live.sum() and (pick & ~live).any()))
            chain_M = torch.from_numpy(chain.astype(np.float32)).cuda()[None]
            sel = torch.from_numpy(looped)
            for bb in (False, True):
                got = m.conditional_probs(b["X"], b["S"], b["mask"], chain_M, b["ridx"], b["cenc"], randn, backbone_only=bb)[0].cpu()
                assert got.shape == (L, 21) and (got[~sel] == 0).all()
                ref = np.where(looped[:, None], unc_ref if bb else cond_full, 0)
                close(got.numpy(), ref, TOL_INTERMEDIATE, tag, "cond_backbone_only" if bb else "cond")
                if chain is pick:
                    assert torch.equal(got[sel], full[bb][sel])
                else:
                    full[bb] = got
        margin("api/cond_vs_uncond/device", float((full[False] - unc[0].cpu()).abs()[torch.from_numpy(live)].max()), ORDER_MOVES)
