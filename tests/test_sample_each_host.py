"""Host side of per-protein sampling (no GPU): the segmented-permutation check, the chunk planner, the descending-length launch
order, and the design_scan driver's pieces — the restatement of the reference's _scores (against a recorded fixture, and against
the reference's own function where its checkout is present), the FASTA writer, batch packing, --fixed, and the seeded chains."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

OFFSETS = [0, 32, 49, 89, 145]


def segmented_orders(offsets, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([a + rng.permutation(b - a) for a, b in zip(offsets, offsets[1:])]) for _ in range(N)])


# ---- the segmented-permutation check ------------------------------------------------------------------------------------
def verdicts(order, S=None, close=None, offsets=OFFSETS):
    from thermompnn_amd.engine import each_verdicts
    order = torch.as_tensor(order, dtype=torch.int32)
    S = torch.zeros_like(order) if S is None else torch.as_tensor(S, dtype=torch.int32)
    close = None if close is None else torch.as_tensor(close, dtype=torch.int32)
    return each_verdicts(order, S, close, torch.tensor(offsets, dtype=torch.int32)).tolist()


def test_segmented_permutation_check():
    order = segmented_orders(OFFSETS, 3, 0)
    assert verdicts(order) == [True, True, True]
    outside = order.copy()
    outside[1, [5, 40]] = outside[1, [40, 5]]                            # a permutation of 0..144 with two entries in the wrong protein
    assert verdicts(outside) == [True, False, True]
    repeated = order.copy()
    repeated[2, 7] = repeated[2, 8]
    assert verdicts(repeated)[0] is False
    assert verdicts(order + 1)[0] is False and verdicts(order - 1)[0] is False          # out of range: refused, nothing indexed with it
    assert verdicts(np.tile(np.arange(145), (2, 1))) == [True, True, True]             # left to right is a valid schedule
    assert verdicts(np.tile(np.arange(145)[::-1], (2, 1)))[:2] == [True, False]         # the whole axis reversed is not
    letters = np.zeros_like(order)
    letters[0, 3] = 21
    assert verdicts(order, S=letters) == [True, True, False]
    # empty proteins take no position
    assert verdicts(segmented_orders([0, 32, 32, 49], 2, 1), offsets=[0, 32, 32, 49]) == [True, True, True]


def test_every_protein_must_close():
    order = segmented_orders(OFFSETS, 2, 3)
    close = np.ones_like(order)
    assert verdicts(order, close=close) == [True] * 5
    pairs = close.copy()
    pairs[:, 0:144:2] = 0                                               # groups of two ... 144 closes, and so do 31 / 48 / 88
    assert verdicts(order, close=pairs)[4] is False                     # step 48 (even) is protein 1's last and stays open
    ok = pairs.copy()
    ok[:, [48, 88]] = 1
    assert verdicts(order, close=ok) == [True] * 5
    spans = close.copy()
    spans[1, 31] = 0                                                    # protein 0's last step open: its group would run into protein 1
    assert verdicts(order, close=spans)[3:] == [True, False]
    two = close.copy()
    two[0, 10] = 2
    assert verdicts(order, close=two)[3] is False


# ---- the chunk planner -------------------------------------------------------------------------------------------------
def check_plan(offsets, N, max_rows):
    from thermompnn_amd.engine import EACH_ROWS_MAX, plan_each_chunks
    plan = plan_each_chunks(offsets, N, max_rows)
    P = len(offsets) - 1
    seen = np.zeros((P, N), np.int64)
    cap = min(max_rows if max_rows is not None else 1 << 18, EACH_ROWS_MAX)
    for p0, p1, n0, n1 in plan:
        assert 0 <= p0 < p1 <= P and 0 <= n0 < n1 <= N                  # one protein and one chain at least
        seen[p0:p1, n0:n1] += 1
        rows = offsets[p1] - offsets[p0]
        if (n1 - n0) * rows > cap:                                      # only a single protein too long for one chain breaks max_rows
            assert p1 == p0 + 1 and n1 == n0 + 1 and rows > cap
        assert 3 * (n1 - n0) * rows < 1 << 24 or rows > EACH_ROWS_MAX
    assert (seen == 1).all()
    return plan


def test_chunk_planner():
    assert check_plan(OFFSETS, 17, None) == [(0, 4, 0, 17)]
    assert [c[:2] for c in check_plan(OFFSETS, 17, 17 * 49)] == [(0, 2), (2, 3), (3, 4), (3, 4)]
    assert check_plan(OFFSETS, 17, 17 * 56)[-1] == (3, 4, 0, 17)
    assert check_plan(OFFSETS, 17, 5 * 56)[:3] == [(0, 1, 0, 8), (0, 1, 8, 16), (0, 1, 16, 17)]
    plan = check_plan(OFFSETS, 3, 40)                                   # proteins 0 and 3 alone exceed max_rows: still planned, chain by chain
    assert (3, 4, 2, 3) in plan and (0, 1, 0, 1) in plan and len(plan) == 11
    check_plan([0, 5, 5, 9], 4, 8)                                      # an empty protein in the middle
    check_plan([0, 7], 1, 1)
    assert check_plan(OFFSETS, 0, None) == [] and check_plan([0], 3, None) == []
    # the hard bound of one launch holds whatever max_rows says: 3 * N * rows < 2**24
    big = [0, 4000, 8000, 12000]
    for c in check_plan(big, 1000, 1 << 30):
        assert 3 * (c[3] - c[2]) * (big[c[1]] - big[c[0]]) < 1 << 24
    rng = np.random.default_rng(0)
    for _ in range(50):
        offs = np.concatenate([[0], np.cumsum(rng.integers(0, 70, rng.integers(1, 9)))]).tolist()
        check_plan(offs, int(rng.integers(1, 40)), int(rng.integers(1, 3000)))


def test_descending_length_schedule():
    from thermompnn_amd.engine import each_schedule
    assert each_schedule(OFFSETS, 0, 4).tolist() == [3, 2, 0, 1] and each_schedule(OFFSETS, 0, 4).dtype == np.int32
    assert each_schedule(OFFSETS, 1, 3).tolist() == [2, 1]
    assert each_schedule(OFFSETS, 2, 3).tolist() == [2] and each_schedule(OFFSETS, 2, 2).tolist() == []
    assert each_schedule([0, 10, 20, 25, 35], 0, 4).tolist() == [0, 1, 3, 2]           # ties keep index order


# ---- the driver's pieces --------------------------------------------------------------------------------------------------
def reference_scores():
    """The reference's own _scores where its checkout is present (the path tests/golden/make_golden.py imports it from), else None."""
    text = open(os.path.join(GOLDEN, "make_golden.py")).read()
    path = os.path.join(re.search(r'^REF = "(.*)"', text, re.M).group(1), "protein_mpnn_utils.py")
    if not os.path.exists(path):
        return None
    spec = importlib.util.spec_from_file_location("_reference_protein_mpnn_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._scores


def test_scores_restates_the_reference():
    from thermompnn_amd.design_scan import scores
    g = load_golden("scores_small")
    S, lp, mask = torch.from_numpy(g["S"]), torch.from_numpy(g["log_probs"]), torch.from_numpy(g["mask"])
    got = scores(S, lp, mask)
    assert got.shape == (3,) and float((got - torch.from_numpy(g["scores"])).abs().max()) <= 1e-6
    by_hand = -sum(float(lp[1, k, S[1, k]]) for k in (1, 2, 4, 5)) / 4                  # row 1: positions 0, 3, 6 are not designed
    assert abs(float(got[1]) - by_hand) <= 1e-6 and abs(float(got[2]) + float(lp[2, 4, S[2, 4]])) <= 1e-6
    assert torch.equal(scores(S.to(torch.int32), lp, mask), got)                         # the sampler's int32 letters
    ref = reference_scores()
    if ref is not None:
        rng = np.random.default_rng(1)
        S2 = torch.from_numpy(rng.integers(0, 21, (4, 9)))
        lp2 = torch.log_softmax(torch.from_numpy(rng.normal(size=(4, 9, 21)).astype(np.float32)), -1)
        m2 = torch.from_numpy((rng.random((4, 9)) > 0.3).astype(np.float32))
        m2[:, 0] = 1
        assert float((scores(S2, lp2, m2) - ref(S2, lp2, m2)).abs().max()) <= 1e-6
        assert float((got - ref(S, lp, mask)).abs().max()) <= 1e-6


def test_fasta_writer():
    from thermompnn_amd.design_scan import fasta_records, letters
    entry = dict(S=np.array([0, 1, 20, 3, 19]), mask=np.array([1, 1, 0, 1, 0], np.float32))
    assert letters(entry["S"], entry["mask"]) == "ACXEX"
    result = dict(S=np.array([[4, 5, 6, 7, 8], [0, 1, 2, 3, 4]]), score=np.array([1.25, 2.0]), seq_recovery=np.array([0.5, 1 / 3]))
    text = fasta_records("toy", entry, result, 0.1, 7)
    lines = text.split("\n")
    assert text.endswith("\n") and len(lines) == 7 and lines[-1] == ""
    assert lines[0] == ">toy, native, L=5, unmasked=3" and lines[1] == "ACXEX"
    assert lines[2] == ">toy, sample=1, T=0.1, seed=7, score=1.250000, seq_recovery=0.5000" and lines[3] == "FGXIX"
    assert lines[4] == ">toy, sample=2, T=0.1, seed=7, score=2.000000, seq_recovery=0.3333" and lines[5] == "ACXEX"


def test_batches_fixed_positions_and_seeded_chains():
    from thermompnn_amd.design_scan import draw_chains, join_chains, pack_batches, parse_positions, ranks_of
    from thermompnn_amd.engine import each_verdicts
    assert pack_batches([100, 200, 50, 400, 10], 300) == [[0, 1], [2], [3], [4]]
    assert pack_batches([100, 200, 50, 400, 10], 1000) == [[0, 1, 2, 3, 4]] and pack_batches([], 10) == []
    assert parse_positions("1,5,10-12") == [0, 4, 9, 10, 11] and parse_positions(None) == [] and parse_positions("3-3") == [2]
    with pytest.raises(ValueError):
        parse_positions("0")
    with pytest.raises(ValueError):
        parse_positions("5-2")
    entries = [dict(S=np.arange(12) % 21, mask=np.array([1] * 10 + [0, 1], np.float32)), dict(S=np.arange(7), mask=np.ones(7, np.float32))]
    draw = lambda seed: [draw_chains(e, 3, [0, 4, 30], g) for g in [torch.Generator().manual_seed(seed)] for e in entries]
    a, b, other = draw(1), draw(1), draw(2)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in x)
    assert not np.array_equal(a[0]["order"], other[0]["order"]) and not np.array_equal(a[1]["u"], other[1]["u"])
    c0 = a[0]
    assert c0["order"].shape == (3, 12) and (np.sort(c0["order"], 1) == np.arange(12)).all()
    assert (c0["free"][:, [0, 4]] == 0).all() and c0["free"].sum() == 3 * 10 and (c0["S_fixed"] == entries[0]["S"]).all()
    assert (np.sort(c0["order"][:, :3], 1) == [0, 4, 10]).all()         # fixed and masked positions are decoded first
    assert ((c0["u"] >= 0) & (c0["u"] < 1)).all() and not np.array_equal(c0["order"][0], c0["order"][1])
    c = join_chains(a)
    assert c["order"].shape == (3, 19) and (c["order"][:, 12:] >= 12).all()
    ok = each_verdicts(torch.as_tensor(c["order"]), torch.as_tensor(c["S_fixed"]), None, torch.tensor([0, 12, 19]))
    assert ok.tolist() == [True, True, True]
    order = torch.as_tensor(c["order"])
    rank = ranks_of(order)
    assert rank.dtype == torch.int32 and torch.equal(torch.gather(rank.long(), 1, order), torch.arange(19)[None].expand(3, 19))
