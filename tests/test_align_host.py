"""The numpy restatements of tmpnn_align_global and tmpnn_ensemble_stats_rows (tests/align_restatement.py) held against what they
restate, on the host: the alignment against datasets.global_alignment_map on letter strings and against a brute-force LCS, the
statistics through a row map against ensemble_restatement on the gathered table. No GPU."""
import itertools

import numpy as np

from align_inputs import SMALL, draw_rows, make_pair, small_batch
from align_restatement import (LETTERS, align_map, align_reference, codes, ensemble_rows_reference, gather, lcs_brute)
from ensemble_inputs import DRAWS, crafted
from ensemble_restatement import assert_ensemble_equal, ensemble_reference


def _letters(a):
    return "".join(LETTERS[int(c)] for c in a)


def test_restatement_equals_global_alignment_map_on_letter_strings():
    from thermompnn_amd.datasets import global_alignment_map
    rng = np.random.default_rng(5)
    seen = 0
    for n, m in [s for s in SMALL if max(s) <= 70]:
        for kind in ("two", "twenty", "identical", "disjoint", "deletions"):
            if kind == "deletions" and n < 8:
                continue
            a, b = make_pair(kind, n, m, rng)
            sa, sb = _letters(a), _letters(b)
            want = [-1 if j is None else j for j in global_alignment_map(sa, sb)]
            got, count = align_map(codes(sa), codes(sb))
            assert got.tolist() == want, (kind, n, m)
            assert count == sum(j >= 0 for j in want)
            assert all(sa[q] == sb[j] for q, j in enumerate(want) if j >= 0)          # the mismatch column never fires
            seen += 1
    assert seen >= 25


def test_every_short_pair_over_two_letters():
    moved = 0
    words = [w for k in range(6) for w in itertools.product((0, 1), repeat=k)]
    for a in words:
        for b in words:
            a_, b_ = np.array(a, np.int32), np.array(b, np.int32)
            out, count = align_map(a_, b_)
            hit = out[out >= 0]
            assert (np.diff(hit) > 0).all() and len(hit) == count
            assert all(a_[q] == b_[j] for q, j in enumerate(out) if j >= 0)
            assert count == lcs_brute(a_, b_), (a, b)
            other, count2 = align_map(a_, b_, rule="down_first")
            assert count2 == count                                                    # equally optimal ...
            moved += int(other.tolist() != out.tolist())
    assert moved > 500, moved                                                         # ... and another map: the fixtures tell the rules apart


def test_another_tie_rule_moves_the_map_on_the_two_letter_fixtures():
    # (an axis that is a subsequence of the member, as 19 codes in 70 are, aligns whole: no step down ever ties there, so the rules
    # can differ only where axis positions stay unaligned: n >= m)
    moved = []
    for kind, n, m, a, b in small_batch():
        if kind == "two" and n >= m >= 19:
            got, count = align_map(a, b)
            other, count2 = align_map(a, b, rule="down_first")
            assert count == count2 and got.tolist() != other.tolist(), (n, m)
            moved.append((n, m))
    assert moved == [(70, 19), (257, 256)]


def test_codes_outside_the_twenty_letters_never_match():
    odd = np.array([20, 21, -1, -2 ** 31, 20, 21, -1], np.int32)
    out, count = align_map(odd, odd)
    assert count == 0 and (out == -1).all()
    a = np.array([3, 20, 5, -1, 7, 21], np.int32)
    out, count = align_map(a, a)                                                      # itself: the letters align, the rest does not
    assert out.tolist() == [0, -1, 2, -1, 4, -1] and count == 3
    assert codes("ACX-Y").tolist() == [0, 1, 20, 21, 19]
    rng = np.random.default_rng(3)
    a, b = make_pair("nonmatch", 70, 19, rng)
    out, _ = align_map(a, b)
    assert ((a < 0) | (a >= 20)).sum() >= 5 and all(0 <= a[q] < 20 and a[q] == b[j] for q, j in enumerate(out) if j >= 0)


def test_call_restatement_checks_descriptors_and_adds():
    a, b = np.array([0, 1, 2], np.int32), np.array([1, 2], np.int32)
    A, B = np.concatenate([a, a]), np.concatenate([b, b])
    desc = np.array([(0, 3, 0, 2, 0, 100), (3, 3, 2, 2, 3, -7), (3, 4, 2, 2, 3, 0)])
    res = align_reference(A, B, desc, 6, 3, 2, out=np.full(6, 55, np.int32), aligned=np.full(3, 66, np.int32))
    assert res["out"].tolist() == [-1, 100, 101, -1, -7, -6] and res["aligned"].tolist() == [2, 2, 66] and res["status"].tolist() == [0, 0, -1]


def test_rows_restatement_equals_the_ensemble_restatement_on_the_gathered_table():
    for draw in DRAWS:
        c = crafted(draw)
        rng = np.random.default_rng(21)
        for rows in (np.arange(c["T"], dtype=np.int32), draw_rows(c, rng)):
            got = ensemble_rows_reference(c["ddg"], c["S"], rows, c["desc"], c["T_out"], c["max_len"], cutoff=-0.5)
            table, S = gather(c["ddg"], c["S"], rows)
            want = ensemble_reference(table, S, c["desc"], c["T_out"], c["max_len"], cutoff=-0.5)
            assert_ensemble_equal(got, want)
            assert got["status"].tolist() == want["status"].tolist() == [0] * len(c["desc"])
        outside = (rows < 0) | (rows >= c["T"])
        assert outside.sum() > 50 and (S[outside] == 20).all() and len(set(rows[~outside].tolist())) < (~outside).sum()   # shared rows
        plain = ensemble_reference(c["ddg"], c["S"], c["desc"], c["T_out"], c["max_len"], cutoff=-0.5)
        assert (plain["count"] != got["count"]).any()                                 # the drawn map is not the identity
