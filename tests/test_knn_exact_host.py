"""The inputs of tests/test_gpu_knn_exact.py, checked on the host (no GPU): the integer rule of lattice_backbones.exact_knn is, row
by row, an ascending valid top-K of the oracle's fp32 adjusted distances with ties exactly where the integer keys tie, and the
layouts have the edge rows they were built for (asserted as conditions, so a change of seed cannot quietly remove an edge)."""
import functools

import numpy as np
import pytest
import torch

from lattice_backbones import (DUPLICATED, LAYOUTS, MASKED, NAMES, SHELL, STEP, atom_offsets, backbone, exact_knn, expected_D,
                               lattice, row_keys)

KS = (48, 30)
LONG = "lat_L4200"


@functools.lru_cache(maxsize=None)
def sorted_rows(name):
    """-> (order [L,L]: every candidate in (key, index) order, ks [L,L]: the keys in that order, live [L] bool)."""
    P, mask = lattice(name)
    key = row_keys(P, mask)
    order = np.argsort(key, axis=1, kind="stable")
    return order, np.take_along_axis(key, order, 1), mask > 0


def test_the_set_of_layouts():
    shape = {n: len(lattice(n)[0]) for n in NAMES}
    assert shape == {"lat_L49m": 49, "lat_L64": 64, "lat_L65": 65, "lat_L100": 100, "lat_L300m": 300, "lat_shell": 123,
                     "lat_L600m": 600, "lat_L4200": 4200, "lat_L90hm": 90, "lat_L520hm": 520}
    assert MASKED == ["lat_L300m", "lat_L49m", "lat_L520hm", "lat_L600m", "lat_L90hm"]
    assert DUPLICATED == ["lat_L100", "lat_L300m", "lat_L4200"]
    for n in NAMES:
        P, mask = lattice(n)
        dead = int((mask == 0).sum())
        assert (dead > 0) == (n in MASKED) and set(np.unique(mask).tolist()) <= {0.0, 1.0}
        if n in ("lat_L49m", "lat_L300m", "lat_L600m"):                       # about 10 % masked
            assert 0.05 * len(P) <= dead <= 0.15 * len(P)
        if n in ("lat_L90hm", "lat_L520hm"):                                  # fewer live residues than K = 48, more than K = 30
            assert 30 < len(P) - dead < 48
        dup = len(P) - len(np.unique(P, axis=0))
        assert dup == (2 if n in DUPLICATED else 0)
        if n in DUPLICATED:
            assert (P[7] == P[3]).all() and (P[11] == P[3]).all() and mask[[3, 7, 11]].all()


@pytest.mark.parametrize("name", NAMES)
def test_generated_coordinates_are_integers_times_the_step(name):
    """exact_knn is only claimed for integer inputs: Ca is STEP * P_int exactly in fp32, the other atoms sit at fixed offsets."""
    P, mask = lattice(name)
    g = backbone(name)
    assert P.dtype == np.int64 and g["X"].dtype == np.float32 and g["X"].shape == (len(P), 4, 3)
    ca = g["X"][:, 1].astype(np.float64)
    assert np.array_equal(ca, STEP * P) and np.array_equal(ca / STEP, np.round(ca / STEP))
    assert float(np.abs(ca).max()) ** 2 * 4 * 3 < 2 ** 24                    # every squared distance is an exact fp32 integer
    off = atom_offsets()
    assert (off[1] == 0).all() and np.isfinite(off).all() and (np.abs(off[[0, 2, 3]]).max(axis=1) > 0.5).all()
    np.testing.assert_allclose(g["X"] - g["X"][:, 1:2], np.broadcast_to(off, g["X"].shape), atol=1e-5)
    assert np.array_equal(g["mask"], mask) and (g["cenc"] == 1).all() and np.array_equal(g["ridx"], np.arange(len(P)))
    assert g["S"].min() >= 0 and g["S"].max() < 20


def test_exact_knn_on_a_hand_made_case():
    """Every rule once: lower index on ties, masked candidates at the row's D_max, a masked row lists 0 .. Keff-1, a duplicate lists
    the earlier residue before itself, L < K."""
    P = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [5, 0, 0], [0, 3, 0]])
    mask = np.array([1, 1, 1, 1, 0, 1], np.float32)
    E, key = exact_knn(P, mask, 48)
    assert E.shape == (6, 6) and E.dtype.kind == "i" and key.dtype == np.int64
    assert E[0].tolist() == [0, 3, 1, 2, 4, 5] and key[0].tolist() == [0, 0, 1, 1, 9, 9]     # 4 is masked: at D_max, before 5
    assert E[3].tolist() == [0, 3, 1, 2, 4, 5]                                               # the duplicate lists 0 before itself
    assert E[4].tolist() == [0, 1, 2, 3, 4, 5] and key[4].tolist() == [0] * 6                # a masked row
    assert E[5].tolist() == [5, 0, 3, 1, 2, 4] and key[5].tolist() == [0, 9, 9, 10, 10, 10]
    E3, _ = exact_knn(P, mask, 3)
    assert np.array_equal(E3, E[:, :3])


@pytest.mark.parametrize("name", NAMES)
def test_exact_knn_is_an_ascending_valid_topk_of_the_oracle(name):
    from oracle import thermompnn_oracle as orc
    P, mask = lattice(name)
    L = len(P)
    g = backbone(name)
    order, ks, live = sorted_rows(name)
    with torch.no_grad():
        D_adj = orc.adjusted_distances(torch.from_numpy(g["X"])[None, :, 1], torch.from_numpy(mask)[None])[0].numpy()
    assert D_adj.dtype == np.float32
    rows = np.arange(0, L, 64) if name == LONG else np.arange(L)
    Ds = np.take_along_axis(D_adj[rows], order[rows], 1)                     # the oracle's distances in (key, index) order
    dk, dD = np.diff(ks[rows], axis=1), np.diff(Ds.view(np.uint32).astype(np.int64), axis=1)
    assert (dk >= 0).all() and (dD >= 0).all()                               # ascending, as bit patterns
    assert np.array_equal(dk == 0, dD == 0)                                  # equal keys <=> bit-equal distances
    for K in KS:
        E, key = exact_knn(P, mask, K, keys=row_keys(P, mask))
        Keff = min(K, L)
        assert E.shape == (L, Keff) and np.array_equal(E, order[:, :Keff]) and np.array_equal(key, ks[:, :Keff])
        assert (np.sort(E, axis=1)[:, 1:] != np.sort(E, axis=1)[:, :-1]).all()               # duplicate-free
        kth = np.sort(D_adj[rows], axis=1)[:, Keff - 1]
        got = np.take_along_axis(D_adj[rows], E[rows], 1)
        assert (got <= kth[:, None]).all() and (np.diff(got, axis=1) >= 0).all()
        # the restated kernel arithmetic gives the oracle's numbers (numpy's and torch's fp32 square roots agree on the CPU)
        if name != LONG:
            assert np.array_equal(expected_D(P, STEP, mask, E).view(np.uint32), np.take_along_axis(D_adj, E, 1).view(np.uint32))
        if (~live).any():
            assert np.array_equal(E[~live], np.broadcast_to(np.arange(Keff), (int((~live).sum()), Keff)))


def _tie_group_sizes(ks_row, place):
    """(number of keys < ks_row[place], number of keys <= ks_row[place]) of a sorted row."""
    v = ks_row[place]
    return int(np.searchsorted(ks_row, v, "left")), int(np.searchsorted(ks_row, v, "right"))


@pytest.mark.parametrize("K", KS)
def test_the_layouts_have_the_edge_rows_they_were_built_for(K):
    straddle = no_threshold = 0
    wide = []
    same_stripe = other_stripe = False
    for name in NAMES:
        if name == LONG:
            continue
        order, ks, live = sorted_rows(name)
        L = len(live)
        if L <= 48:
            continue
        for i in np.nonzero(live)[0]:
            lo, hi = _tie_group_sizes(ks[i], K - 1)                           # the tie group of the K-th place: places lo+1 .. hi
            straddle += hi > K
            # knn_row_sel needs a value whose cumulative count lies in [K, 64]; the smallest cumulative count >= K is hi
            if L > 64 and hi > 64:
                no_threshold += 1
                mask = lattice(name)[1]
                if hi - lo > 64 and mask[order[i, lo:hi]].all():
                    wide.append((name, int(i)))
            # ties inside the first K+1 places: between two indices of one lane stripe (congruent mod 64), and of two stripes
            head_k, head_j = ks[i, :K + 1], order[i, :K + 1]
            for v in np.unique(head_k[:-1][head_k[1:] == head_k[:-1]]):
                js = head_j[head_k == v]
                r = js % 64
                same_stripe |= len(np.unique(r)) < len(r)
                other_stripe |= len(np.unique(r)) > 1
    print(f"K={K}: {straddle} rows with equal K-th and (K+1)-th keys, {no_threshold} without a threshold, wide tie groups {wide}")
    assert straddle >= 100
    # K = 30 leaves a window of 35 places for a threshold: on a lattice box no tie group is that wide, only lat_shell's is
    assert no_threshold >= (10 if K == 48 else 1)
    assert (SHELL, 0) in wide
    assert same_stripe and other_stripe
    order, ks, _ = sorted_rows(SHELL)                                        # row 0: places 22 .. 93 are the 72 points at s2 = 26
    assert _tie_group_sizes(ks[0], K - 1) == (21, 93) and ks[0, K - 1] == 26 and ks[0, 63] == 26 and ks[0, 20] <= 3 and ks[0, 93] >= 36


@pytest.mark.parametrize("K", KS)
def test_the_long_layout_has_ties_across_the_two_rescan_passes(K):
    """L > 4096: the long-row form rescans a lane stripe in two passes (indices below 4096, then the rest). Rows where an index >= 4096
    ties with one < 4096 across the K-th place; among them rows where the two share a stripe (congruent mod 64)."""
    order, ks, live = sorted_rows(LONG)
    assert live.all() and len(live) > 4096
    rows, rows_same_stripe = [], []
    for i in range(len(live)):
        lo, hi = _tie_group_sizes(ks[i], K - 1)
        if hi <= K:
            continue
        js = order[i, lo:hi]
        if (js >= 4096).any() and (js < 4096).any():
            rows.append(i)
            hi_r = set((js[js >= 4096] % 64).tolist())
            if hi_r & set((js[js < 4096] % 64).tolist()):
                rows_same_stripe.append(i)
    print(f"K={K}: {len(rows)} rows tie across 4096 at the K-th place, {len(rows_same_stripe)} of them inside one stripe")
    assert len(rows) >= 1 and len(rows_same_stripe) >= 1


def test_masked_candidates_tie_with_the_farthest_live_residue_at_the_kth_place():
    """A live row lists masked residues only when it has fewer than K live candidates nearer than its farthest one: with 10 % masked
    that is lat_L49m alone (44 live residues); lat_L90hm and lat_L520hm put the same tie into rows longer than 64 and 512. There,
    at K = 48, EVERY live row's K-th place carries the key of the row's farthest live residue, ties with the place behind it
    and the row lists masked residues. In every masked layout the masked candidates of a live row carry that key and come in index order behind
    all nearer live residues."""
    for name in MASKED:
        P, mask = lattice(name)
        order, ks, live = sorted_rows(name)
        n_live = int(live.sum())
        s2 = row_keys(P, np.ones(len(P), np.float32))
        for i in np.nonzero(live)[0]:
            far = s2[i, live].max()
            assert (ks[i, n_live:] == far).all() and ks[i, n_live - 1] == far
            is_dead = ~live[order[i]]
            assert (ks[i][is_dead] == far).all() and (np.diff(order[i][is_dead]) > 0).all()
        if n_live < 48:
            E, key = exact_knn(P, mask, 48)
            for i in np.nonzero(live)[0]:
                assert key[i, 47] == s2[i, live].max() and (~live[E[i]]).any() and ks[i, 48] == key[i, 47]
        else:
            assert name in ("lat_L300m", "lat_L600m")
    assert sum(int((lattice(n)[1] > 0).sum()) < 48 for n in MASKED) == 3


@pytest.mark.parametrize("name", DUPLICATED)
def test_a_duplicate_lists_the_earlier_residue_first(name):
    P, mask = lattice(name)
    for K in KS:
        if name == LONG:
            key = row_keys(P[:12], mask[:12])                                # rows 3, 7, 11 against each other suffice for the order
            assert np.argsort(key, axis=1, kind="stable")[[3, 7, 11], :3].tolist() == [[3, 7, 11]] * 3
            order, _, _ = sorted_rows(name)
            E = order[:, :K]
        else:
            E, _ = exact_knn(P, mask, K)
        assert E[7, 0] == 3 and E[7, :3].tolist() == [3, 7, 11] and E[11, :3].tolist() == [3, 7, 11] and E[3, :3].tolist() == [3, 7, 11]


def test_pairs_at_exactly_the_centrality_radius_exist():
    """With a 2 A step, pairs at s2 = 25 lie at exactly 10.0 A: compute_centrality counts d < radius, so they must not be counted."""
    for name in ("lat_L100", "lat_L300m"):
        P, mask = lattice(name)
        s2 = row_keys(P, np.ones(len(P), np.float32))
        live = mask > 0
        at = (s2 == 25) & live[:, None] & live[None, :]
        print(name, int(at.sum()) // 2, "live pairs at exactly 10.0 A")
        assert at.sum() >= 20
