"""The hit selection (csrc/tmpnn_hits.hip) where tests/test_gpu_hits.py does not go: every sort width m = 2 .. 256, every stage-1
size 32 .. 8192, block counts up to 31 away from powers of two, tables of arbitrary 32-bit patterns (negative and signalling NaNs,
denormals, neighbouring floats), cutoffs on and beside table values, and the contract lines of include/tmpnn.h that had no device
test. Every comparison is exact against the numpy restatement (tests/hits_restatement.py), itself checked on such values in
tests/test_hits_host.py; the inputs come from tests/hits_inputs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from hits_inputs import (B, NETWORK_KS, NETWORK_LENGTHS, assert_table_is_hostile, bits_table, candidate_counts, letters, network_batch,
                         offsets_of)
from hits_restatement import assert_hits_equal, hits_reference

pytestmark = pytest.mark.gpu

INF = float("inf")
MINUS_ONE_UP = np.nextafter(np.float32(-1), np.float32(0))           # 0xbf7fffff
MINUS_ONE_DOWN = np.nextafter(np.float32(-1), np.float32(-INF))      # 0xbf800001


@pytest.fixture(scope="module")
def engine(synthetic_weights):
    from thermompnn_amd.engine import Engine
    return Engine(synthetic_weights, "cuda:0", 48)


@pytest.fixture(scope="module")
def network():
    """The 18 proteins of hits_inputs.NETWORK_LENGTHS on a bit-pattern table, uploaded once: (table, S, offsets, device table)."""
    table, S, offsets = network_batch()
    assert_table_is_hostile(table, S)
    assert (S < 0).any() and (S >= 20).any()
    dev = torch.from_numpy(table).cuda()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), table.view(np.uint32))      # the upload keeps every bit, NaN payloads too
    return table, S, offsets, dev


def _np(hits):
    return {name: v.cpu().numpy() for name, v in hits.items()}


def _row(hits, p):
    return {name: v[p:p + 1] for name, v in hits.items()}


@pytest.mark.parametrize("one", [False, True])
def test_every_sort_width_stage1_size_and_block_count_on_bit_patterns(engine, network, one):
    table, S, offsets, dev = network
    lengths = np.array(NETWORK_LENGTHS)
    widths = set()
    for i, k in enumerate(NETWORK_KS):
        cys = bool(i & 1) != one                         # alternates with k (and with `one`): both values at every width m
        widths.add((1 << (k - 1).bit_length(), cys))
        want = hits_reference(table, S, offsets, k, None, cys, one)
        have = candidate_counts(table, S, offsets, None, cys, one)
        np.testing.assert_array_equal(want["hit_count"], np.minimum(have, k))       # k hits wherever k candidates exist
        if one:
            assert (want["hit_count"] <= lengths).all()
        short = (want["hit_count"] > 0) & (want["hit_count"] < k)
        assert short.any() or k < (5 if one else 64)     # the larger k: some protein runs out of candidates and is padded
        assert (have[9:] >= k).all()                     # from three blocks on every list is full: the merge decides all k places
        got = _np(engine.select_hits(dev, S, offsets, k, include_cys=cys, one_per_position=one))
        assert_hits_equal(got, want)
        if k in (33, 129):                               # nb = 3, 7, 31 alone: the bits do not depend on the batch
            for p in (9, 12, 17):
                t0, t1 = int(offsets[p]), int(offsets[p + 1])
                alone = engine.select_hits(dev[t0:t1], S[t0:t1], [0, t1 - t0], k, include_cys=cys, one_per_position=one)
                assert_hits_equal(alone, _row(got, p))
    assert {m for m, _ in widths} == {2, 4, 8, 16, 32, 64, 128, 256}
    assert all((m, c) in widths for m in (4, 32, 64, 128, 256) for c in (False, True))


def _twelve_blocks(seed):
    """L = 12 B rows of +1.0 with a letter everywhere; -> (table, S, sites) where sites[t] is one candidate letter of row t."""
    rng = np.random.default_rng(seed)
    L = 12 * B
    S = rng.integers(0, 20, size=L).astype(np.int32)
    sites = np.array([rng.choice([a for a in range(20) if a != s and a != 1]) for s in S])
    return np.ones((L, 21), np.float32), S, sites


PLACE_KS = (5, 32, 129, 256)


@pytest.mark.parametrize("one", [False, True])
def test_winners_in_one_inner_block_all_equal_and_striped_over_blocks(engine, one):
    off = [0, 12 * B]
    # all 256 best values in block 5 only, one per row, shuffled
    table, S, sites = _twelve_blocks(31)
    rows = 5 * B + np.arange(B)
    table[rows, sites[rows]] = -(1.0 + np.random.default_rng(32).permutation(B)).astype(np.float32)
    dev = torch.from_numpy(table).cuda()
    for k in PLACE_KS:
        want = hits_reference(table, S, off, k, one_per_position=one)
        assert (want["hit_pos"][0] // B == 5).all() and want["hit_ddg"][0, 0] == -256.0
        if k == 256:
            assert sorted(want["hit_pos"][0].tolist()) == rows.tolist()          # every row of the block survives stage 1
        assert_hits_equal(engine.select_hits(dev, S, off, k, one_per_position=one), want)
    # one value everywhere: position and letter alone decide
    dev = torch.full((12 * B, 21), 0.5, device="cuda")
    first = 19 if S[0] == 1 else 18                      # position 0's candidates: 20 letters less its own and cysteine
    for k in PLACE_KS:
        want = hits_reference(dev.cpu().numpy(), S, off, k, one_per_position=one)
        got = _np(engine.select_hits(dev, S, off, k, one_per_position=one))
        assert_hits_equal(got, want)
        if one:
            assert got["hit_pos"][0].tolist() == list(range(k))
        else:
            assert got["hit_pos"][0, :first + 1].tolist() == ([0] * first + [1])[:k]
            assert (np.diff(got["hit_pos"][0] * 32 + got["hit_aa"][0]) > 0).all()
    # the j-th best value sits in block j % 12: every leader list contributes to the merge's output
    table, S, sites = _twelve_blocks(33)
    within = np.random.default_rng(34).permutation(B)
    j = np.arange(12 * 40)
    at = (j % 12) * B + within[j // 12]
    table[at, sites[at]] = (-1000.0 + j).astype(np.float32)
    dev = torch.from_numpy(table).cuda()
    for k in PLACE_KS:
        want = hits_reference(table, S, off, k, one_per_position=one)
        assert (want["hit_pos"][0] // B == np.arange(k) % 12).all() and want["hit_count"][0] == k
        assert_hits_equal(engine.select_hits(dev, S, off, k, one_per_position=one), want)


def _same(a, b):
    return all(np.array_equal(a[n].view(np.uint32) if a[n].dtype == np.float32 else a[n],
                              b[n].view(np.uint32) if b[n].dtype == np.float32 else b[n]) for n in a)


def test_cutoffs_on_the_value_grid(engine, network):
    """Cutoffs equal to a table value, one ulp to either side, -0.0, a denormal, a Python float that is no float32, +-inf. A cutoff
    shows only in a protein with fewer than k candidates below it, and bits_table holds -1.0 with the three floats BELOW it only. So
    here protein 0 (three rows) is +2.0 everywhere, and the rows of proteins 0 .. 3 get the float above -1.0, -1.0, the float below
    it and the smallest denormal at candidate sites: the three cutoffs around -1.0, and 1e-40 against 0.0, all separate."""
    table, S, offsets, _ = network
    table = table.copy()
    bits = table.view(np.uint32)
    table[:int(offsets[1])] = 2.0
    assert ((S[:int(offsets[1])] >= 0) & (S[:int(offsets[1])] < 20)).any()
    for t in range(int(offsets[4])):                     # proteins 0 .. 3: 27 rows
        if 0 <= S[t] < 20:
            free = [a for a in range(2, 20) if a != S[t]]
            bits[t, free[:4]] = 0xbf7fffff, 0xbf800000, 0xbf800001, 0x00000001
    assert_table_is_hostile(table, S)
    dev = torch.from_numpy(table).cuda()
    for k in (17, 128):
        ref = {}
        for cutoff in (0.0, -0.0, -1.0, MINUS_ONE_UP, MINUS_ONE_DOWN, 1e-40, -0.1, -INF, INF, None):
            for one in (False, True):
                want = hits_reference(table, S, offsets, k, cutoff, False, one)
                assert_hits_equal(engine.select_hits(dev, S, offsets, k, cutoff=None if cutoff is None else float(cutoff), one_per_position=one), want)
                ref[(str(cutoff), one)] = want
        up, at, down = (ref[(str(c), False)] for c in (MINUS_ONE_UP, -1.0, MINUS_ONE_DOWN))
        assert not _same(up, at) and not _same(at, down) and not _same(up, down)
        assert (up["hit_count"] >= at["hit_count"]).all() and (at["hit_count"] >= down["hit_count"]).all()
        assert _same(ref[("0.0", False)], ref[("-0.0", False)]) and _same(ref[("inf", False)], ref[("None", False)])
        assert not _same(ref[("1e-40", False)], ref[("0.0", False)])                 # a denormal cutoff is not flushed to zero
        low = ref[("-inf", False)]
        n = low["hit_count"]
        assert n.sum() > 0 and all((low["hit_ddg"][p, :n[p]].view(np.uint32) == 0xff800000).all() for p in range(len(n)))


def test_empty_proteins_first_in_the_middle_and_last_and_a_protein_without_letters(engine):
    offsets = [0, 0, 300, 300, 300, 813, 813]
    table, S = bits_table(813, 21, 41), letters(813, 42)
    assert_table_is_hostile(table, S)
    dev = torch.from_numpy(table).cuda()
    for k, one in ((33, False), (256, True)):
        got = _np(engine.select_hits(dev, S, offsets, k, one_per_position=one))
        assert_hits_equal(got, hits_reference(table, S, offsets, k, one_per_position=one))
        for p in (0, 2, 3, 5):
            assert got["hit_count"][p] == 0 and (got["hit_pos"][p] == -1).all() and (got["hit_aa"][p] == -1).all()
            assert (got["hit_ddg"][p].view(np.uint32) == 0x7fc00000).all()
        for p, (t0, t1) in ((1, (0, 300)), (4, (300, 813))):
            assert got["hit_count"][p] > 0
            assert_hits_equal(engine.select_hits(dev[t0:t1], S[t0:t1], [0, t1 - t0], k, one_per_position=one), _row(got, p))
    S2 = S.copy()
    S2[300:813] = -1                                     # negative letters: no residue
    got = _np(engine.select_hits(dev, S2, offsets, 33))
    assert_hits_equal(got, hits_reference(table, S2, offsets, 33))
    assert got["hit_count"].tolist() == [0, 33, 0, 0, 0, 0]


def test_tables_of_twenty_columns_strided_and_transposed_and_device_index_arrays(engine):
    lengths = [7, 300, 0, 513]
    T, offsets = sum(lengths), offsets_of(lengths)
    table, S = bits_table(T, 20, 51), letters(T, 52)
    assert_table_is_hostile(table, S)
    want = {(k, one): hits_reference(table, S, offsets, k, one_per_position=one) for k in (17, 100) for one in (False, True)}
    dev = torch.from_numpy(table).cuda()
    wide = torch.from_numpy(bits_table(T, 24, 53)).cuda()                # hostile bits around the window as well
    wide[:, 2:22] = dev
    turned = dev.t().contiguous().t()                                    # [T, 20] with strides (1, T): select_hits packs it
    assert wide[:, 2:22].data_ptr() != wide.data_ptr() and turned.stride() == (1, T)
    assert np.array_equal(wide[:, 2:22].cpu().numpy().view(np.uint32), table.view(np.uint32))
    S_dev, off_dev = torch.from_numpy(S).cuda(), torch.from_numpy(offsets).cuda()
    for (k, one), w in want.items():
        for tab in (dev, wide[:, 2:22], turned):
            assert_hits_equal(engine.select_hits(tab, S, offsets, k, one_per_position=one), w)
        assert_hits_equal(engine.select_hits(dev, S_dev, off_dev, k, one_per_position=one), w)
        assert_hits_equal(engine.select_hits(wide[:, 2:22], S_dev.long(), off_dev.long(), k, one_per_position=one), w)


def test_c_entry_gives_an_overlong_protein_minus_one_and_serves_its_neighbour(engine):
    """include/tmpnn.h: a protein above 8192 rows gets hit_count = -1 and padding, the others are served, the return code is
    TMPNN_OK. Engine.select_hits refuses such a batch on the host, so the entry is called as Engine would call it. Well-formed
    offsets; the neighbour's workspace slots are (8193 >> 8) + 1 = 33 and 34 of (8493 >> 8) + 2 = 35."""
    k, T = 33, 8493
    table, S = bits_table(T, 21, 61), letters(T, 62)
    assert_table_is_hostile(table[8193:], S[8193:])
    dev, S_dev = torch.from_numpy(table).cuda(), torch.from_numpy(S).cuda()
    off_dev = torch.tensor([0, 8193, T], dtype=torch.int32, device="cuda")
    hit_ddg = torch.full((2, k), 7.0, dtype=torch.float32, device="cuda")
    hit_pos, hit_aa = (torch.full((2, k), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    hit_count = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    need = engine.lib.tmpnn_hits_workspace_bytes(T, 2, k)
    assert need >= 35 * k * 8
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = engine.lib.tmpnn_select_hits(ptr(dev), 21, ptr(S_dev), ptr(off_dev), 2, T, k, INF, 0, ptr(hit_ddg), ptr(hit_pos), ptr(hit_aa),
                                      ptr(hit_count), ptr(ws), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = _np(dict(hit_ddg=hit_ddg, hit_pos=hit_pos, hit_aa=hit_aa, hit_count=hit_count))
    assert got["hit_count"][0] == -1 and (got["hit_pos"][0] == -1).all() and (got["hit_aa"][0] == -1).all()
    assert np.isnan(got["hit_ddg"][0]).all()
    want = hits_reference(table[8193:], S[8193:], [0, 300], k)
    assert want["hit_count"][0] == k
    assert_hits_equal(_row(got, 1), want)


def test_a_batch_without_rows_is_padding_without_a_launch(engine):
    got = _np(engine.select_hits(torch.empty((0, 21), device="cuda"), [], [0, 0, 0], 5))
    assert_hits_equal(got, hits_reference(np.zeros((0, 21), np.float32), np.zeros(0, np.int32), [0, 0, 0], 5))
    assert got["hit_count"].tolist() == [0, 0] and got["hit_pos"].shape == (2, 5)
