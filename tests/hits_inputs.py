"""Inputs for the hit-list tests that go beyond a pool of eight values: tables of arbitrary 32-bit patterns, letters on both sides of
0..19, the batch that reaches every sort width and stage-1 size of csrc/tmpnn_hits.hip, and the conditions on such inputs that keep a
test from passing while it tests nothing. Shared by tests/test_hits_host.py and tests/test_gpu_hits_network.py; no GPU, no torch."""
import numpy as np

B = 256                                     # residues per stage-1 block (csrc/tmpnn_hits.hip)
NEG_NAN_QUIET, NEG_NAN_ONES, SNAN = 0xffc00000, 0xffffffff, 0x7f800001
NEG_ZERO, POS_ZERO, NEG_INF, MINUS_ONE = 0x80000000, 0x00000000, 0xff800000, 0xbf800000

# 18 proteins. Single block: pow2(rows * 20) = 64, 128, ... 8192, every stage-1 size above the 32 of one row. Several blocks: the tail
# blocks repeat those sizes, nb = 2, 3, 4, 5, 7, 12, 16, 17, 24, 31 leader lists meet in the merge kernel.
NETWORK_LENGTHS = [3, 4, 7, 13, 26, 52, 103, 205,
                   B + 4, 2 * B + 13, 3 * B + 26, 4 * B + 52, 6 * B + 103, 11 * B + 205, 16 * B, 16 * B + 1, 23 * B + 7, 30 * B + 255]
NETWORK_KS = (2, 3, 4, 5, 16, 17, 32, 33, 64, 100, 128, 129, 255)       # m = 2, 4, 4, 8, 16, 32, 32, 64, 64, 128, 128, 256, 256


def bits_table(T, ld, seed):
    """[T, ld] float32 of uniform random 32-bit patterns with about a twelfth of the entries overwritten by each of eight classes:
    denormals of both signs, the quiet negative NaN, the all-ones NaN, a signalling NaN, -0.0, +0.0, -inf, and -1.0 with its three
    neighbours. Handed over as float32 by a view: no conversion ever touches the bits."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, size=(T, ld), dtype=np.uint64).astype(np.uint32)
    cls = rng.integers(0, 12, size=(T, ld))                              # 8 .. 11: the random pattern stays
    for c, val in enumerate((b & np.uint32(0x807fffff), NEG_NAN_QUIET, NEG_NAN_ONES, SNAN, NEG_ZERO, POS_ZERO, NEG_INF,
                             np.uint32(MINUS_ONE) + (b & np.uint32(3)))):
        b = np.where(cls == c, np.asarray(val, dtype=np.uint32), b)
    return np.ascontiguousarray(b.astype(np.uint32)).view(np.float32)


def letters(T, seed):
    """[T] int32 drawn from -2 .. 22: negative and >= 20 (no residue) both occur."""
    return np.random.default_rng(seed).integers(-2, 23, size=T).astype(np.int32)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def candidate_sites(table, S, include_cys=False):
    """[T, 20] bool: the sites whose residue and letter make a candidate, whatever the value there."""
    S = np.asarray(S).astype(np.int64)
    aa = np.arange(20)[None, :]
    site = ((S >= 0) & (S < 20))[:, None] & (aa != S[:, None])
    return site if include_cys else site & (aa != 1)


def negative_nan(table):
    b = np.ascontiguousarray(table).view(np.uint32)
    return (b >> 31 == 1) & ((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000))


def assert_table_is_hostile(table, S):
    """What keeps a test on a bit-pattern table honest: negative NaNs — whose order-preserving image is near 0, the best hit of every
    protein if only the cutoff compare kept NaNs out — are at least 5 % of the table, and at least one sits at a candidate site."""
    nn = negative_nan(table)
    assert nn.mean() >= 0.05, nn.mean()
    assert (nn[:, :20] & candidate_sites(table, S)).any()


def candidate_counts(table, S, offsets, cutoff=None, include_cys=False, one_per_position=False):
    """[P] the number of candidates of every protein, from the raw-bit rules alone (no sort)."""
    with np.errstate(invalid="ignore"):
        ok = candidate_sites(table, S, include_cys) & ~np.isnan(table[:, :20])
        if cutoff is not None:
            ok &= table[:, :20] <= np.float32(cutoff)
    per_row = ok.any(axis=1).astype(np.int64) if one_per_position else ok.sum(axis=1)
    c = np.concatenate([[0], np.cumsum(per_row)])
    offsets = np.asarray(offsets).astype(np.int64)
    return c[offsets[1:]] - c[offsets[:-1]]


def network_batch(seed=2024):
    """The packed batch of NETWORK_LENGTHS: (table [29 751, 21], S, offsets)."""
    T = int(sum(NETWORK_LENGTHS))
    return bits_table(T, 21, seed), letters(T, seed + 1), offsets_of(NETWORK_LENGTHS)
