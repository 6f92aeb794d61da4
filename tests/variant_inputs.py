"""Inputs for the tests of the three reductions over variant tables [V, L, ld] (tmpnn_select_variant_hits, tmpnn_pair_map,
tmpnn_beam_step) that make their float work decide places: tables of finite floats whose sums and differences ROUND, a counted handful
of special sums planted at candidate sites, tables of arbitrary bit patterns, the cases built from them, and the conditions on such
inputs that keep a test from passing while it tests nothing. The counterpart of tests/hits_inputs.py; shared by
tests/test_variant_inputs_host.py and tests/test_gpu_variant_rounding.py, which therefore see the same inputs; no GPU, no torch.

Every condition here is computed from the inputs and the numpy restatements alone, never from device output."""
from itertools import combinations

import numpy as np

import hits_inputs
from beam_restatement import beam_step_reference, pack_sub
from pair_hits_restatement import CYS, MAX_TAG, variant_hits_reference
from pair_map_restatement import pair_map_reference

EXP_LO, EXP_HI = 118, 134                   # exponent fields of a rounding table: magnitudes 2^-9 .. 2^8
NEG_NAN_QUIET, NEG_NAN_ONES, SNAN = hits_inputs.NEG_NAN_QUIET, hits_inputs.NEG_NAN_ONES, hits_inputs.SNAN
TINY_BASE = 0x80800001                      # -(2^-126)(1 + 2^-23): with the entries below its sums are -1, 0, 1 and 2 denormal ulps
TINY_ENTRIES = (0x00800000, 0x00800001, 0x00800002, 0x00800003)
HUGE = np.float32(3e38)                     # HUGE + HUGE overflows
TOP_LIMIT_K = 32                            # the smallest k >= 32 of the sweeps: at most a quarter of it may be specials that lead


def _finite_bits(rng, shape):
    sign = rng.integers(0, 2, size=shape, dtype=np.uint64) << np.uint64(31)
    expo = rng.integers(EXP_LO, EXP_HI + 1, size=shape, dtype=np.uint64) << np.uint64(23)
    return np.ascontiguousarray((sign | expo | rng.integers(0, 1 << 23, size=shape, dtype=np.uint64)).astype(np.uint32)).view(np.float32)


def rounding_table(V, L, seed, ld=21):
    """-> ddg [V, L, ld], base [V], wt [L, ld]: finite float32 assembled from bits (random sign, exponent field uniform in 118 .. 134,
    random 23-bit mantissa) and handed over by a view. Sums and differences of two such values are exact in float64 and mostly not in
    float32, and a sum of many depends on its order."""
    rng = np.random.default_rng(seed)
    return _finite_bits(rng, (V, L, ld)), _finite_bits(rng, (V,)), _finite_bits(rng, (L, ld))


def hostile_table(V, L, seed, ld=21):
    """-> ddg [V, L, ld], base [V]: hits_inputs.bits_table — arbitrary 32-bit patterns, NaNs of every kind, denormals, zeros, -inf.
    For NaN and ordering robustness, not for rounding."""
    return hits_inputs.bits_table(V * L, ld, seed).reshape(V, L, ld), hits_inputs.bits_table(V, 1, seed + 1).reshape(V)


def inexact(a, b, minus=False):
    """Whether the float32 sum (difference) of a and b differs from the float64 one of the same operands (exact for rounding tables)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s32 = (a - b) if minus else (a + b)
        s64 = (a.astype(np.float64) - b.astype(np.float64)) if minus else (a.astype(np.float64) + b.astype(np.float64))
        return s32.astype(np.float64) != s64                 # (a NaN sum counts as inexact; no condition leans on that)


def rounded_once(a, b, minus=False):
    """The float64 sum (difference) rounded once to float32: an independent statement of the one IEEE operation (innocuous double
    rounding: 53 >= 2 x 24 + 2)."""
    with np.errstate(invalid="ignore", over="ignore"):                        # (a signalling NaN is quieted by the cast)
        a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
        return ((a - b) if minus else (a + b)).astype(np.float32)


# ---- specials ---------------------------------------------------------------------------------------------------------------------
def plant_specials(ddg, base, S_var, variants, rows, blocked=None, blocked_always=False):
    """Overwrites a counted handful of sites of the eight ``variants`` (in place: entries of ddg, base of five of them, and S_var
    where a site had no residue) so that each special sum occurs at a candidate site under every flag: a letter that is neither
    cysteine nor the variant's own, at the first of ``rows`` that ``blocked`` [V, L] (skipped or mutated positions) leaves open.
      variants[0]  entries -inf and +inf                                        sums -inf, +inf
      variants[1]  base +inf, an entry -inf                                     +inf + -inf: a NaN from operands that are not
      variants[2]  base +3e38, entries +3e38 and -3e38                          an overflow to +inf from finite operands; +0.0
      variants[3]  base -3e38, one entry -3e38, the row's others +3e38          an overflow to -inf; -base exactly: +0.0. Its other
                   rows lose their residue (S_var = 20): every sum of theirs would lead the list (rows that are blocked
                   under every flag, ``blocked_always``, keep theirs)
      variants[4]  entries -base and its two neighbours                         +0.0 and one ulp of base to either side
      variants[5]  base -0.0, an entry -0.0                                     -0.0 + -0.0 = -0.0
      variants[6]  base 0x80800001, entries 0x00800000 .. 0x00800003            non-zero DENORMAL sums (and one +0.0)
      variants[7]  a negative quiet NaN, the all-ones NaN, a signalling NaN     no candidate
    -> dict(sites=[(v, q, b, kind)], n_top): n_top counts the sites that lead every ordinary sum in a right or a subtly wrong kernel
    (-inf, the overflow to -inf, the two negative NaNs); it is at most TOP_LIMIT_K / 4, so the specials never fill a list."""
    V, L = S_var.shape
    blocked = np.zeros((V, L), bool) if blocked is None else blocked
    sites = []
    bits = ddg.view(np.uint32)

    def place(v, kinds_and_bits, fill=None):
        q = next(r for r in rows if not blocked[v, r])
        if not 0 <= S_var[v, q] < 20:
            S_var[v, q] = 7
        free = [b for b in range(2, 20) if b != S_var[v, q]]
        if fill is not None:
            bits[v, q, :] = fill
        for b, (kind, pattern) in zip(free, kinds_and_bits):
            bits[v, q, b] = pattern
            sites.append((int(v), int(q), int(b), kind))
        return q

    def pat(x):
        return int(np.float32(x).view(np.uint32))

    a, bn, c, d, e, f, g, h = (int(v) for v in variants)
    place(a, [("-inf", 0xff800000), ("+inf", 0x7f800000)])
    base[bn] = np.inf
    place(bn, [("inf-inf", 0xff800000)])
    base[c] = HUGE
    place(c, [("overflow+", pat(HUGE)), ("zero", pat(-HUGE))])
    base[d] = -HUGE
    q = place(d, [("overflow-", pat(-HUGE))], fill=pat(HUGE))
    keep = blocked[d].copy() if blocked_always else np.zeros(L, bool)
    keep[q] = True
    S_var[d, ~keep] = 20
    minus = np.float32(-base[e])
    place(e, [("zero", pat(minus)), ("ulp", pat(np.nextafter(minus, np.float32(np.inf)))), ("ulp", pat(np.nextafter(minus, np.float32(-np.inf))))])
    base[f] = -0.0
    place(f, [("-0.0", 0x80000000)])
    base.view(np.uint32)[g] = TINY_BASE
    place(g, [("denormal", TINY_ENTRIES[0]), ("zero", TINY_ENTRIES[1]), ("denormal", TINY_ENTRIES[2]), ("denormal", TINY_ENTRIES[3])])
    place(h, [("nan", NEG_NAN_QUIET), ("nan", NEG_NAN_ONES), ("nan", SNAN)])
    n_top = sum(kind in ("-inf", "overflow-") for *_, kind in sites) + 2
    assert n_top <= TOP_LIMIT_K // 4
    return dict(sites=sites, n_top=n_top)


def assert_specials_are_candidates(ddg, base, S_var, planted, blocked=None):
    """Every planted special sits at a candidate site whatever the flags (a letter, not cysteine, not the variant's own residue, not
    blocked), and together they produce a denormal non-zero sum, an overflow from finite operands, an inf - inf NaN and a -0.0 sum."""
    seen = set()
    for v, q, b, kind in planted["sites"]:
        assert 0 <= S_var[v, q] < 20 and b != S_var[v, q] and b != CYS and 0 <= b < 20, (v, q, b, kind)
        assert blocked is None or not blocked[v, q], (v, q, kind)
        x, y = np.float32(base[v]), np.float32(ddg[v, q, b])
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.float32(x + y)
        sb = int(s.view(np.uint32))
        if 0 < (sb & 0x7fffffff) < 0x00800000:
            seen.add("denormal")
        if np.isinf(s) and np.isfinite(x) and np.isfinite(y):
            seen.add("overflow")
        if np.isnan(s) and np.isinf(x) and np.isinf(y):
            seen.add("inf-inf")
        if sb == 0x80000000:
            seen.add("-0.0")
        if np.isnan(y) and sb >> 31:
            seen.add("negative NaN sum")
    assert seen == {"denormal", "overflow", "inf-inf", "-0.0", "negative NaN sum"}, seen


def assert_table_rounds(ddg, base, least=0.5):
    """At least half of the sums base[v] + ddg[v, q, b] of a rounding table are inexact."""
    share = inexact(base[:, None, None], ddg[:, :, :20]).mean()
    assert share >= least, share
    return share


# ---- the hit lists ----------------------------------------------------------------------------------------------------------------
HITS_KS = tuple(sorted(set(hits_inputs.NETWORK_KS) | {1, 256}))             # m = 2, 2, 4, 4, 8, 16, 32, 32, 64, 64, 128, 128, 256 x 3
SPECIAL_VARIANTS = (3, 8, 13, 18, 22, 27, 31, 35)
SPECIAL_ROWS = (255, 256, 299, 44)                                            # the ends of both blocks of 256 residues first


def hits_flags(i):
    """The flags of the i-th k of a sweep: include_cys alternates and upper is its opposite, so both values of both occur at every
    width that two k reach."""
    return dict(include_cys=bool(i & 1), upper=not (i & 1))


def hits_case(V, L, seed, ld=21, table="rounding"):
    """dict(ddg, S_var, base, tag, skip) as Engine.select_variant_hits takes them."""
    rng = np.random.default_rng(seed + 1000)
    ddg, base = rounding_table(V, L, seed, ld)[:2] if table == "rounding" else hostile_table(V, L, seed, ld)
    S_var = rng.integers(-2, 22, size=(V, L)).astype(np.int32)                # 20, 21: no residue; negative letters
    tag = rng.permutation(MAX_TAG + 1)[:V].astype(np.int32)
    skip = rng.integers(-1, L, size=V).astype(np.int32)
    return dict(ddg=ddg, S_var=S_var, base=base, tag=tag, skip=skip)


def hits_rounding_cases():
    """-> (dense, sparse, planted). dense: V = 37 variants of L = 300 rows (the tail block has 44) on a rounding table with the
    specials planted; its winners are -inf and large negative sums that round. sparse: the same tables with a residue left only at the
    specials' rows of their variants — fewer than 256 candidates, so a full-width list shows EVERY sum, the denormal, zero and +inf
    ones too, and a cutoff parts it."""
    c = hits_case(37, 300, 11)
    c["tag"][[0, 1]] = 0, MAX_TAG
    c["skip"][list(SPECIAL_VARIANTS)] = np.minimum(c["skip"][list(SPECIAL_VARIANTS)], 200)
    c["skip"][[0, 1]] = -1, 299
    blocked = np.arange(300)[None, :] <= c["skip"][:, None]                   # (upper: q > skip; without it q != skip, which is less)
    planted = plant_specials(c["ddg"], c["base"], c["S_var"], SPECIAL_VARIANTS, SPECIAL_ROWS, blocked)
    planted["blocked"] = blocked
    sparse = dict(c, S_var=np.full_like(c["S_var"], 20))
    for v, q, _, _ in planted["sites"]:
        sparse["S_var"][v, q] = c["S_var"][v, q]
    return c, sparse, planted


def hits_hostile_case():
    """V = 12 variants of L = 70 rows of arbitrary bit patterns. skip is L - 1 or L - 2, so under `upper` a variant has one row or none
    and the longer lists run short."""
    c = hits_case(12, 70, 21, table="hostile")
    c["skip"] = (70 - 1 - np.arange(12) % 2).astype(np.int32)
    return c


def hits_cap_case(m):
    """L = 3 and V = 8192 / m + 5 variants: V items against W = 8192 / m - 1 workgroups, so six workgroups take a second trip. The six
    best values sit in the LAST six variants."""
    V = 8192 // m + 5
    c = hits_case(V, 3, 40 + m)
    c["S_var"][V - 6:, 1], c["skip"][V - 6:] = 5, -1
    c["ddg"][V - 6:, 1, 9] = np.float32(-1000.37) - np.float32(3.1) * np.arange(6, dtype=np.float32)
    return c


def hits_ref(c, k, sl=slice(None), state=None, **kw):
    return variant_hits_reference(c["ddg"][sl], c["S_var"][sl], c["base"][sl], c["tag"][sl], c["skip"][sl], k, kw.get("cutoff"),
                                  kw.get("include_cys", False), kw.get("upper", False), state)


def winners_inexact(c, ref):
    """[hit_count] bool: whether each winner's sum is inexact (the winner found again by its tag, position and letter)."""
    n = int(ref["hit_count"][0])
    v_of = {int(t): v for v, t in enumerate(c["tag"])}
    v = np.array([v_of[int(t)] for t in ref["hit_tag"][:n]], dtype=np.int64)
    return inexact(c["base"][v], c["ddg"][v, ref["hit_pos"][:n], ref["hit_aa"][:n]])


# ---- the pair map -----------------------------------------------------------------------------------------------------------------
PMAP_V, PMAP_R = 37, 6


def plant_epistasis_specials(ddg, wt, S_var, variants, q, alone):
    """At row ``q`` of five ``variants`` (in place): e = ddg - wt of +inf, -inf, NaN (inf - inf, neither operand NaN), -0.0 (-0.0 - +0.0)
    and a negative NaN entry. At row ``q + 1`` of the variants ``alone`` (each a run of its own in some row layout) every entry is
    wt + |x|, so every e is positive, and one is a DENORMAL difference of two tiny normals: the smallest e of its state entry, which
    eps_lo therefore holds. -> [(v, q, b, kind)]."""
    sites = []
    db, wb = ddg.view(np.uint32), wt.view(np.uint32)
    for v, row in [(v, q) for v in variants] + [(v, q + 1) for v in alone]:
        if not 0 <= S_var[v, row] < 20:
            S_var[v, row] = 7
    for i, (kind, x, w) in enumerate((("+inf", 0x7f800000, None), ("-inf", 0xff800000, None), ("inf-inf", 0x7f800000, 0x7f800000),
                                      ("-0.0", 0x80000000, 0x00000000), ("nan", NEG_NAN_ONES, None))):
        v = int(variants[i])
        b = 2 + 3 * i                                                         # one column each: wt is shared by all variants
        while b == S_var[v, q]:
            b += 1
        db[v, q, b] = x
        if w is not None:
            wb[q, b] = w
        sites.append((v, int(q), b, kind))
    b = next(b for b in range(2, 20) if all(b != S_var[v, q + 1] for v in alone))
    wb[q + 1, b] = 0x00800001
    for v in alone:
        ddg[v, q + 1, :20] = wt[q + 1, :20] + np.abs(ddg[v, q + 1, :20])
        db[v, q + 1, b] = 0x00800003
        sites.append((int(v), int(q) + 1, b, "denormal"))
    return sites


def pmap_case(V, L, seed, ld=21, specials=True):
    """dict(ddg, wt, base, S_var, letter, skip) on rounding tables, every variant live unless a test says otherwise."""
    rng = np.random.default_rng(seed + 2000)
    ddg, base, wt = rounding_table(V, L, seed, ld)
    c = dict(ddg=ddg, wt=wt, base=base, S_var=rng.integers(-2, 22, size=(V, L)).astype(np.int32),
             letter=rng.integers(0, 20, size=V).astype(np.int32), skip=rng.integers(-1, L, size=V).astype(np.int32))
    if specials:
        q = L // 2
        variants, alone = (1, 7, 12, 21, 33), (0, V - 1)                      # (the first and the last variant: runs of one in ROWS_A / _B)
        c["skip"][list(variants + alone)] = -1
        c["letter"][list(alone)] = 0, 19
        c["sites"] = plant_epistasis_specials(ddg, wt, c["S_var"], variants, q, alone)
    return c


def pmap_crafted():
    """{(L, ld): the 37 variants} for L = 19, 70 and ld = 20, 21, as the sibling file's, on rounding tables with the epistasis specials."""
    out = {}
    for L, ld in ((19, 21), (19, 20), (70, 21), (70, 20)):
        c = pmap_case(PMAP_V, L, L + ld, ld)
        c["letter"][[3, 20, 30]] = 20, -1, 35                                 # out of range: these variants contribute nothing
        c["skip"][[2, 4, 5]] = 0, L - 1, L - 1
        out[L, ld] = c
    return out


def pmap_short_cases():
    """{L: (case, rows, R)} for L = 1, 2, 255, 256, 257: a 256-row tile spans many variants and (q0 + r) % L wraps many times, or the
    tile borders creep through the variants. V L is no multiple of 256 except at L = 256, where no V can make it so. Every variant
    is live; one skip is 0 and one is L - 1."""
    out = {}
    for L in (1, 2, 255, 256, 257):
        V = 300 if L <= 2 else 3
        c = pmap_case(V, L, 50 + L, specials=False)
        c["S_var"] = np.random.default_rng(L).integers(0, 20, size=(V, L)).astype(np.int32)
        c["skip"][:] = -1
        c["skip"][[0, 1]] = 0, L - 1
        rows = np.repeat([2, 0, 1], [100, 150, 50] if V == 300 else [1, 1, 1]).astype(np.int32)
        assert (V * L) % 256 != 0 or L == 256
        out[L] = (c, rows, 4)
    return out


def pmap_long_run_case():
    """L = 5, V = 612: one state row named by 600 consecutive variants between two runs of one variant each; the last 10 variants fall
    in a second row. -> (case, rows, R)."""
    c = pmap_case(612, 5, 77, specials=False)
    rows = np.repeat([2, 0, 3, 1], [1, 600, 1, 10]).astype(np.int32)
    return c, rows, 4


def pmap_ref(c, rows, R, sl=slice(None), state=None, **kw):
    return pair_map_reference(c["ddg"][sl], c["S_var"][sl], c["base"][sl], rows[sl], c["letter"][sl],
                              None if kw.get("no_skip") else c["skip"][sl], c["wt"], R, kw.get("include_cys", False), kw.get("upper", False), state)


def pmap_inner(c, **kw):
    """-> (inner sums [V, L] float32, counts [V, L]): every variant in a state row of its own (+0.0 + x = x)."""
    V = c["S_var"].shape[0]
    one = pmap_ref(c, np.arange(V, dtype=np.int32), V, **kw)
    return one["eps_abs_sum"], one["count"]


def pmap_reversed_b(c):
    """The case with its 20 letter columns mirrored (b -> 19 - b; cysteine's column made NaN so that the mirror needs no cysteine
    rule): the restatement on it, with include_cys, sums |e| in DESCENDING b over the same candidates as without include_cys on c."""
    m = dict(c, ddg=c["ddg"].copy(), wt=c["wt"].copy())
    m["ddg"][:, :, CYS] = np.nan
    m["ddg"][:, :, :20], m["wt"][:, :20] = m["ddg"][:, :, 19::-1].copy(), m["wt"][:, 19::-1].copy()
    m["S_var"] = np.where((c["S_var"] >= 0) & (c["S_var"] < 20), 19 - c["S_var"], c["S_var"]).astype(np.int32)
    return m


def assert_pair_map_order_shows(c, rows, R, runs=True, **kw):
    """The restatement with b summed in descending order differs in bits at >= 25 % of the live (v, q) inner sums, and with v folded
    in descending order at >= 25 % of the state entries that have runs of >= 2 variants. -> the two shares."""
    assert not kw.get("include_cys")
    inner, cnt = pmap_inner(c, **kw)
    mirrored, cnt_m = pmap_inner(pmap_reversed_b(c), **dict(kw, include_cys=True))
    np.testing.assert_array_equal(cnt, cnt_m)
    live = cnt >= 2
    share_b = (inner.view(np.uint32) != mirrored.view(np.uint32))[live].mean()
    assert live.sum() >= 20 and share_b >= 0.25, share_b
    fwd = pmap_ref(c, rows, R, **kw)
    back = pmap_ref({k: (v[::-1] if k not in ("wt", "sites") else v) for k, v in c.items()}, rows[::-1], R, **kw)
    np.testing.assert_array_equal(fwd["count"], back["count"])
    np.testing.assert_array_equal(fwd["best"], back["best"])
    terms = np.zeros_like(fwd["count"])
    for v in range(len(rows)):
        if 0 <= rows[v] < R:
            terms[rows[v]] += cnt[v] > 0
    busy = terms >= 2
    if not runs:                                                              # (a case whose runs are single variants has no fold order)
        assert not busy.any()
        return share_b, None
    share_v = (fwd["eps_abs_sum"].view(np.uint32) != back["eps_abs_sum"].view(np.uint32))[busy].mean()
    assert busy.any() and share_v >= 0.25, share_v
    return share_b, share_v


# ---- the beam ---------------------------------------------------------------------------------------------------------------------
BEAM_PAIRS = ((1, 2), (2, 2), (2, 4), (3, 5), (4, 8), (7, 9), (2, 64), (8, 32), (3, 85), (2, 125), (7, 36))   # m = 2 .. 256, 256 x 3
BEAM_POOL = {1: 7, 2: 7, 3: 7, 4: 7, 7: 7, 8: 8}                              # depth -> pool size: 1, 7, 21, 35, 7, 8 members
BEAM_SEED = {1: 1, 2: 2, 3: 3, 4: 4, 7: 7, 8: 8}


def _distinct_members(rng, muts, S_var, first, free_rows, depth, taken):
    for v in range(first, len(muts)):
        while True:
            pos = np.sort(rng.choice(free_rows, size=depth - 1, replace=False))
            let = rng.integers(0, 20, size=depth - 1)
            if tuple(pack_sub(pos, let)) not in taken:
                break
        taken.add(tuple(pack_sub(pos, let)))
        S_var[v, pos] = let
        muts[v] = pack_sub(pos, let)


def rounding_beam(depth, L=40, seed=None, extra=10, specials=True):
    """A beam on rounding tables whose pool children collide by ``depth`` paths, a different inexact sum on each: the layout of
    beam_restatement.duplicate_fixture. The first members are ALL (depth - 1)-subsets of a pool of n substitutions with weights
    w_z = -|x_z| - 8; a pool member's score is the float32 chain sum of its weights, and every table is |x| (nothing below zero) except,
    in a pool member, at each pool site z it lacks, which holds w_z with its low 12 mantissa bits redrawn — so the heaviest pool
    children lead every list among the other children of the heavy members (sums that round too), and the d paths to one child set give d nearly equal sums that round differently and lie side by side in the order.
    ``extra`` unrelated distinct members follow (scores |x|), eight of them carrying the specials; the first of them is made the second parent of the child that the planted
    -inf entry makes, so the very top of the list is one set by two paths, both -inf. -> dict(ddg, S_var, score, muts, depth, pool, planted, blocked)."""
    n_pool = BEAM_POOL[depth]
    rng = np.random.default_rng(3000 + (BEAM_SEED[depth] if seed is None else seed))
    members = list(combinations(range(n_pool), depth - 1))
    V = len(members) + (extra if depth > 1 else 0)
    ddg, score, _ = rounding_table(V, L, 3000 + depth if seed is None else seed)
    sites = np.linspace(0, L - 1, n_pool).astype(np.int64)                    # the first and the last row among them
    assert len(set(sites.tolist())) == n_pool
    letters = np.array([(3 + 2 * i) % 20 for i in range(n_pool)], np.int64)   # none is cysteine
    weight = (-np.abs(_finite_bits(rng, (n_pool,))) - np.float32(8)).astype(np.float32)
    S_var = rng.integers(-2, 22, size=(V, L)).astype(np.int32)
    muts = np.zeros((V, depth - 1), np.int32)
    ddg = np.abs(ddg)                                                         # nothing below zero but the pool's entries and the specials
    for v, mem in enumerate(members):
        S_var[v, sites] = (letters + 1 + rng.integers(0, 18, size=n_pool)) % 20             # a letter, and not the pool's
        S_var[v, sites[list(mem)]] = letters[list(mem)]
        muts[v] = pack_sub(sites[list(mem)], letters[list(mem)])
        total = np.float32(0.0)
        for z in mem:
            total = np.float32(total + weight[z])
        score[v] = total
        for z in range(n_pool):
            if z not in mem:
                wbits = (int(weight[z].view(np.uint32)) & ~0xfff) | int(rng.integers(0, 1 << 12))
                ddg.view(np.uint32)[v, sites[z], letters[z]] = wbits
    score[len(members):] = np.abs(score[len(members):])
    free = np.setdiff1d(np.arange(L), sites)
    if depth > 1:
        _distinct_members(rng, muts, S_var, len(members), free, depth, set())
    blocked = np.zeros((V, L), bool)
    for col in range(depth - 1):
        blocked[np.arange(V), muts[:, col] >> 5] = True
    planted = None
    if specials and depth > 1:
        rows = [int(r) for r in free[::-1]]
        first = len(members)                                                  # member `first` becomes the second parent of the -inf child
        planted = plant_specials(ddg, score, S_var, range(first + 1, first + 9), rows, blocked, blocked_always=True)
        v, q, b, kind = planted["sites"][0]
        assert kind == "-inf"
        if muts[v, 0] & 31 == CYS:
            muts[v, 0] += 1
            S_var[v, muts[v, 0] >> 5] = muts[v, 0] & 31
        lacks = int(muts[v, 0])                                               # `first` = that member's child less its first substitution
        muts[first] = np.sort(np.concatenate([muts[v, 1:], [q << 5 | b]]))
        S_var[first, muts[first] >> 5] = muts[first] & 31
        S_var[first, lacks >> 5] = (lacks & 31) + 1 if (lacks & 31) < 19 else 0
        ddg[first, lacks >> 5, lacks & 31] = -np.inf
        blocked[first] = False
        blocked[first, muts[first] >> 5] = True
        alive = [tuple(m) for m in muts.tolist()]
        assert len(set(alive)) == len(alive)
    return dict(ddg=ddg, S_var=S_var, score=score, muts=muts if depth > 1 else None, depth=depth,
                pool=set(int(x) for x in pack_sub(sites, letters)), planted=planted, blocked=blocked)


def sparse_beam(fx):
    """(fixture, allowed) in which only the specials' own sites are open and have a residue: fewer candidates than any k >= 64, so the
    result shows EVERY sum, the denormal and zero ones too."""
    S_var = fx["S_var"].copy()
    L = S_var.shape[1]
    allowed = np.zeros(L, np.int32)
    mine = np.zeros(S_var.shape, bool)
    for v, q, _, _ in fx["planted"]["sites"]:
        allowed[q], mine[v, q] = 1, True
    S_var[(allowed != 0)[None, :] & ~mine] = 20
    return dict(fx, S_var=S_var), allowed


def beam_cap_case(k, V, L):
    """d = 2 at the workgroup cap: V members (V items at L <= 256) against W = 8192 / pow2(2 k) - 1 workgroups. The members are the
    singles of a pool of three and distinct unrelated singles (L x 20 >= V: L = 3 cannot hold V distinct sets); the best children sit
    in the LAST members."""
    rng = np.random.default_rng(5000 + k)
    ddg, score, _ = rounding_table(V, L, 5000 + k)
    S_var = rng.integers(0, 20, size=(V, L)).astype(np.int32)
    muts = np.zeros((V, 1), np.int32)
    taken = set()
    pool_rows, pool_letters = np.array([0, L // 2, L - 1]), np.array([3, 5, 7])
    weight = np.array([-300.3, -280.7, -260.1], np.float32)
    for v in range(3):
        ddg[v] = np.abs(ddg[v])
        muts[v, 0] = pack_sub(pool_rows[v], pool_letters[v])
        S_var[v, pool_rows] = (pool_letters + 1 + v) % 20
        S_var[v, pool_rows[v]] = pool_letters[v]
        score[v] = weight[v]
        taken.add((int(muts[v, 0]),))
        for z in range(3):
            if z != v:
                ddg[v, pool_rows[z], pool_letters[z]] = weight[z] + np.float32(rng.integers(0, 64)) * np.float32(2.0 ** -18)
    _distinct_members(rng, muts, S_var, 3, np.arange(L), 2, taken)
    assert len({int(e) for e in muts[:, 0]}) == V
    for i, v in enumerate(range(V - 6, V)):                                   # about -702 to -710: below the pool's children, which are
        q = (int(muts[v, 0] >> 5) + 1) % L                                    # below every other sum (>= -512)
        S_var[v, q] = 11
        score[v] = np.float32(-1.7) - np.float32(0.3) * np.float32(i)
        ddg[v, q, 4] = np.float32(-700.6) - np.float32(1.3) * np.float32(i)
    return dict(ddg=ddg, S_var=S_var, score=score, muts=muts, depth=2)


def hostile_beam():
    """d = 2, V = 12 members of L = 70 rows on arbitrary bit patterns, scores too; distinct singles, letters on both sides of 0 .. 19."""
    ddg, score = hostile_table(12, 70, 61)
    rng = np.random.default_rng(62)
    S_var = rng.integers(-2, 23, size=(12, 70)).astype(np.int32)
    muts = np.zeros((12, 1), np.int32)
    _distinct_members(rng, muts, S_var, 0, np.arange(70), 2, set())
    return dict(ddg=ddg, S_var=S_var, score=score, muts=muts, depth=2)


def beam_ref(fx, k, **kw):
    return beam_step_reference(fx["ddg"], fx["S_var"], fx["score"], fx["muts"], fx["depth"], k, kw.get("allowed"), kw.get("cutoff"),
                               kw.get("include_cys", False))


def beam_winners_inexact(fx, ref):
    """[out_count] bool: whether each kept child's sum is inexact (the path that represents it: its parent and the substitution the
    parent lacks)."""
    n = int(ref["out_count"][0])
    out = np.zeros(n, bool)
    for r in range(n):
        v = int(ref["out_parent"][r])
        own = set() if fx["muts"] is None else set(int(e) for e in fx["muts"][v])
        (add,) = set(int(e) for e in ref["out_muts"][r]) - own
        out[r] = inexact(fx["score"][v], fx["ddg"][v, add >> 5, add & 31])
    return out
