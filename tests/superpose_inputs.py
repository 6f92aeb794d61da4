"""Fixtures for tmpnn_superpose, shared by tests/test_superpose_host.py and tests/test_gpu_superpose.py, which therefore see the same
coordinates; no GPU, no torch. Random-walk C-alpha chains of 3.8 A steps stored as fp32, centroids up to 500 A from the origin; the
members of an ensemble are rotated and translated copies of its chain with coordinate noise of 0, 0.3 and 2.0 A in turn. The other
three atom slots of X hold NaN in every fourth row: the entry reads slot 1 only. degenerate(): the fits whose rotation is not unique
or nearly so, and structurally special ones, for tests/test_gpu_superpose_degenerate.py; centroids out to 9 000 A."""
import numpy as np

SHAPES = ((1, 19), (2, 3), (3, 70), (17, 257), (5, 1025), (0, 5), (300, 19))   # (M, L): L = 257 and 1 025 leave one column to a second
FIT_TO = (0, 1, 2, 0, 4, 0, 150)                                               # and a fifth round of the 256 threads; M = 300: many slots
NOISE = (0.0, 0.3, 2.0)
INT32_MIN = -2 ** 31


def chain(L, rng, centre=500.0):
    """[L, 3] float64: a random walk of 3.8 A steps whose first point is up to ``centre`` A from the origin."""
    steps = rng.standard_normal((L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    start = rng.standard_normal(3)
    return np.cumsum(steps, axis=0) + start / np.linalg.norm(start) * centre * rng.uniform(0.2, 1.0)


def rotation(rng):
    w, x, y, z = (q := rng.standard_normal(4)) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def moved(P, rng, noise, shift=30.0):
    """A rotated (about the chain's centroid) and translated copy of P with Gaussian coordinate noise of ``noise`` A."""
    c = P.mean(axis=0)
    return (P - c) @ rotation(rng).T + c + rng.standard_normal(3) * shift + rng.standard_normal(P.shape) * noise


def backbone(ca, rng):
    """C-alpha [n, 3] -> X [n, 4, 3] float32: slot 1 is the C-alpha, the others lie near it, NaN in every fourth row."""
    X = (ca[:, None, :] + rng.standard_normal((len(ca), 4, 3))).astype(np.float32)
    X[:, 1] = ca.astype(np.float32)
    X[::4, 0] = X[::4, 2] = X[::4, 3] = np.nan
    return X


def pack(shapes, fit_to, mem_gap=0):
    """-> (desc [E, 6] int32, R = T, NM, T_out, max_len): members contiguous and in order, the identity map."""
    desc, at, out, mem = [], 0, 0, 0
    for (M, L), f in zip(shapes, fit_to):
        desc.append((at, M, L, out, mem, f))
        at, out, mem = at + M * L, out + L, mem + M + mem_gap
    return np.array(desc, np.int32).reshape(-1, 6), at, mem, out, max([L for _, L in shapes], default=0)


def crafted(seed=11, shapes=SHAPES, fit_to=FIT_TO, holes=True):
    """One batch of ``shapes``: dict(X [T, 4, 3], mask [T], rows: the identity map [R = T], desc, R, T, NM, T_out, max_len, members,
    lengths, fit_to, coord: the largest |coordinate|). ``holes``: in ensembles of L >= 19 about one row in 16 is masked (mask 0, -1 or
    NaN) and a few C-alphas hold NaN or inf."""
    rng = np.random.default_rng(seed)
    desc, T, NM, T_out, max_len = pack(shapes, fit_to)
    ca = np.zeros((T, 3))
    for (M, L), d in zip(shapes, desc):
        base = chain(L, rng)
        for m in range(M):
            ca[d[0] + m * L:d[0] + (m + 1) * L] = moved(base, rng, NOISE[m % 3])
    X = backbone(ca, rng)
    coord = float(np.abs(X[:, 1]).max()) if T else 0.0
    mask = np.ones(T, np.float32)
    if holes:
        for (M, L), d in zip(shapes, desc):
            if L < 19:
                continue
            at = np.arange(d[0], d[0] + M * L)
            off = at[rng.random(len(at)) < 1 / 16]
            mask[off] = rng.choice(np.array([0.0, -1.0, np.nan], np.float32), size=len(off))
            bad = at[rng.random(len(at)) < 1 / 64]
            X[bad, 1, rng.integers(0, 3, size=len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=len(bad))
    return dict(X=X, mask=mask, rows=np.arange(T, dtype=np.int32), desc=desc, R=T, T=T, NM=NM, T_out=T_out, max_len=max_len,
                members=[M for M, _ in shapes], lengths=[L for _, L in shapes], fit_to=list(fit_to), coord=coord)


def long_pair(seed=5):
    """One ensemble of 2 members of 8 192 columns, the longest the entry serves: 32 rounds of the 256 threads."""
    return crafted(seed, shapes=((2, 8192),), fit_to=(1,))


def drawn_map(c, rng):
    """A copy of batch c's identity map with about one entry in 12 replaced by -1, T, T + 5 or INT32_MIN (the member is out there),
    and, in the (3, 70) ensemble, member 1 naming member 0's rows: two members on the same rows."""
    rows = c["rows"].copy()
    off = rng.random(len(rows)) < 1 / 12
    rows[off] = rng.choice(np.array([-1, c["T"], c["T"] + 5, INT32_MIN], np.int64), size=int(off.sum())).astype(np.int32)
    for d in c["desc"]:
        if (d[1], d[2]) == (3, 70):
            rows[d[0] + 70:d[0] + 140] = rows[d[0]:d[0] + 70]
    return rows


def subset(c, which, mem_gap=3):
    """The ensembles ``which`` of batch c, in that order, as a batch of their own over the SAME X, mask and map (so map0 stays), with
    other output rows and other member slots (``mem_gap`` unused slots between the ensembles) -> (batch, member slots [k] and output
    rows [k] of c that the new batch's slots and rows correspond to, as index arrays: new -> old; -1 for the unused slots)."""
    desc, out, mem, slots, cols = [], 0, 0, [], []
    for e in which:
        map0, M, L, out0, mem0, f = (int(v) for v in c["desc"][e])
        desc.append((map0, M, L, out, mem, f))
        slots += list(range(mem0, mem0 + M)) + [-1] * mem_gap
        cols += list(range(out0, out0 + L))
        out, mem = out + L, mem + M + mem_gap
    b = dict(c, desc=np.array(desc, np.int32).reshape(-1, 6), NM=mem, T_out=out, max_len=max([c["lengths"][e] for e in which], default=0))
    return b, np.array(slots, np.int64), np.array(cols, np.int64)


def special(seed=23):
    """The special cases in one batch, through an explicit map. Ensembles (member 0 is the fit target unless said):
      0  (7, 12)  the target is masked at columns 0 and 1. Member 1 is valid at columns 0, 1 only: 0 in common; members 2, 3, 4 at 1, 2
                  and 3 further columns: n_fit 1, 2, 3; member 5 has no valid row at all (its map is -1); member 6 is whole
      1  (4, 40)  fit_to = 3. Member 0 names the target's rows (an exact copy through the map), member 1 holds the same coordinates in
                  rows of its own, member 2 is a mirror image (x -> -x) moved elsewhere
      2  (2, 3)   three collinear points: no unique rotation (``loose``)
    -> the batch dict plus loose: member slots without a unique rotation, loose_ensembles: their ensembles."""
    rng = np.random.default_rng(seed)
    shapes, fit_to = ((7, 12), (4, 40), (2, 3)), (0, 3, 0)
    desc, T, NM, T_out, max_len = pack(shapes, fit_to)
    ca = np.zeros((T, 3))
    for (M, L), d in zip(shapes, desc):
        base = chain(L, rng)
        for m in range(M):
            ca[d[0] + m * L:d[0] + (m + 1) * L] = moved(base, rng, 0.3)
    d1 = int(desc[1][0])
    ca[d1 + 40:d1 + 80] = ca[d1 + 120:d1 + 160]                                        # member 1 = the target's coordinates
    mirror = ca[d1 + 120:d1 + 160] * np.array([-1.0, 1.0, 1.0])
    ca[d1 + 80:d1 + 120] = moved(mirror, rng, 0.0)
    d2 = int(desc[2][0])
    line = np.array([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0], [7.6, 0.0, 0.0]]) @ rotation(rng).T + 40.0
    ca[d2:d2 + 3], ca[d2 + 3:d2 + 6] = line, moved(line, rng, 0.0)
    X = backbone(ca, rng)
    mask = np.ones(T, np.float32)
    rows = np.arange(T, dtype=np.int32)
    mask[0:2] = 0.0                                                                    # the target of ensemble 0, columns 0 and 1
    for m, keep in ((1, (0, 1)), (2, (0, 1, 2)), (3, (0, 1, 2, 3)), (4, (0, 1, 2, 3, 4))):
        gone = np.setdiff1d(np.arange(12), keep)
        rows[m * 12 + gone[::2]] = -1                                                  # out through the map ...
        mask[m * 12 + gone[1::2]] = 0.0                                                # ... and through the mask
    rows[5 * 12:6 * 12] = -1
    rows[d1:d1 + 40] = np.arange(d1 + 120, d1 + 160)
    return dict(X=X, mask=mask, rows=rows, desc=desc, R=T, T=T, NM=NM, T_out=T_out, max_len=max_len, members=[M for M, _ in shapes],
                lengths=[L for _, L in shapes], fit_to=list(fit_to), coord=float(np.abs(X[:, 1]).max()), loose=[NM - 1], loose_ensembles=[2])


DEGENERATE_SIZES = (3, 4, 19, 257)
DEGENERATE_LONG = 1025                                                             # the collinear and the planar families only
LOOSE_FAMILIES = ("collinear", "collinear_noisy", "near_collinear_4", "near_collinear_10", "near_collinear_16", "coincident",
                  "both_coincident", "inverted_cube", "inverted_tetrahedron", "inverted_near_cube_10", "inverted_near_cube_16",
                  "inverted_near_cube_22")
CONDITIONED_FAMILIES = ("half_turn_x", "half_turn_y", "half_turn_z", "half_turn_generic", "far", "inversion", "quarter_turn_z",
                        "translation", "planar_mirror", "planar_mirror_noisy")


def _f32(P):
    """P rounded to fp32 and back: what a member built from ANOTHER member's stored coordinates starts from."""
    return np.asarray(P, np.float64).astype(np.float32).astype(np.float64)


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _line_ensemble(L, rng):
    """The target: L points at 3.8 A steps on a line of generic direction (fp32 storage leaves it collinear to about 2^-16 A). The
    members: a moved copy, one with 0.3 A of noise, and moved copies with transverse offsets of 2^-k A, k = 4, 10, 16."""
    u = _unit(rng)
    line = chain(1, rng) + 3.8 * np.arange(L)[:, None] * u
    members, names = [line, moved(line, rng, 0.0), moved(line, rng, 0.3)], ["target", "collinear", "collinear_noisy"]
    for k in (4, 10, 16):
        across = np.cross(rng.standard_normal((L, 3)), u)
        across *= 2.0 ** -k / np.linalg.norm(across, axis=1, keepdims=True)
        members.append(moved(line + across, rng, 0.0))
        names.append(f"near_collinear_{k}")
    return members, names


def _generic_ensemble(L, rng):
    """The target: a chain. The members: every point the same point; the target's stored coordinates turned by 180 degrees about x, y
    and z (sign changes: exact) and about a generic axis; a copy with 0.3 A of noise whose centroid is 9 000 A out; the inversion of
    the target through its centroid, moved, with 0.3 A of noise."""
    P = _f32(chain(L, rng))
    c = P.mean(axis=0)
    u = _unit(rng)
    far = moved(P, rng, 0.3)
    far += _unit(rng) * 9000.0 - far.mean(axis=0)
    members = [P, np.repeat(chain(1, rng), L, axis=0), P * np.array([1.0, -1.0, -1.0]), P * np.array([-1.0, 1.0, -1.0]),
               P * np.array([-1.0, -1.0, 1.0]), (P - c) @ (2.0 * np.outer(u, u) - np.eye(3)).T + c + rng.standard_normal(3) * 30.0, far,
               moved(2.0 * c - P, rng, 0.3)]
    return members, ["target", "coincident", "half_turn_x", "half_turn_y", "half_turn_z", "half_turn_generic", "far", "inversion"]


def _integer_ensemble(L, rng):
    """The target: a chain rounded to integer coordinates. The members: (x, y, z) -> (-y, x, z) and an integer shift, both exact."""
    P = np.round(chain(L, rng))
    return [P, P[:, [1, 0, 2]] * np.array([-1.0, 1.0, 1.0]), P + np.array([17.0, -230.0, 64.0])], ["target", "quarter_turn_z", "translation"]


def _point_ensemble(L, rng):
    return [np.repeat(_f32(chain(1, rng)), L, axis=0), np.repeat(_f32(chain(1, rng)), L, axis=0)], ["target", "both_coincident"]


def _planar_ensemble(L, rng):
    """The target: a walk of 3.8 A steps in a plane of generic orientation. The members: its mirror image IN that plane (one in-plane
    coordinate negated about the centroid), moved, without noise and with 0.3 A of noise. Turning the plane over undoes the mirror."""
    e1 = _unit(rng)
    e2 = np.cross(e1, _unit(rng))
    e2 /= np.linalg.norm(e2)
    ang = rng.uniform(0.0, 2.0 * np.pi, L)
    uv = np.cumsum(3.8 * np.stack([np.cos(ang), np.sin(ang)], axis=1), axis=0)
    uv -= uv.mean(axis=0)
    centre = chain(1, rng)
    P = centre + uv[:, :1] * e1 + uv[:, 1:] * e2
    Q = centre + uv[:, :1] * e1 - uv[:, 1:] * e2
    return [P, moved(Q, rng, 0.0), moved(Q, rng, 0.3)], ["target", "planar_mirror", "planar_mirror_noisy"]


def _inverted_solid(corners, centre, name):
    """``corners`` (half-edge units, exact in fp32) around ``centre`` and their inversion through the centroid, shifted by integers:
    the centred covariance is diagonal and exact, Horn's matrix is diagonal."""
    P = np.asarray(corners, np.float64) + np.asarray(centre, np.float64)
    return [P, 2.0 * np.asarray(centre, np.float64) - P + (np.array([16.0, 32.0, -48.0]) if any(centre) else 0.0)], ["target", name]


def degenerate(seed=41):
    """Fits whose rotation is not unique or nearly so, and structurally special ones, in one batch through the identity map; no
    holes. One ensemble per (kind of target, size); member 0 is the fit target and every other member belongs to one family.
      line     L = 3, 4, 19, 257, 1 025   collinear, collinear_noisy, near_collinear_{4, 10, 16}
      generic  L = 3, 4, 19, 257          coincident, half_turn_{x, y, z, generic}, far, inversion
      integer  L = 3, 4, 19, 257          quarter_turn_z, translation
      point    L = 3, 4, 19, 257          both_coincident
      planar   L = 3, 4, 19, 257, 1 025   planar_mirror, planar_mirror_noisy
      cube (L = 8), tetrahedron (L = 4), near_cube_{10, 16, 22} (L = 8, edges 1 : 1 + 2^-k : 1 + 2^-k+1, centred at the origin): inverted
    -> the batch dict of crafted() plus ca [T, 3] float32, names [E], family [NM] ('target' for member 0), loose / conditioned: the
    member slots of LOOSE_FAMILIES / CONDITIONED_FAMILIES, loose_ensembles, and ensembles: {kind of target: its ensembles}."""
    rng = np.random.default_rng(seed)
    built = []
    for kind, make, sizes in (("line", _line_ensemble, DEGENERATE_SIZES + (DEGENERATE_LONG,)), ("generic", _generic_ensemble, DEGENERATE_SIZES),
                             ("integer", _integer_ensemble, DEGENERATE_SIZES), ("point", _point_ensemble, DEGENERATE_SIZES),
                             ("planar", _planar_ensemble, DEGENERATE_SIZES + (DEGENERATE_LONG,))):
        built += [(kind, L) + make(L, rng) for L in sizes]
    cube = [(sx, sy, sz) for sx in (-2.0, 2.0) for sy in (-2.0, 2.0) for sz in (-2.0, 2.0)]
    built.append(("cube", 8) + _inverted_solid(cube, (304.0, -208.0, 96.0), "inverted_cube"))
    built.append(("tetrahedron", 4) + _inverted_solid([(2.0, 2.0, 2.0), (2.0, -2.0, -2.0), (-2.0, 2.0, -2.0), (-2.0, -2.0, 2.0)],
                                                      (-176.0, 240.0, 320.0), "inverted_tetrahedron"))
    for k in (10, 16, 22):
        edges = np.array([1.0, 1.0 + 2.0 ** -k, 1.0 + 2.0 ** (1 - k)])
        built.append((f"near_cube_{k}", 8) + _inverted_solid(np.array(cube) * edges, (0.0, 0.0, 0.0), f"inverted_near_cube_{k}"))
    shapes = tuple((len(members), L) for _, L, members, _ in built)
    desc, T, NM, T_out, max_len = pack(shapes, (0,) * len(shapes))
    ca = np.concatenate([np.concatenate(members) for _, _, members, _ in built])
    family = [name for _, _, _, names in built for name in names]
    assert ca.shape == (T, 3) and len(family) == NM and set(family) == set(LOOSE_FAMILIES + CONDITIONED_FAMILIES + ("target",))
    X = backbone(ca, rng)
    ensembles = {}
    for e, (kind, _, _, _) in enumerate(built):
        ensembles.setdefault(kind.rsplit("_", 1)[0] if kind.startswith("near_cube") else kind, []).append(e)
    loose = [g for g, name in enumerate(family) if name in LOOSE_FAMILIES]
    return dict(X=X, mask=np.ones(T, np.float32), rows=np.arange(T, dtype=np.int32), desc=desc, R=T, T=T, NM=NM, T_out=T_out,
                max_len=max_len, members=[M for M, _ in shapes], lengths=[L for _, L in shapes], fit_to=[0] * len(shapes),
                coord=float(np.abs(X[:, 1]).max()), ca=X[:, 1].copy(), names=[f"{kind}:{L}" for kind, L, _, _ in built], family=family,
                loose=loose, conditioned=[g for g, name in enumerate(family) if name in CONDITIONED_FAMILIES],
                loose_ensembles=sorted({e for e, d in enumerate(desc) if set(range(d[4], d[4] + d[1])) & set(loose)}), ensembles=ensembles)


def scaled(c, k):
    """Batch c with every coordinate multiplied by 2^k in fp32 (exact unless it leaves fp32's normal range: the caller checks)."""
    return dict(c, X=(c["X"] * np.float32(2.0 ** k)).astype(np.float32), coord=c["coord"] * 2.0 ** k)


SCALE_ENSEMBLES = ("generic:19", "line:257", "near_cube_10:8", "near_cube_16:8", "near_cube_22:8")
SCALE_K = (-60, -20, 20, 60)


def scale_subset(c):
    """The ensembles of degenerate() that the power-of-two tests run, as a batch of their own -> (batch, its member slots, output
    columns and map entries)."""
    sub, _, _ = subset(c, [c["names"].index(name) for name in SCALE_ENSEMBLES], mem_gap=0)
    entries = np.concatenate([np.arange(int(d[0]), int(d[0]) + int(d[1]) * int(d[2])) for d in sub["desc"]])
    return sub, np.arange(sub["NM"]), np.arange(sub["T_out"]), entries


def bad_descriptors(c):
    """{kind: (desc row, rows NULL?)} of descriptors the device must refuse, made from ensemble 2 of batch c, (3, 70)."""
    map0, M, L, out0, mem0, f = (int(v) for v in c["desc"][2])
    return {"map0 < 0": ((-1, M, L, out0, mem0, f), False), "M < 0": ((map0, -1, L, out0, mem0, f), False),
            "L < 0": ((map0, M, -1, out0, mem0, f), False), "out_row0 < 0": ((map0, M, L, -1, mem0, f), False),
            "mem0 < 0": ((map0, M, L, out0, -1, f), False), "L > max_len": ((map0, 1, c["max_len"] + 1, 0, mem0, 0), False),
            "map0 + M L > R": ((c["R"] - M * L + 1, M, L, out0, mem0, f), False),
            "out_row0 + L > T_out": ((map0, M, L, c["T_out"] - L + 1, mem0, f), False),
            "mem0 + M > NM": ((map0, M, L, out0, c["NM"] - M + 1, f), False), "fit_to = M": ((map0, M, L, out0, mem0, M), False),
            "fit_to = -1": ((map0, M, L, out0, mem0, -1), False), "M L overflows int32": ((map0, 2 ** 31 - 1, L, out0, mem0, 0), False),
            "map0 + M L > T, rows NULL": ((c["T"] - M * L + 1, M, L, out0, mem0, f), True)}
