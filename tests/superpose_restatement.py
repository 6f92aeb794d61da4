"""tmpnn_superpose restated in numpy float64 (include/tmpnn.h has the contract): centred Kabsch by SVD with the determinant
correction, and the entry's rules for validity, n_fit < 3, the fit target and NaN. A second, independent solver (Horn's quaternion
matrix through numpy.linalg.eigh) and the relative gap of that matrix, for tests/test_superpose_host.py. A third solver, jacobi_port:
the kernel's own sup_solve line by line. And the two criteria that hold where the rotation is not unique
(tests/test_gpu_superpose_degenerate.py): assert_optimal, the residual a transform reaches against the 120-digit optimum of
tests/golden/superpose_degenerate.npz, and assert_self_consistent, rmsd, dev and rmsf against the transform they came with. No GPU,
no torch."""
import numpy as np

NAN_BITS = 0x7fc00000
ARRAYS = (("n_fit", np.int32), ("rmsd", np.float32), ("xform", np.float64), ("dev", np.float32), ("rmsf", np.float32),
          ("col_count", np.int32))
FLOOR = 1e-9              # Angstrom: results that are differences of nearly equal numbers (identical members)
ULP = 2.0 ** -23          # the kernel computes in float64 and rounds once; a float64 error can flip that rounding


def _nan32():
    return np.array([NAN_BITS], np.uint32).view(np.float32)[0]


def filled(c, bits=0x7fc54321):
    """Sentinel-filled output buffers of batch ``c``: what a call must leave where it writes nothing."""
    shape = dict(n_fit=c["NM"], rmsd=c["NM"], xform=(c["NM"], 12), dev=c["R"], rmsf=c["T_out"], col_count=c["T_out"])
    out = {}
    for name, dt in ARRAYS:
        a = np.zeros(shape[name], dt)
        a.view(np.uint32 if a.itemsize == 4 else np.uint64)[...] = bits
        out[name] = a
    return out


def check_desc(d, R, T, NM, T_out, max_len, rows_null):
    map0, M, L, out0, mem0, fit = (int(v) for v in d)
    return (map0 >= 0 and M >= 0 and L >= 0 and out0 >= 0 and mem0 >= 0 and L <= max_len and map0 + M * L <= R and
            (not rows_null or map0 + M * L <= T) and out0 + L <= T_out and mem0 + M <= NM and (M == 0 or 0 <= fit < M))


def member_points(X, mask, rows, T, at, L):
    """Map entries at .. at + L -> (P [L, 3] float64, valid [L] bool)."""
    r = np.arange(at, at + L, dtype=np.int64) if rows is None else np.asarray(rows[at:at + L]).astype(np.int64)
    inside = (r >= 0) & (r < T)                                                       # (uint32)r < T
    rr = np.where(inside, r, 0)
    P = X[rr, 1, :].astype(np.float64) if T > 0 else np.zeros((L, 3))
    valid = inside.copy()
    if T > 0:
        with np.errstate(invalid="ignore"):
            valid &= mask[rr] > 0
        valid &= np.isfinite(X[rr, 1, :]).all(axis=1)
    P[~valid] = 0.0                                                                   # (never used; keeps NaN out of the products)
    return P, valid


def covariance(Pm, Pf):
    """-> (c_m, c_f, S [3, 3]) with S[a][b] = sum (p_m - c_m)_a (p_f - c_f)_b."""
    cm, cf = Pm.mean(axis=0), Pf.mean(axis=0)
    return cm, cf, (Pm - cm).T @ (Pf - cf)


def kabsch(S, correct=True):
    """The rotation that maximises trace(R S): R = V diag(1, 1, d) U^T of S = U W V^T, d = the sign of det(V U^T) (``correct=False``:
    d = 1, which admits a reflection)."""
    U, _, Vt = np.linalg.svd(S)
    V = Vt.T
    d = np.sign(np.linalg.det(V @ U.T)) if correct else 1.0
    return V @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T


def horn_matrix(S):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def horn(S):
    """The second method: the rotation of the unit quaternion that is the eigenvector of the largest eigenvalue of Horn's matrix."""
    _, vec = np.linalg.eigh(horn_matrix(S))
    w, x, y, z = vec[:, 3] / np.linalg.norm(vec[:, 3])
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def horn_gap(S):
    """(lambda_1 - lambda_2) / lambda_1 of Horn's matrix: what the rotation's conditioning hangs on (0: no unique rotation)."""
    lam = np.linalg.eigvalsh(horn_matrix(S))
    return float((lam[3] - lam[2]) / lam[3]) if lam[3] > 0 else 0.0


def jacobi_port(S, absolute_stop=False, first_column=False, max_sweeps=32):
    """The third method: sup_solve of csrc/tmpnn_superpose.hip line by line in Python floats (IEEE double, no contraction): Horn's
    matrix, cyclic Jacobi with the rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per sweep, the stop rule off <= 1e-40 dia, at most 32
    sweeps, the column of the largest diagonal entry (ties: the first), normalised -> R [3, 3]. The switches make deliberately WRONG
    variants for tests/test_superpose_host.py, which shows that the criteria reject them: ``absolute_stop``: off <= 1e-40 without dia;
    ``first_column``: column 0 whatever the diagonal holds; ``max_sweeps``: a lower sweep cap."""
    sqrt = np.sqrt                                                                     # (correctly rounded, as the device's)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = [[float(v) for v in row] for row in np.asarray(S, np.float64)]
    A = [[0.0] * 4 for _ in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    A[0][0] = Sxx + Syy + Szz
    A[1][1] = Sxx - Syy - Szz
    A[2][2] = Syy - Sxx - Szz
    A[3][3] = Szz - Sxx - Syy
    A[0][1] = A[1][0] = Syz - Szy
    A[0][2] = A[2][0] = Szx - Sxz
    A[0][3] = A[3][0] = Sxy - Syx
    A[1][2] = A[2][1] = Sxy + Syx
    A[1][3] = A[3][1] = Szx + Sxz
    A[2][3] = A[3][2] = Syz + Szy

    def rotate(P, Q):
        apq = A[P][Q]
        if apq == 0.0:
            return
        with np.errstate(over="ignore"):
            theta = float(np.float64(A[Q][Q] - A[P][P]) / np.float64(2.0 * apq))
            tt = float(np.float64(1.0) / (np.float64(abs(theta)) + sqrt(np.float64(theta) * np.float64(theta) + 1.0)))
        t = -tt if theta < 0.0 else tt
        c = 1.0 / float(sqrt(t * t + 1.0))
        s = t * c
        A[P][P] = A[P][P] - t * apq
        A[Q][Q] = A[Q][Q] + t * apq
        A[P][Q] = A[Q][P] = 0.0
        for r in range(4):
            if r != P and r != Q:
                arp, arq = A[r][P], A[r][Q]
                A[r][P] = A[P][r] = c * arp - s * arq
                A[r][Q] = A[Q][r] = s * arp + c * arq
            vrp, vrq = V[r][P], V[r][Q]
            V[r][P] = c * vrp - s * vrq
            V[r][Q] = s * vrp + c * vrq

    for _ in range(max_sweeps):
        off = (A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3])
        dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3]
        if off <= (1e-40 if absolute_stop else 1e-40 * dia):
            break
        for P, Q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            rotate(P, Q)
    col = 0
    if not first_column:
        for k in range(1, 4):
            if A[k][k] > A[col][col]:
                col = k
    w, x, y, z = V[0][col], V[1][col], V[2][col], V[3][col]
    inv = 1.0 / float(sqrt(w * w + x * x + y * y + z * z))
    w, x, y, z = w * inv, x * inv, y * inv, z * inv
    return np.array([[w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def residual_of(xform, Pm, Pf):
    """-> (sum |R p_m + t - p_f|^2, the squared residuals [n]) of a GIVEN xform (R row-major, then t) in numpy.longdouble, so that the
    host's own rounding stays out of the lines below (x86: 64 mantissa bits; where longdouble is float64 the lines still hold for
    a float64 recomputation of fp32 inputs, only with less to spare)."""
    xf = np.asarray(xform, np.longdouble).reshape(12)
    Rm, t = xf[:9].reshape(3, 3), xf[9:]
    d = np.asarray(Pm, np.longdouble) @ Rm.T + t - np.asarray(Pf, np.longdouble)
    r2 = (d * d).sum(axis=1)
    return r2.sum(), r2


def proper_residual_of(xform, Pm, Pf):
    """sum |R' (p_m - c_m) - (p_f - c_f)|^2 for R' the EXACT rotation nearest the R of ``xform`` (Newton's iteration R <- (R + R^-T) / 2
    in numpy.longdouble: from a defect of 1e-16 two steps are below longdouble's rounding) with the best translation for it. A float64
    R is orthonormal to about 1e-16 only, and a matrix that shrinks the member by that much reaches a residual BELOW the optimum over
    rotations whenever the fit is not perfect: the lower line of assert_optimal is true of rotations, and is taken on this."""
    Rm = np.asarray(xform, np.longdouble).reshape(12)[:9].reshape(3, 3)
    for _ in range(3):
        cof = np.stack([np.cross(Rm[1], Rm[2]), np.cross(Rm[2], Rm[0]), np.cross(Rm[0], Rm[1])])
        Rm = (Rm + cof / (Rm[0] * cof[0]).sum()) / 2
    Pm, Pf = np.asarray(Pm, np.longdouble), np.asarray(Pf, np.longdouble)
    d = (Pm - Pm.sum(axis=0) / len(Pm)) @ Rm.T - (Pf - Pf.sum(axis=0) / len(Pf))
    return (d * d).sum(axis=1).sum()


def assert_optimal(n_res, opt, G, C, what="", n_proper=None):
    """The minimum is unique even where the minimiser is not: for any two point sets the least sum of squared residuals over proper
    rotations and translations is opt = G - 2 lambda_max (G: the two centred sums of squares, lambda_max: of Horn's matrix).
    ``n_res`` = n rmsd^2, the sum of squared residuals a transform reaches: n_res - opt <= C 2^-52 G. The lower line,
    -1e-3 2^-52 G <= n_proper - opt, checks ``opt`` itself (tests/golden/superpose_degenerate.npz): no ROTATION beats the optimum.
    ``n_proper``: proper_residual_of the same transform (default: n_res, for a transform that is a rotation to longdouble's rounding).
    ``opt`` as numpy.longdouble: the file's opt + opt_lo. -> (n_res - opt) / (2^-52 G)."""
    unit = 2.0 ** -52 * float(G)
    excess = float(np.longdouble(n_res) - np.longdouble(opt))
    below = float(np.longdouble(n_res if n_proper is None else n_proper) - np.longdouble(opt))
    ratio = excess / unit if unit > 0 else 0.0
    assert excess <= C * unit and -1e-3 * unit <= below, (what, ratio, below / unit if unit > 0 else below, float(n_res), float(opt), float(G))
    return ratio


OPTIMAL_C = 16.0          # 8 x the worst host ratio (1.22, Kabsch by SVD on crafted()), up to a power of two: test_superpose_host.py


def golden_optimum(z, name, c):
    """{member slot: (n, G, opt as longdouble)} of batch ``c`` from tests/golden/superpose_degenerate.npz (loaded as ``z``), after
    checking that the file was made from these very coordinates."""
    import hashlib
    sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(c["X"][:, 1]).tobytes()).digest(), np.uint8)
    assert (sha == z[name + "_sha256"]).all(), f"{name}: the fixture's coordinates are not the ones the golden file was made from"
    opt = z[name + "_opt"].astype(np.longdouble) + z[name + "_opt_lo"].astype(np.longdouble)
    return {int(g): (int(n), float(G), o) for g, n, G, o in zip(z[name + "_slot"], z[name + "_n"], z[name + "_G"], opt)}


def assert_all_optimal(xform, c, golden, C=OPTIMAL_C, rmsd=None):
    """assert_optimal for every fit of batch ``c`` on the residual recomputed from ``xform`` [NM, 12] (and, where ``rmsd`` [NM] fp32 is
    given: |rmsd^2 - opt / n| <= 2^-22 opt / n + C 2^-52 G / n). -> the worst (n res - opt) / (2^-52 G)."""
    fits = fit_sets(c)
    assert sorted(golden) == [g for g, _, _ in fits]
    worst = 0.0
    for g, Pm, Pf in fits:
        n, G, opt = golden[g]
        assert n == len(Pm)
        total, _ = residual_of(xform[g], Pm, Pf)
        worst = max(worst, assert_optimal(total, opt, G, C, what=g, n_proper=proper_residual_of(xform[g], Pm, Pf)))
        if rmsd is not None:
            mean = float(opt) / n
            assert abs(float(rmsd[g]) ** 2 - mean) <= 2.0 ** -22 * mean + C * 2.0 ** -52 * G / n, (g, float(rmsd[g]), mean)
    return worst


def assert_scale_covariant(base, got, k, slots, cols, entries):
    """``got``: the outputs for coordinates 2^k times those of ``base``. n_fit and col_count equal, R the same bits, t, rmsd, dev and
    rmsf equal to ldexp(base, k) bit for bit (NaNs included), at the member slots, output columns and map entries given. -> how many
    float words were compared."""
    b = {n: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for n, v in base.items()}
    g = {n: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for n, v in got.items()}
    np.testing.assert_array_equal(g["n_fit"][slots], b["n_fit"][slots])
    np.testing.assert_array_equal(g["col_count"][cols], b["col_count"][cols])
    bx, gx = b["xform"].reshape(-1, 12)[slots], g["xform"].reshape(-1, 12)[slots]
    assert (_bits(gx[:, :9]) == _bits(bx[:, :9])).all(), ("R", k)
    assert (_bits(gx[:, 9:]) == _bits(np.ldexp(bx[:, 9:], k))).all(), ("t", k)
    seen = gx.size
    for name, idx in (("rmsd", slots), ("dev", entries), ("rmsf", cols)):
        want = np.ldexp(b[name][idx], k).astype(np.float32)
        assert (_bits(g[name][idx]) == _bits(want)).all(), (name, k, int((_bits(g[name][idx]) != _bits(want)).sum()))
        seen += want.size
    return seen


def from_xform(c, rows, xform):
    """What rmsd, dev, rmsf, n_fit and col_count have to be GIVEN the transforms ``xform`` [NM, 12] (the device's own), by the entry's
    rules and in numpy.longdouble; every descriptor of batch ``c`` is good. The column loop of superpose_reference, over all columns of
    an ensemble at once."""
    res = {k: v.copy() for k, v in filled(c, 0).items() if k != "xform"}
    nan = _nan32()
    xform = np.asarray(xform, np.float64).reshape(-1, 12)
    for d in np.asarray(c["desc"], np.int64).reshape(-1, 6):
        map0, M, L, out0, mem0, fit = (int(v) for v in d)
        pts = [member_points(c["X"], c["mask"], rows, c["T"], map0 + m * L, L) for m in range(M)]
        moved, takes = np.zeros((M, L, 3), np.longdouble), np.zeros((M, L), bool)
        for m, (P, valid) in enumerate(pts):
            g = mem0 + m
            dev = np.full(L, nan, np.float32)
            F = valid & pts[fit][1]
            n = int(F.sum())
            res["n_fit"][g] = n
            if m == fit or n == 0:
                res["rmsd"][g] = nan if n == 0 else np.float32(0.0)
                if m == fit:
                    dev[valid] = 0.0
            else:
                total, r2 = residual_of(xform[g], P[F], pts[fit][0][F])
                res["rmsd"][g] = np.float32(np.sqrt(total / n))
                if n >= 3:
                    dev[F] = np.sqrt(r2).astype(np.float32)
            res["dev"][map0 + m * L:map0 + (m + 1) * L] = dev
            xf = xform[g].astype(np.longdouble)
            moved[m], takes[m] = P.astype(np.longdouble) @ xf[:9].reshape(3, 3).T + xf[9:], valid & (n >= 3 or m == fit)
        if M == 0:
            res["col_count"][out0:out0 + L], res["rmsf"][out0:out0 + L] = 0, nan
            continue
        count = takes.sum(axis=0)
        some = np.maximum(count, 1).astype(np.longdouble)
        mu = (moved * takes[:, :, None]).sum(axis=0) / some[:, None]
        spread = ((((moved - mu) ** 2).sum(axis=2)) * takes).sum(axis=0) / some
        res["col_count"][out0:out0 + L] = count
        res["rmsf"][out0:out0 + L] = np.where(count > 0, np.sqrt(spread).astype(np.float32), nan)
    return res


def assert_self_consistent(got, c, rows="own"):
    """The device's rmsd, dev and rmsf are what its OWN xform gives on the inputs (from_xform): within 2^-23 |want| + FLOOR, NaNs in
    the same places with the canonical bits, n_fit and col_count exact. Every member, the ones without a unique rotation included:
    whichever minimiser the device took, its other outputs have to be that minimiser's. -> the worst ratio to the line per output."""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}
    want = from_xform(c, c["rows"] if isinstance(rows, str) else rows, g["xform"])
    np.testing.assert_array_equal(g["n_fit"], want["n_fit"])
    np.testing.assert_array_equal(g["col_count"], want["col_count"])
    worst = {}
    for name in ("rmsd", "dev", "rmsf"):
        a, b = g[name], want[name]
        nan = np.isnan(b)
        assert (np.isnan(a) == nan).all(), name
        assert (_bits(a)[nan] == NAN_BITS).all(), name
        line = ULP * np.abs(b[~nan].astype(np.float64)) + FLOOR
        ratio = np.abs(a[~nan].astype(np.float64) - b[~nan].astype(np.float64)) / line
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        assert worst[name] <= 1.0, (name, worst[name], int(np.flatnonzero(~nan)[ratio.argmax()]))
    return worst


def fit_sets(c, rows="own"):
    """Every fit of batch ``c`` with at least one column: [(member slot g, Pm [n, 3], Pf [n, 3])] float64 (fp32 values), the fit
    target's own slot left out."""
    rows = c["rows"] if isinstance(rows, str) else rows
    out = []
    for d in np.asarray(c["desc"], np.int64).reshape(-1, 6):
        map0, M, L, _, mem0, fit = (int(v) for v in d)
        pts = [member_points(c["X"], c["mask"], rows, c["T"], map0 + m * L, L) for m in range(M)]
        for m, (P, valid) in enumerate(pts):
            F = valid & pts[fit][1]
            if m != fit and F.any():
                out.append((mem0 + m, P[F], pts[fit][0][F]))
    return out


def fit_points(Pm, Pf, solver=kabsch):
    """Pm onto Pf, [n, 3] float64 each, n >= 1 -> (R, t, the residuals |R p_m + t - p_f| [n], S)."""
    cm, cf, S = covariance(Pm, Pf)
    Rm = solver(S)
    t = cf - Rm @ cm
    return Rm, t, np.sqrt((((Pm @ Rm.T + t) - Pf) ** 2).sum(axis=1)), S


def superpose_reference(X, mask, rows, desc, R, T, NM, T_out, max_len, out=None, solver=kabsch):
    """-> dict(n_fit, rmsd, xform, dev, rmsf, col_count, status, gap). ``out``: buffers to write into (copied; default NaN / zero
    filled ones, which a good call covers wherever the comparison looks). ``gap`` [NM] float64: horn_gap of every fit with n_fit >= 3
    of a member that is not the fit target, NaN elsewhere."""
    X = np.asarray(X, np.float32).reshape(-1, 4, 3)
    desc = np.asarray(desc, np.int64).reshape(-1, 6)
    c = dict(NM=NM, R=R, T_out=T_out)
    res = {k: v.copy() for k, v in (filled(c, 0) if out is None else out).items()}
    res["status"] = np.zeros(len(desc), np.int32)
    res["gap"] = np.full(NM, np.nan)
    nan = _nan32()
    for e, d in enumerate(desc):
        if not check_desc(d, R, T, NM, T_out, max_len, rows is None):
            res["status"][e] = -1
            continue
        map0, M, L, out0, mem0, fit = (int(v) for v in d)
        pts = [member_points(X, mask, rows, T, map0 + m * L, L) for m in range(M)]
        moved = []
        for m, (P, valid) in enumerate(pts):
            g = mem0 + m
            dev = np.full(L, nan, np.float32)
            F = valid & pts[fit][1]
            n = int(F.sum())
            Rm, t = np.eye(3), np.zeros(3)
            res["n_fit"][g] = n
            if m == fit or n == 0:
                res["rmsd"][g] = nan if n == 0 else np.float32(0.0)
                if m == fit:
                    dev[valid] = 0.0
            else:
                Rm, t, resid, S = fit_points(P[F], pts[fit][0][F], solver)
                res["rmsd"][g] = np.float32(np.sqrt((resid ** 2).sum() / n))
                if n >= 3:
                    dev[F] = resid.astype(np.float32)
                    res["gap"][g] = horn_gap(S)
            res["xform"][g, :9], res["xform"][g, 9:] = Rm.reshape(-1), t
            res["dev"][map0 + m * L:map0 + (m + 1) * L] = dev
            moved.append((P @ Rm.T + t, valid & (n >= 3 or m == fit)))
        for q in range(L):
            pts_q = [Pm[q] for Pm, takes in moved if takes[q]]                        # ascending m
            res["col_count"][out0 + q] = len(pts_q)
            if pts_q:
                mu = np.sum(pts_q, axis=0) / len(pts_q)
                res["rmsf"][out0 + q] = np.float32(np.sqrt(((np.array(pts_q) - mu) ** 2).sum() / len(pts_q)))
            else:
                res["rmsf"][out0 + q] = nan
    return res


def assert_conditioned(want, loose=(), floor=0.01):
    """Every fit with n_fit >= 3 whose rotation the comparisons use has a relative gap of Horn's matrix of at least ``floor``.
    -> (the smallest, the largest) gap met."""
    gap = want["gap"].copy()
    gap[np.asarray(loose, np.int64)] = np.nan
    seen = gap[~np.isnan(gap)]
    assert seen.size and seen.min() >= floor, (float(seen.min()) if seen.size else None, int(np.nanargmin(gap)) if seen.size else None)
    return float(seen.min()), float(seen.max())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def assert_superpose_close(got, want, coord, members=None, loose=(), cols=None, entries=None):
    """The lines of the issue. Exact: n_fit, col_count (and status, by the caller), NaNs in the same places with the canonical bits.
    The fp32 outputs within 2^-23 |want| + 1e-9 A; R within 1e-11, t within 1e-11 max(1, ``coord``); R R^T = I within 1e-12 and
    det R = +1. ``members`` / ``cols`` / ``entries``: index arrays into [NM] / [T_out] / [R] to compare (default: all). ``loose``:
    member slots without a unique rotation: only n_fit, rmsd, orthonormality and det are compared there, the caller leaves their
    ensemble's entries and columns out. -> the worst ratio to its line per output."""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}
    members = np.arange(len(want["n_fit"])) if members is None else np.asarray(members, np.int64)
    cols = np.arange(len(want["rmsf"])) if cols is None else np.asarray(cols, np.int64)
    entries = np.arange(len(want["dev"])) if entries is None else np.asarray(entries, np.int64)
    worst = {}

    def close(name, idx):
        a, b = g[name][idx], want[name][idx]
        nan = np.isnan(b)
        assert (np.isnan(a) == nan).all(), name
        assert (_bits(a)[nan] == NAN_BITS).all(), name
        line = ULP * np.abs(b[~nan].astype(np.float64)) + FLOOR
        ratio = np.abs(a[~nan].astype(np.float64) - b[~nan].astype(np.float64)) / line
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        assert worst[name] <= 1.0, (name, worst[name])

    np.testing.assert_array_equal(g["n_fit"][members], want["n_fit"][members])
    np.testing.assert_array_equal(g["col_count"][cols], want["col_count"][cols])
    close("rmsd", members)
    close("dev", entries)
    close("rmsf", cols)
    xf = g["xform"][members].reshape(-1, 12)
    Rm = xf[:, :9].reshape(-1, 3, 3)
    worst["orthonormal"] = float(np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() / 1e-12) if len(Rm) else 0.0
    assert worst["orthonormal"] <= 1.0, worst
    assert (np.abs(np.linalg.det(Rm) - 1.0) <= 1e-12).all()
    tight = ~np.isin(members, np.asarray(loose, np.int64)) & ~np.isin(want["n_fit"][members], (1, 2))   # n_fit 1 or 2: any minimiser
    wx = want["xform"][members].reshape(-1, 12)
    worst["R"] = float(np.abs(xf[tight, :9] - wx[tight, :9]).max() / 1e-11) if tight.any() else 0.0
    worst["t"] = float(np.abs(xf[tight, 9:] - wx[tight, 9:]).max() / (1e-11 * max(1.0, coord))) if tight.any() else 0.0
    assert worst["R"] <= 1.0 and worst["t"] <= 1.0, worst
    return worst
