"""tmpnn_superpose restated in numpy float64 (include/tmpnn.h has the contract): centred Kabsch by SVD with the determinant
correction, and the entry's rules for validity, n_fit < 3, the fit target and NaN. A second, independent solver (Horn's quaternion
matrix through numpy.linalg.eigh) and the relative gap of that matrix, for tests/test_superpose_host.py. No GPU, no torch."""
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
