"""The least residual of every superposition fit of the fixtures, at 120 digits: tests/golden/superpose_degenerate.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_superpose_golden.py

For two point sets p_m, p_f of n points each the least sum of squared residuals over proper rotations R and translations t is

    opt = G - 2 lambda_max,   G = sum |p_m - c_m|^2 + sum |p_f - c_f|^2,

lambda_max the largest eigenvalue of Horn's 4 x 4 matrix of S = sum (p_m - c_m)(p_f - c_f)^T. That minimum is unique even where the
minimising rotation is not (collinear points, coincident points, an inverted cube). Everything here — centroids, G, S, the
eigenvalues (mpmath.eigsy) — is computed in mpmath at 120 digits from the fp32 coordinates, which are exact there; only the results
are rounded, to float64. Needs mpmath, numpy and the two helper modules of tests/; nothing else, no GPU.

Stored: ``ca`` [T, 3] float32, the C-alphas of superpose_inputs.degenerate(), and for it and for crafted(), special() and long_pair()
(prefixes degenerate_, crafted_, special_, long_pair_; their coordinates are not stored, a SHA-256 of the C-alpha bytes is):
``slot`` [k] int32, the member slots of the fits with at least one column (the fit targets have none), ``n`` [k], ``G`` [k] and
``opt`` [k] float64, and ``opt_lo`` [k] float64, what rounding opt to float64 took away.
"""
import hashlib
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import superpose_inputs as si                     # noqa: E402
import superpose_restatement as sr                # noqa: E402

DIGITS = 120
OUT = os.path.join(HERE, "superpose_degenerate.npz")
BATCHES = {"degenerate": si.degenerate, "crafted": si.crafted, "special": si.special, "long_pair": si.long_pair}


def optimum(Pm, Pf):
    """[n, 3] float arrays holding fp32 values -> (G, opt, opt_lo) as float64, computed at DIGITS digits. opt + opt_lo is the optimum
    to 2^-106: rounding it to one float64 alone moves it by up to 2^-53 opt, 500 x the lower line of assert_optimal."""
    with mp.workdps(DIGITS):
        n = len(Pm)
        pm = [[mp.mpf(float(v)) for v in p] for p in Pm]
        pf = [[mp.mpf(float(v)) for v in p] for p in Pf]
        cm = [mp.fsum(p[a] for p in pm) / n for a in range(3)]
        cf = [mp.fsum(p[a] for p in pf) / n for a in range(3)]
        pm = [[p[a] - cm[a] for a in range(3)] for p in pm]
        pf = [[p[a] - cf[a] for a in range(3)] for p in pf]
        G = mp.fsum(v * v for p in pm for v in p) + mp.fsum(v * v for p in pf for v in p)
        (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = [[mp.fsum(p[a] * q[b] for p, q in zip(pm, pf)) for b in range(3)] for a in range(3)]
        N = mp.matrix([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                       [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                       [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                       [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
        E = mp.eigsy(N, eigvals_only=True) if G > 0 else mp.zeros(4, 1)
        lam = max(E[i] for i in range(4))
        opt = G - 2 * lam
        return float(G), float(opt), float(opt - mp.mpf(float(opt)))


def digest(c):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(c["X"][:, 1]).tobytes()).digest(), np.uint8)


def entries(c, only=None):
    """-> (slot, n, G, opt, opt_lo) of the fits of batch ``c`` (``only``: of these member slots)."""
    fits = [f for f in sr.fit_sets(c) if only is None or f[0] in only]
    done = [optimum(Pm, Pf) for _, Pm, Pf in fits]
    return (np.array([g for g, _, _ in fits], np.int32), np.array([len(Pm) for _, Pm, _ in fits], np.float64),
            np.array([v[0] for v in done], np.float64), np.array([v[1] for v in done], np.float64), np.array([v[2] for v in done], np.float64))


def main():
    out = {}
    for name, make in BATCHES.items():
        c = make()
        out[name + "_slot"], out[name + "_n"], out[name + "_G"], out[name + "_opt"], out[name + "_opt_lo"] = entries(c)
        out[name + "_sha256"] = digest(c)
        if name == "degenerate":
            out["ca"] = c["ca"]
        print(f"{name}: {len(out[name + '_slot'])} fits")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
