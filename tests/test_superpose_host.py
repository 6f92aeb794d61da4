"""The numpy restatement of tmpnn_superpose (tests/superpose_restatement.py) held against a second method, its fixtures
(tests/superpose_inputs.py) against the conditioning the GPU comparisons rely on, and the entry's host-side argument errors. The
criteria of tests/test_gpu_superpose_degenerate.py on the host: three float64 methods reach the 120-digit optimum of every fixture
fit, deliberately wrong solvers do not, and the golden file regenerates. No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from superpose_inputs import (CONDITIONED_FAMILIES, LOOSE_FAMILIES, NOISE, bad_descriptors, chain, crafted, degenerate, drawn_map, long_pair,
                              moved, SCALE_K, scale_subset, scaled, special, subset)
from superpose_restatement import (OPTIMAL_C, assert_all_optimal, assert_conditioned, assert_optimal, assert_scale_covariant,
                                   assert_self_consistent, assert_superpose_close, filled, fit_points, fit_sets, golden_optimum, horn,
                                   horn_gap, jacobi_port, kabsch, proper_residual_of, residual_of, superpose_reference)


def _reference(c, rows="own", **kw):
    rows = c["rows"] if isinstance(rows, str) else rows
    return superpose_reference(c["X"], c["mask"], rows, c["desc"], c["R"], c["T"], c["NM"], c["T_out"], c["max_len"], **kw)


def test_kabsch_by_svd_agrees_with_horn_by_eigh():
    """Two float64 methods that share only the covariance: they agreed to 4.4e-15 A on rmsd and 3.4e-13 A on deviations when the
    fixtures were written; the line is 1e-11."""
    rng = np.random.default_rng(2)
    worst_rmsd = worst_dev = 0.0
    for L in (3, 4, 7, 19, 64, 257, 1025, 2048):
        for noise in NOISE:
            Pf = chain(L, rng).astype(np.float32).astype(np.float64)
            Pm = moved(Pf, rng, noise).astype(np.float32).astype(np.float64)
            Ra, ta, da, S = fit_points(Pm, Pf, kabsch)
            Rb, tb, db, _ = fit_points(Pm, Pf, horn)
            assert horn_gap(S) >= 0.01, (L, noise)
            assert abs(np.linalg.det(Ra) - 1) < 1e-12 and abs(np.linalg.det(Rb) - 1) < 1e-12
            worst_rmsd = max(worst_rmsd, abs(np.sqrt((da ** 2).mean()) - np.sqrt((db ** 2).mean())))
            worst_dev = max(worst_dev, float(np.abs(da - db).max()))
            assert np.abs(Ra - Rb).max() <= 1e-11, (L, noise)
    print(f"kabsch against horn: rmsd {worst_rmsd:.2e} A, deviations {worst_dev:.2e} A")
    assert worst_rmsd <= 1e-11 and worst_dev <= 1e-11


def test_whole_restatement_with_either_solver():
    """The restatement as the GPU tests use it, on the crafted batch through a drawn map, with the second solver in place of the
    first: the lines the device is held to."""
    c = crafted()
    rows = drawn_map(c, np.random.default_rng(31))
    a, b = _reference(c, rows), _reference(c, rows, solver=horn)
    assert a["status"].tolist() == [0] * 7
    worst = assert_superpose_close(b, a, c["coord"])
    print("horn against kabsch, worst ratio to the line:", worst)
    fit = np.array(c["fit_to"]) + c["desc"][:, 4]
    for e, g in enumerate(fit):
        if c["members"][e]:
            assert a["xform"][g].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and a["rmsd"][g] == 0 or a["n_fit"][g] == 0


def test_every_fixture_fit_is_well_conditioned():
    """(lambda_1 - lambda_2) / lambda_1 >= 0.01 of Horn's matrix for every fit with n_fit >= 3 whose rotation a comparison uses: the
    1e-11 line on R presumes it. The collinear ensemble is the one exception, and there no rotation is compared."""
    c = crafted()
    lo, hi = [], []
    for want, loose in ((_reference(c), ()), (_reference(c, drawn_map(c, np.random.default_rng(31))), ()),
                        (_reference(c, None), ()), (_reference(long_pair()), ())):
        a, b = assert_conditioned(want, loose)
        lo.append(a), hi.append(b)
    s = special()
    want = _reference(s)
    a, b = assert_conditioned(want, s["loose"])
    print(f"relative gaps: {min(lo + [a]):.3f} .. {max(hi + [b]):.3f}")
    assert want["gap"][s["loose"][0]] < 1e-6                                           # collinear: no unique rotation
    assert want["n_fit"][:7].tolist() == [10, 0, 1, 2, 3, 0, 10]
    assert np.isnan(want["rmsd"][1]) and want["rmsd"][2] <= 1e-9 and want["rmsd"][3] > 1e-6 and np.isnan(want["rmsd"][5])
    assert np.isnan(want["dev"][2 * 12:4 * 12]).all() and (~np.isnan(want["dev"][4 * 12:5 * 12])).sum() == 3
    assert want["col_count"][:12].tolist() == [2, 2, 3, 3, 3] + [2] * 7                # members 4 and 6; at 2, 3, 4 the target too; then
    d1 = int(s["desc"][1][4])
    assert want["rmsd"][d1] <= 1e-9 and want["rmsd"][d1 + 1] <= 1e-9                     # exact copies: through the map, and in rows of its own
    assert want["rmsd"][d1 + 2] > 1.0                                                  # the mirror image does not fit


def test_a_mirror_image_is_not_fitted_by_a_reflection():
    rng = np.random.default_rng(9)
    Pf = chain(60, rng)
    Pm = moved(Pf * np.array([-1.0, 1.0, 1.0]), rng, 0.0)
    Rp, _, proper, _ = fit_points(Pm, Pf, kabsch)
    Rr, _, reflected, _ = fit_points(Pm, Pf, lambda S: kabsch(S, correct=False))
    assert np.linalg.det(Rp) > 0.999 and np.linalg.det(Rr) < -0.999
    rmsd = lambda d: float(np.sqrt((d ** 2).mean()))
    assert rmsd(reflected) < 1e-9 and rmsd(proper) > 1.0
    _, _, by_horn, _ = fit_points(Pm, Pf, horn)
    assert abs(rmsd(by_horn) - rmsd(proper)) <= 1e-11


def test_bad_descriptors_and_subsets_in_the_restatement():
    c = crafted()
    good = _reference(c)
    for kind, (row, null) in bad_descriptors(c).items():
        desc = c["desc"].copy()
        desc[2] = row
        out = filled(c)
        b = dict(c, desc=desc, R=c["R"] + (8 if null else 0))
        if null:
            out["dev"] = np.concatenate([out["dev"], out["dev"][:8]])
        got = _reference(b, None if null else "own", out=out)
        assert got["status"].tolist() == [0, 0, -1, 0, 0, 0, 0], kind
        assert (got["rmsf"][22:92].view(np.uint32) == 0x7fc54321).all() and (got["rmsf"][:22].view(np.uint32) == good["rmsf"][:22].view(np.uint32)).all(), kind
    sub, slots, cols = subset(c, [4, 2, 0])
    part = _reference(sub)
    live = slots >= 0
    assert (part["n_fit"][live] == good["n_fit"][slots[live]]).all() and (part["xform"][live] == good["xform"][slots[live]]).all()
    assert (part["col_count"] == good["col_count"][cols]).all()


def test_argument_errors_do_not_need_a_gpu():
    """tmpnn_superpose refuses before any launch, with an error code and a message, as the neighbouring entries do."""
    from thermompnn_amd import _lib
    lib = _lib.load()
    p = 256                                                                            # a non-null pointer that no refused call reads

    def call(X=p, mask=p, rows=p, R=10, desc=p, E=1, T=10, NM=2, T_out=5, max_len=5, n_fit=p, rmsd=p, xform=p, dev=p, rmsf=p,
             col_count=p, status=p):
        return lib.tmpnn_superpose(X, mask, rows, R, desc, E, T, NM, T_out, max_len, n_fit, rmsd, xform, dev, rmsf, col_count, status, None)

    for bad in (dict(E=-1), dict(T=-1), dict(NM=-1), dict(T_out=-1), dict(max_len=-1), dict(R=-1)):
        assert call(**bad) == -1 and b"bad sizes" in lib.tmpnn_last_error(), bad
    for name in ("X", "mask", "desc", "n_fit", "rmsd", "xform", "dev", "rmsf", "col_count", "status"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.tmpnn_last_error(), name
    assert call(max_len=8193) == -2 and b"max_len" in lib.tmpnn_last_error()
    assert call(E=65536) == -2 and b"65535" in lib.tmpnn_last_error()
    for name in ("T", "NM", "T_out", "R"):
        assert call(**{name: 2 ** 31}) == -2 and b"2^31 - 1" in lib.tmpnn_last_error(), name
    assert call(E=0) == 0 and call(E=0, desc=None, status=None, rows=None) == 0        # a no-op: nothing is launched
    with pytest.raises(_lib.TmpnnError, match="superpose"):
        _lib.check(call(max_len=8193), "tmpnn_superpose")


# ---- where the rotation is not unique: the optimum is (tests/golden/superpose_degenerate.npz, make_superpose_golden.py) --------------
BATCHES = {"degenerate": degenerate, "crafted": crafted, "special": special, "long_pair": long_pair}
IN_BETWEEN = {"inverted_near_cube_10": 3.9e-3, "inverted_near_cube_16": 6.2e-5}      # 4 x 2^-k to first order: the edge ratios as given


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(the batch, its golden optimum per member slot); left unchanged."""
    c = BATCHES[name]()
    return c, golden_optimum(load_golden("superpose_degenerate"), name, c)


def _xforms(c, solver):
    """[NM, 12]: the transform of every fit of batch c by ``solver``, in float64 as fit_points computes it; zero where there is none."""
    xf = np.zeros((c["NM"], 12))
    for g, Pm, Pf in fit_sets(c):
        Rm, t, _, _ = fit_points(Pm, Pf, solver)
        xf[g, :9], xf[g, 9:] = Rm.reshape(-1), t
    return xf


def _slot(c, ensemble, family):
    d = c["desc"][c["names"].index(ensemble)]
    return int(d[4]) + c["family"][d[4]:d[4] + d[1]].index(family)


def test_degenerate_families_lie_outside_the_conditioned_range():
    """The loose families have a relative gap of Horn's matrix of at most 1e-6, the conditioned ones of at least 0.01: none of the
    former was admitted by assert_conditioned before. Two members sit in between BY THEIR DEFINITION: an inverted box of edges
    1 : 1 + 2^-k : 1 + 2^-k+1 has the gap 2 (b^2 - a^2) / (b^2 + c^2 - a^2) = 4 x 2^-k to first order, which is 3.9e-3 at k = 10 and
    6.1e-5 at k = 16 (k = 22: 9.5e-7). They are loose all the same, below the 0.01 that a comparison of R presumes."""
    c, _ = _batch("degenerate")
    want = _reference(c)
    assert want["status"].tolist() == [0] * len(c["desc"])
    assert sorted(c["loose"] + c["conditioned"]) == [g for g in range(c["NM"]) if c["family"][g] != "target"]
    lengths = np.repeat(c["lengths"], c["members"])
    assert (want["n_fit"] == lengths).all()
    for g in c["loose"]:
        name, gap = c["family"][g], want["gap"][g]
        if name in IN_BETWEEN:
            assert 0.5 * IN_BETWEEN[name] <= gap <= IN_BETWEEN[name] < 0.01, (name, gap)
        else:
            assert gap <= 1e-6, (name, int(lengths[g]), gap)
    lo, hi = assert_conditioned(want, c["loose"])
    print(f"conditioned families: relative gaps {lo:.3f} .. {hi:.3f}")
    for family in LOOSE_FAMILIES + CONDITIONED_FAMILIES:
        sizes = sorted(int(lengths[g]) for g in range(c["NM"]) if c["family"][g] == family)
        if family.startswith("inverted"):
            assert sizes == [4 if "tetra" in family else 8], family
        else:
            assert sizes == [3, 4, 19, 257] + [1025] * (("collinear" in family) or ("planar" in family)), (family, sizes)
    rmsd = {(c["family"][g], int(lengths[g])): float(want["rmsd"][g]) for g in range(c["NM"])}
    for L in (3, 4, 19, 257, 1025):                                                   # turning the plane over undoes an in-plane mirror
        assert rmsd["planar_mirror", L] <= 1e-3 and 0.1 <= rmsd["planar_mirror_noisy", L] <= 0.3 * 3 ** 0.5 * 1.2
    assert 8500.0 <= c["coord"] <= 9500.0                                              # the far member: the edge of the PDB range


def test_the_golden_optimum_regenerates():
    """A sample of the file's entries recomputed at 120 digits, the stored coordinates against degenerate() on this numpy, and the
    digests of the other three batches."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, GOLDEN)
    try:
        import make_superpose_golden as gen
    finally:
        sys.path.remove(GOLDEN)
    z = load_golden("superpose_degenerate")
    assert os.path.getsize(os.path.join(GOLDEN, "superpose_degenerate.npz")) < 400_000
    c, _ = _batch("degenerate")
    assert z["ca"].dtype == np.float32 and (z["ca"].view(np.uint32) == c["X"][:, 1].view(np.uint32)).all()
    for name, every in (("degenerate", 3), ("special", 1), ("crafted", 40)):
        b, _ = _batch(name)
        assert (gen.digest(b) == z[name + "_sha256"]).all(), name
        pick = z[name + "_slot"][::every].tolist()
        slot, n, G, opt, opt_lo = gen.entries(b, only=set(pick))
        at = np.isin(z[name + "_slot"], pick)
        for key, val in (("slot", slot), ("n", n), ("G", G), ("opt", opt), ("opt_lo", opt_lo)):
            assert np.array_equal(z[name + "_" + key][at], val), (name, key)
    b, _ = _batch("long_pair")                                                         # (8 192 points: 0.3 s at 120 digits; no need for less)
    assert np.array_equal(gen.entries(b)[3], z["long_pair_opt"])


def test_three_methods_reach_the_optimum_on_every_fit():
    """Kabsch by SVD, Horn by eigh and the line-by-line port of the kernel's solver, on degenerate(), crafted(), special() and
    long_pair(): (n res - opt) / (2^-52 G) measured 0.64 / 0.63 / 0.50, 1.22 / 0.66 / 0.64, 0.00 / 0.31 / 0.13 and 0 / 0 / 0 when this
    was written. OPTIMAL_C is 8 x the worst of them, up to a power of two: 16. The 8 pays for the device's other summation order and
    its float64 residual sweep; here the methods have to stay within C / 8 themselves."""
    worst = {}
    for name in BATCHES:
        c, golden = _batch(name)
        for label, solver in (("kabsch", kabsch), ("horn", horn), ("port", jacobi_port)):
            worst[name, label] = assert_all_optimal(_xforms(c, solver), c, golden, C=OPTIMAL_C / 8)
    print("worst (n res - opt) / (2^-52 G):", {k: round(v, 3) for k, v in worst.items()})
    assert 8 * max(worst.values()) <= OPTIMAL_C


def test_the_port_is_the_restatement_with_a_third_solver():
    """The whole restatement through jacobi_port against Kabsch on the conditioned fixtures, at the lines the device is held to; and
    its own outputs pass the self-consistency check (through the float64 xform it returns)."""
    for name in ("crafted", "long_pair"):
        c, _ = _batch(name)
        a, b = _reference(c), _reference(c, solver=jacobi_port)
        print(name, "port against kabsch, worst ratio to the line:", assert_superpose_close(b, a, c["coord"]))
    c, _ = _batch("degenerate")
    b = _reference(c, solver=jacobi_port)
    print("degenerate, the port's outputs against its own xform:", assert_self_consistent(b, c))
    off = dict(b, dev=b["dev"].copy())
    off["dev"][c["desc"][0][0] + 7] *= np.float32(1 + 2.0 ** -20)                      # a loose member's deviation (0.4 A), 8 ulps out
    with pytest.raises(AssertionError, match="dev"):
        assert_self_consistent(off, c)


def test_wrong_solvers_are_rejected():
    """The criteria can fail: each deliberately wrong variant of the port misses one on a named fixture, where the port passes."""
    c, golden = _batch("degenerate")

    def reaches(solver, g):
        _, Pm, Pf = next(f for f in fit_sets(c) if f[0] == g)
        Rm, t, _, _ = fit_points(Pm, Pf, solver)
        xf = np.concatenate([Rm.reshape(-1), t])
        return assert_optimal(residual_of(xf, Pm, Pf)[0], golden[g][2], golden[g][1], OPTIMAL_C, n_proper=proper_residual_of(xf, Pm, Pf))

    # first_column: after a half turn w = 0, the largest eigenvalue does not end in column 0
    for family in ("half_turn_x", "half_turn_y", "half_turn_z", "half_turn_generic"):
        g = _slot(c, "generic:19", family)
        reaches(jacobi_port, g)
        with pytest.raises(AssertionError):
            reaches(functools.partial(jacobi_port, first_column=True), g)
    # one sweep does not converge on a generic fit
    g = _slot(c, "generic:257", "far")
    reaches(jacobi_port, g)
    with pytest.raises(AssertionError):
        reaches(functools.partial(jacobi_port, max_sweeps=1), g)
    # an absolute stop rule: at 2^-60 of the scale every entry of Horn's matrix squared is below it, no sweep runs
    sub, slots, cols = subset(c, [c["names"].index("generic:19")], mem_gap=0)
    entries = np.arange(int(sub["desc"][0][0]), int(sub["desc"][0][0]) + int(sub["desc"][0][1]) * 19)
    for solver, passes in ((jacobi_port, True), (functools.partial(jacobi_port, absolute_stop=True), False)):
        base, small = _reference(sub, solver=solver), _reference(scaled(sub, -60), solver=solver)
        if passes:
            assert_scale_covariant(base, small, -60, np.arange(sub["NM"]), np.arange(19), entries)
        else:
            with pytest.raises(AssertionError, match="R"):
                assert_scale_covariant(base, small, -60, np.arange(sub["NM"]), np.arange(19), entries)


def test_power_of_two_scaling_is_exact_for_the_port():
    """The precondition of the device's scaling test: multiplying by 2^k is exact in fp32 and stays in its normal range, no fp32
    output of the restatement (with the kernel's solver) is subnormal at any k, and every entry is compared: the restatement's R keeps
    its bits, t, rmsd, dev and rmsf are ldexp(unscaled, k)."""
    c, _ = _batch("degenerate")
    sub, slots, cols, entries = scale_subset(c)
    base = _reference(sub, solver=jacobi_port)
    ca = sub["X"][np.unique(entries), 1]
    tiny = np.float32(2.0 ** -126)
    for k in SCALE_K:
        s = scaled(sub, k)
        back = s["X"][np.unique(entries), 1] * np.float32(2.0 ** -k)
        assert (back.view(np.uint32) == ca.view(np.uint32)).all() and np.isfinite(s["X"][np.unique(entries), 1]).all()
        assert ((np.abs(s["X"][np.unique(entries), 1]) >= tiny) | (ca == 0)).all()
        got = _reference(s, solver=jacobi_port)
        for name, idx in (("rmsd", slots), ("dev", entries), ("rmsf", cols)):
            v = got[name][idx]
            assert not np.isnan(v).any() and ((np.abs(v) >= tiny) | (base[name][idx] == 0)).all(), (name, k)
        seen = assert_scale_covariant(base, got, k, slots, cols, entries)
        assert seen == 12 * len(slots) + len(slots) + len(entries) + len(cols)           # nothing is left out
