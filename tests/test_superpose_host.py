"""The numpy restatement of tmpnn_superpose (tests/superpose_restatement.py) held against a second method, its fixtures
(tests/superpose_inputs.py) against the conditioning the GPU comparisons rely on, and the entry's host-side argument errors. No GPU."""
import numpy as np
import pytest

from superpose_inputs import NOISE, bad_descriptors, chain, crafted, drawn_map, long_pair, moved, special, subset
from superpose_restatement import (assert_conditioned, assert_superpose_close, filled, fit_points, horn, horn_gap, kabsch,
                                   superpose_reference)


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
