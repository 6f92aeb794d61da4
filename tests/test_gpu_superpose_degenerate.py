"""tmpnn_superpose (csrc/tmpnn_superpose.hip) where the rotation is not unique, and at any scale. The kernel's header says that R is a
proper rotation for ANY point set; tests/test_gpu_superpose.py compares numbers only for fits whose Horn matrix has a relative gap of
at least 0.01. Here: collinear and nearly collinear points, coincident points, an inverted cube, tetrahedron and near-cubes, half and
quarter turns, a pure translation, a member 9 000 A out, planar mirror images, an inverted chain (superpose_inputs.degenerate()).

The minimum is unique even where the minimiser is not, so two things hold for any input and any of the minimisers:
  optimal          the device's own (R, t) reaches n rmsd^2 = opt = G - 2 lambda_max, computed at 120 digits from the fp32 inputs
                   (tests/golden/superpose_degenerate.npz): n res - opt <= C 2^-52 G for the residual recomputed in longdouble from
                   the device's xform, and >= -1e-3 2^-52 G for the exact rotation nearest its R (a check of the file: a float64 R is
                   orthonormal to 1e-16 only, and a matrix that shrinks the member by that much beats every rotation by up to
                   0.94 2^-52 G on the host; no rotation does). The file holds opt as a float64 pair: one float64 is 2^-53 opt off.
  self-consistent  the device's rmsd, dev and rmsf are what its own xform gives: 2^-23 |want| + 1e-9 A, the lines of
                   test_gpu_superpose.py; NaNs in the same places; n_fit and col_count exact. Members without a unique rotation
                   included: their dev and rmsf were compared with nothing before.
C = 16: the three host methods (Kabsch by SVD, Horn by eigh, the line-by-line port of sup_solve) reach ratios (n res - opt) / (2^-52 G)
of 0.64 / 0.63 / 0.50 on degenerate(), 1.22 / 0.66 / 0.64 on crafted(), 0.00 / 0.31 / 0.13 on special() and 0 on long_pair()
(tests/test_superpose_host.py); C is 8 x the worst, up to a power of two, and is not taken from the device."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from superpose_inputs import SCALE_K, crafted, degenerate, long_pair, scale_subset, scaled, special, subset
from superpose_restatement import (ARRAYS, OPTIMAL_C, assert_all_optimal, assert_scale_covariant, assert_self_consistent,
                                   assert_superpose_close, golden_optimum, superpose_reference)
from test_gpu_superpose import _raw, _same_bits, _words

pytestmark = pytest.mark.gpu
NAMES = [name for name, _ in ARRAYS]
BATCHES = {"degenerate": degenerate, "crafted": crafted, "special": special, "long_pair": long_pair}


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(the batch, its golden optimum per member slot); left unchanged."""
    c = BATCHES[name]()
    return c, golden_optimum(load_golden("superpose_degenerate"), name, c)


@functools.lru_cache(maxsize=None)
def _device(name):
    """One call of the entry on the batch -> its outputs on the device; left unchanged."""
    c, _ = _batch(name)
    rc, got, status = _raw(c, c["rows"])
    assert rc == 0 and status.tolist() == [0] * len(c["desc"])
    return got


def _proper(got, c):
    xf = got["xform"].cpu().numpy().reshape(-1, 12)
    assert np.isfinite(xf).all()
    Rm = xf[:, :9].reshape(-1, 3, 3)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(Rm) - 1.0).max() <= 1e-12
    return xf


def test_every_degenerate_fit_is_optimal_and_self_consistent():
    c, golden = _batch("degenerate")
    got = _device("degenerate")
    xf = _proper(got, c)
    rmsd = got["rmsd"].cpu().numpy()
    print("degenerate, worst (n res - opt) / (2^-52 G):", assert_all_optimal(xf, c, golden, rmsd=rmsd))
    print("degenerate, worst ratio to the line against the device's own xform:", assert_self_consistent(got, c))
    # the conditioned families against the restatement, as test_gpu_superpose.py does; rmsf where no member of the ensemble is loose
    want = superpose_reference(c["X"], c["mask"], c["rows"], c["desc"], c["R"], c["T"], c["NM"], c["T_out"], c["max_len"])
    tight = [e for e in range(len(c["desc"])) if e not in c["loose_ensembles"]]
    cols = np.concatenate([np.arange(c["desc"][e][3], c["desc"][e][3] + c["desc"][e][2]) for e in tight])
    lengths = np.repeat(c["lengths"], c["members"])
    starts = np.concatenate([[0], np.cumsum(lengths)])
    members = np.array([g for g in range(c["NM"]) if g not in c["loose"]])
    entries = np.concatenate([np.arange(starts[g], starts[g + 1]) for g in members])
    print("conditioned families, worst ratio to the line:",
          assert_superpose_close({k: got[k] for k in NAMES}, want, c["coord"], members=members, cols=cols, entries=entries))
    # a coincident member: S = 0, R is the identity bit for bit, t = c_f - c_m (64 roundings of 2^-53 of the largest coordinate)
    for g in range(c["NM"]):
        if c["family"][g] in ("coincident", "both_coincident"):
            assert xf[g, :9].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and not np.signbit(xf[g, :9]).any(), g
            e = next(e for e, d in enumerate(c["desc"]) if d[4] <= g < d[4] + d[1])
            ca = c["X"][:, 1].astype(np.longdouble)
            cm = ca[starts[g]:starts[g + 1]].sum(axis=0) / lengths[g]
            cf = ca[c["desc"][e][0]:c["desc"][e][0] + lengths[g]].sum(axis=0) / lengths[g]
            assert np.abs(xf[g, 9:] - (cf - cm)).max() <= 64 * 2.0 ** -53 * c["coord"], g
    family = {(c["family"][g], int(lengths[g])): g for g in range(c["NM"])}
    for L in (3, 4, 19, 257, 1025):                                                   # the mirror image of a planar set is a rotation of it
        assert rmsd[family["planar_mirror", L]] <= 1e-3 and rmsd[family["planar_mirror_noisy", L]] <= 0.3 * 3 ** 0.5 * 1.2
    assert rmsd[family["inverted_cube", 8]] == 4.0 and rmsd[family["inverted_tetrahedron", 4]] == 4.0   # a half turn leaves one axis 2 x 2 A off: exact


@pytest.mark.parametrize("name", ["crafted", "special", "long_pair"])
def test_the_existing_batches_are_optimal_and_self_consistent(name):
    c, golden = _batch(name)
    got = _device(name)
    xf = got["xform"].cpu().numpy().reshape(-1, 12)
    print(name, "worst (n res - opt) / (2^-52 G):", assert_all_optimal(xf, c, golden, rmsd=got["rmsd"].cpu().numpy()))
    print(name, "worst ratio to the line against the device's own xform:", assert_self_consistent(got, c))


def test_nothing_but_the_ensemble_decides_a_bit():
    """A rerun and every degenerate ensemble alone give the bits of the one call: ties are where an order dependence would hide."""
    c, _ = _batch("degenerate")
    full = _device("degenerate")
    rc, again, _ = _raw(c, c["rows"])
    assert rc == 0 and _same_bits(again, full)
    for e in range(len(c["desc"])):
        sub, slots, cols = subset(c, [e], mem_gap=1)
        rc, got, status = _raw(sub, c["rows"])
        assert rc == 0 and status.tolist() == [0]
        live, old = torch.from_numpy(slots >= 0).cuda(), torch.from_numpy(slots[slots >= 0]).cuda()
        for name in ("n_fit", "rmsd", "xform"):
            assert torch.equal(_words(got[name])[live], _words(full[name])[old]), (c["names"][e], name)
        at = torch.from_numpy(cols).cuda()
        assert torch.equal(_words(got["rmsf"]), _words(full["rmsf"])[at]) and torch.equal(got["col_count"], full["col_count"][at]), c["names"][e]
        map0, M, L = c["desc"][e][:3].tolist()
        assert torch.equal(_words(got["dev"])[map0:map0 + M * L], _words(full["dev"])[map0:map0 + M * L]), c["names"][e]


def test_power_of_two_scaling():
    """Coordinates times 2^k, k = -60, -20, 20, 60, on a generic ensemble, a collinear one and the inverted near-cubes: R keeps its bits,
    t, rmsd, dev and rmsf are ldexp(unscaled, k) bit for bit, every entry compared. Every operation of the kernel is covariant under the
    scaling and its only threshold (the Jacobi stop rule) is relative; tests/test_superpose_host.py holds the precondition (exact in
    fp32, no subnormal output) and shows that an absolute threshold fails this."""
    c, _ = _batch("degenerate")
    sub, slots, cols, entries = scale_subset(c)
    rc, base, status = _raw(sub, sub["rows"])
    assert rc == 0 and status.tolist() == [0] * len(sub["desc"])
    for k in SCALE_K:
        s = scaled(sub, k)
        rc, got, status = _raw(s, s["rows"])
        assert rc == 0 and status.tolist() == [0] * len(sub["desc"]), k
        seen = assert_scale_covariant(base, got, k, slots, cols, entries)
        assert seen == 13 * len(slots) + len(entries) + len(cols)


def test_the_wrapper_returns_the_raw_bits(synthetic_weights):
    from thermompnn_amd.engine import Engine
    c, _ = _batch("degenerate")
    engine = Engine(synthetic_weights, "cuda:0", 48)
    res = engine.superpose(torch.from_numpy(c["X"]).cuda(), c["mask"], c["members"], c["lengths"], rows=c["rows"], fit_to=c["fit_to"])
    assert _same_bits(res, _device("degenerate")) and res["status"].tolist() == [0] * len(c["desc"])
