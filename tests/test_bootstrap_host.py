"""Bootstrap intervals, the parts that need no GPU: the numpy restatement of tmpnn_bootstrap_metrics against metrics.get_metrics on
the gathered resamples and against exact rational arithmetic, the condition that keeps the device tests from passing while they test
nothing (ranks without tie averaging DO move spearman on these fixtures), the tie groups torch.unique gives, the argument errors of the
C entry (before any launch), and the command line with ``-gpu n``."""
import csv
import ctypes as C
import io

import numpy as np
import pytest

from bootstrap_restatement import (HOST_SIZES, LDS_N, MAX_B, MAX_M, MAX_N, METRICS, SPEARMAN_TOL, assert_metrics_close,
                                   bootstrap_brute, bootstrap_exact, bootstrap_reference, dense_rank, fixture_rows,
                                   fixture_values, value_tol)


@pytest.mark.parametrize("N", HOST_SIZES)
def test_restatement_equals_get_metrics_on_the_gathered_arrays(N):
    v, idx = fixture_values(N), fixture_rows(N)
    ref = bootstrap_reference(v, dense_rank(v), idx)
    assert (ref["status"] == 0).all()
    base = N * (N + 1) ** 2
    for b in range(idx.shape[0]):
        assert_metrics_close(ref["metrics"][b], bootstrap_brute(v, idx[b]), N)
    # the special rows and columns are what they say: the all-one-index row is constant in every column, the last column everywhere
    const_row = idx.shape[0] - 3
    assert (ref["ranks"][const_row] == base).all() and np.isnan(ref["metrics"][const_row][:, [0, 3, 4]]).all()
    assert not np.isnan(ref["metrics"][..., 1:3]).any()                   # mse and rmse are always defined
    assert (ref["ranks"][:, -1, 1] == base).all() and np.isnan(ref["metrics"][:, -1, 3:]).all()
    if N >= 19:
        live = ref["ranks"][:4, 0, :]
        assert (live[:, 1] > base).all() and (live[:, 2] > base).all() and not np.isnan(ref["metrics"][:4, 0]).any()
        assert (np.abs(ref["metrics"][:4, :, 0]) <= 3).all()              # the conditioning the tolerance asks for


@pytest.mark.parametrize("N", HOST_SIZES)
def test_restatement_against_exact_rational_arithmetic(N):
    """The float64 restatement lies within a QUARTER of the line from the exact value, so a device result may use the rest."""
    v, idx = fixture_values(N), fixture_rows(N, n_random=3)
    ref = bootstrap_reference(v, dense_rank(v), idx)
    worst = 0.0
    for b in range(idx.shape[0]):
        want = bootstrap_exact(v, idx[b])
        got = ref["metrics"][b]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        live = ~np.isnan(want)
        err = np.abs(got[live] - want[live])
        line = np.where(np.broadcast_to(np.arange(5) == 3, want.shape), SPEARMAN_TOL, value_tol(N, np.nan_to_num(want)))[live]
        worst = max(worst, float((err / line).max()))
        if b < 4 and N >= 19:                                             # the random rows and the identity row: well conditioned
            std, mean = v[:2, idx[b]].astype(np.float64).std(axis=1), v[:2, idx[b]].astype(np.float64).mean(axis=1)
            assert (np.abs(mean) <= 3 * std).all() and (np.abs(want[:2, 0]) <= 3).all()
    print(f"N={N}: worst |restatement - exact| / line = {worst:.3g}")
    assert worst <= 0.25


def test_ordinal_ranks_move_spearman_in_every_resample():
    """A condition on the reference alone: ranks without tie averaging move spearman in every random resample of the fixture, so
    a kernel that ignored ties could not pass the device comparison."""
    moved = 0
    for N in (19, 257, 1000):
        v, idx = fixture_values(N, M=1), fixture_rows(N, n_random=6)[:6]
        for b in range(6):
            tied, ordinal = bootstrap_exact(v, idx[b])[0, 3], bootstrap_exact(v, idx[b], ordinal=True)[0, 3]
            assert abs(tied - ordinal) > 100 * SPEARMAN_TOL, (N, b)
            moved += 1
    assert moved == 18


def test_spearman_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    N = 257
    v, idx = fixture_values(N), fixture_rows(N)
    ref = bootstrap_reference(v, dense_rank(v), idx[:3])
    for b in range(3):
        for m in range(2):
            want = stats.spearmanr(v[m + 1, idx[b]], v[0, idx[b]]).statistic
            assert abs(ref["metrics"][b, m, 3] - want) <= 1e-13


def test_tie_groups_from_torch_unique():
    import torch
    from thermompnn_amd.bootstrap import dense_rank as torch_rank
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    col = np.array([0.0, -0.0, one, up, -0.0, up, one, -1.5, 0.0], np.float32)
    v = np.stack([col, col[::-1]])
    gid = torch_rank(torch.from_numpy(v.copy())).numpy()
    assert gid.dtype == np.int32
    np.testing.assert_array_equal(gid[0], [1, 1, 2, 3, 1, 3, 2, 0, 1])     # +-0.0 share a group; one ulp apart do not
    np.testing.assert_array_equal(gid, dense_rank(v))
    f = fixture_values(257)
    np.testing.assert_array_equal(torch_rank(torch.from_numpy(f)).numpy(), dense_rank(f))
    special = f[1]                                                        # M = 3: the column of +-0.0 and one-ulp neighbours
    assert {0x00000000, 0x80000000, 0x3f800000, 0x3f800001} <= set(special.view(np.uint32).tolist())


# ---- the C entry before any launch -------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    from thermompnn_amd import _lib
    lib = _lib.load()
    d = C.c_void_p(256)                                                   # never dereferenced: every call below fails before a launch
    ptrs = ("values", "gid", "idx", "metrics", "ranks", "status", "workspace")

    def call(Cn=2, N=100, B=10, flags=1, workspace_bytes=0, **kw):
        p = {name: kw.get(name, d) for name in ptrs}
        return lib.tmpnn_bootstrap_metrics(p["values"], p["gid"], Cn, N, p["idx"], B, p["metrics"], p["ranks"], p["status"], p["workspace"],
                                           workspace_bytes, flags, None)

    for name in ptrs:
        assert call(**{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    for name in ptrs[:-1]:                                                # the LDS form takes no workspace; the others still count
        assert call(flags=0, workspace=None, **{name: None}) == -1 and b"null" in lib.tmpnn_last_error(), name
    assert call(Cn=1) == -1 and b"C=1" in lib.tmpnn_last_error()
    assert call(Cn=10) == -1 and b"C=10" in lib.tmpnn_last_error()
    assert call(N=-1) == -1 and call(B=-1) == -1 and b"sizes" in lib.tmpnn_last_error()
    assert call(flags=2) == -1 and b"flag" in lib.tmpnn_last_error()
    assert call(N=MAX_N + 1) == -2 and b"1048576" in lib.tmpnn_last_error()       # TMPNN_E_UNSUPPORTED
    assert call(B=MAX_B + 1) == -2 and b"1048576" in lib.tmpnn_last_error()
    need = lib.tmpnn_bootstrap_workspace_bytes(2, 100, 10, 1)
    assert need >= 10 * 2 * 100 * 4
    assert call(workspace_bytes=need - 300) == -4 and b"workspace" in lib.tmpnn_last_error()      # TMPNN_E_WORKSPACE
    assert call(N=LDS_N + 1, flags=0, workspace_bytes=1000) == -4
    # B == 0 or N == 0 is a no-op and needs no address
    assert call(B=0) == 0 and call(N=0) == 0
    assert call(B=0, **{name: None for name in ptrs}) == 0 and call(N=0, **{name: None for name in ptrs}) == 0
    assert call(B=0, Cn=1) == -1 and call(N=0, B=MAX_B + 1) == -2         # the errors come first
    assert (_lib.BOOT_LDS_N, _lib.BOOT_MAX_N, _lib.BOOT_MAX_B, _lib.BOOT_MAX_M) == (LDS_N, MAX_N, MAX_B, MAX_M)
    assert _lib.BOOT_LDS_N >= 8192 and _lib.BOOT_METRICS == METRICS
    assert lib.tmpnn_version() == 200


def test_workspace_bytes_is_monotone_in_n():
    from thermompnn_amd import _lib
    lib = _lib.load()
    sizes = [1, 2, 3, 19, 257, 1000, LDS_N, LDS_N + 1, 40001, 1 << 18, MAX_N]
    for B in (1, 37, 300, MAX_B):
        forced = [lib.tmpnn_bootstrap_workspace_bytes(2, N, B, 1) for N in sizes]
        assert all(a <= b for a, b in zip(forced, forced[1:])) and forced[0] > 0
        assert all(f >= min(B, 256) * 2 * N * 4 for f, N in zip(forced, sizes))
        plain = [lib.tmpnn_bootstrap_workspace_bytes(2, N, B, 0) for N in sizes]
        assert all(a <= b for a, b in zip(plain, plain[1:]))
        assert all((p == 0) == (N <= LDS_N) for p, N in zip(plain, sizes))        # the LDS form needs none
        assert all(p == f for p, f, N in zip(plain, forced, sizes) if N > LDS_N)
    assert lib.tmpnn_bootstrap_workspace_bytes(9, MAX_N, 1, 0) == lib.tmpnn_bootstrap_workspace_bytes(2, MAX_N, 1, 0)
    assert lib.tmpnn_bootstrap_workspace_bytes(1, 100, 10, 1) == 0 and lib.tmpnn_bootstrap_workspace_bytes(2, MAX_N + 1, 10, 1) == 0


def test_binding_refuses_cpu_tensors():
    import torch
    from thermompnn_amd._lib import TmpnnError
    from thermompnn_amd.bootstrap import bootstrap_metrics, bootstrap_stats
    with pytest.raises(TmpnnError, match="device"):
        bootstrap_stats(torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(TmpnnError, match="host loop"):
        bootstrap_metrics(np.zeros(4), np.ones(4), 3, device="cpu")


# ---- the command line on the host ---------------------------------------------------------------------------------------------------
def _write_preds(path, N=60, extra=False, seed=3):
    """a raw-predictions file in the layout run_prediction_keep_preds writes, with rows that lack a measured value"""
    rng = np.random.default_rng(seed)
    t = np.round(rng.normal(-0.7, 1.5, N) * 2) / 2
    p, q = 0.6 * t + rng.normal(0, 1, N), 0.2 * t + rng.normal(0, 1, N)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["", "WT Seq", "Model", "Dataset", "ddG_true", "ddG_pred"] + (["other"] if extra else []))
        for i in range(N):
            gone = i % 17 == 5
            w.writerow([i, "ACD", "m", "d", "" if gone else t[i], "" if gone else p[i]] + ([q[i]] if extra else []))
    keep = np.arange(N) % 17 != 5
    return t[keep], p[keep], q[keep]


def test_cli_on_the_host_writes_the_reference_layout(tmp_path):
    from thermompnn_amd.bootstrap import bootstrap_metrics_host, main, read_columns
    src, out = str(tmp_path / "m_d_raw_preds.csv"), str(tmp_path / "boot.csv")
    t, p, _ = _write_preds(src)
    assert main(["-i", src, "-o", out, "-it", "12", "-gpu", "n", "--seed", "5"]) == 0
    lines = open(out).read().split("\n")
    assert lines[0] == ",r2,mse,rmse,spearman,pearson" and lines[-1] == "" and len(lines) == 14
    res = bootstrap_metrics_host(*read_columns(src), 12, seed=5)
    assert res.n == len(t) and res.samples.shape == (12, 1, 5)
    rng = np.random.default_rng(5)
    from thermompnn_amd.metrics import get_metrics
    for i, line in enumerate(lines[1:-1]):
        f = line.split(",")
        row = rng.integers(0, len(t), len(t))
        want = get_metrics(p.astype(np.float32)[row], t.astype(np.float32)[row])
        assert f[0] == str(i) and f[1:] == [str(np.float32(want[k])) for k in METRICS]
    pd = pytest.importorskip("pandas")
    buf = io.StringIO()
    pd.DataFrame(columns=list(METRICS), data=res.samples[:, 0].astype(np.float32)).to_csv(buf, index=True)
    assert buf.getvalue() == open(out).read()                             # byte for byte what the reference's frame writes


def test_cli_writes_nan_as_an_empty_field_and_prefixes_several_columns(tmp_path):
    from thermompnn_amd.bootstrap import BootstrapResult, main, write_samples_csv
    src, out, summ = str(tmp_path / "in.csv"), str(tmp_path / "boot.csv"), str(tmp_path / "summary.csv")
    _write_preds(src, extra=True)
    assert main(["-i", src, "-o", out, "-it", "9", "-gpu", "n", "--pred", "ddG_pred", "other", "--summary", summ]) == 0
    head = open(out).readline().strip().split(",")
    assert head == [""] + [f"{c}:{k}" for c in ("ddG_pred", "other") for k in METRICS]
    rows = list(csv.reader(open(summ)))
    assert rows[0] == ["column", "metric", "n", "point", "mean", "std", "lo", "hi", "share"] and len(rows) == 1 + 10 + 5
    assert rows[11][0] == "ddG_pred - other" and 0.0 <= float(rows[11][-1]) <= 1.0
    with pytest.raises(ValueError, match="no column 'absent'"):
        main(["-i", src, "-o", out, "-it", "2", "-gpu", "n", "--pred", "absent"])
    samples = np.array([[[0.5, 1.0, 1.0, np.nan, np.nan]], [[np.nan, 0.25, 0.5, 1 / 3, -0.1]]])
    nan_out = str(tmp_path / "nan.csv")
    write_samples_csv(nan_out, BootstrapResult(["ddG_pred"], samples, samples[0], 4))
    text = open(nan_out).read()
    assert text == ",r2,mse,rmse,spearman,pearson\n0,0.5,1.0,1.0,,\n1,,0.25,0.5,0.33333334,-0.1\n"
    pd = pytest.importorskip("pandas")
    buf = io.StringIO()
    pd.DataFrame(columns=list(METRICS), data=samples[:, 0].astype(np.float32)).to_csv(buf, index=True)
    assert buf.getvalue() == text


def test_summary_and_difference_against_numpy_percentiles():
    from thermompnn_amd.bootstrap import BootstrapResult
    rng = np.random.default_rng(11)
    samples = rng.normal(0.5, 0.1, (400, 2, 5))
    samples[::7, 1, 3] = np.nan                                           # resamples in which a column was constant
    res = BootstrapResult(["a", "b"], samples, np.nanmean(samples, axis=0), 123)
    s = res.summary(0.9)
    col = samples[:, 0, 2]
    near = lambda x: pytest.approx(float(x), rel=1e-12, abs=0)            # (the level arrives as 50 (1 -+ 0.9): an ulp off 5 and 95)
    assert s["a"]["rmse"] == dict(point=float(res.point[0, 2]), mean=float(col.mean()), std=float(col.std(ddof=1)),
                                  lo=near(np.percentile(col, 5.0)), hi=near(np.percentile(col, 95.0)))
    live = samples[:, 1, 3][~np.isnan(samples[:, 1, 3])]
    assert s["b"]["spearman"]["mean"] == float(live.mean()) and s["b"]["spearman"]["hi"] == near(np.percentile(live, 95.0))
    lo95, hi95 = np.percentile(samples[:, 1, 0], [2.5, 97.5])
    assert (res.summary()["b"]["r2"]["lo"], res.summary()["b"]["r2"]["hi"]) == (near(lo95), near(hi95))
    d = res.difference("a", "b", 0.9)
    diff = samples[:, 0, 1] - samples[:, 1, 1]
    assert d["mse"]["share"] == float((diff < 0).mean()) and d["mse"]["lo"] == near(np.percentile(diff, 5.0))       # lower wins
    diff = (samples[:, 0, 3] - samples[:, 1, 3])
    diff = diff[~np.isnan(diff)]
    assert diff.size == 400 - len(range(0, 400, 7))
    assert d["spearman"]["share"] == float((diff > 0).mean()) and d["spearman"]["mean"] == float(diff.mean())        # higher wins
    assert res.difference(0, 1, 0.9) == d
