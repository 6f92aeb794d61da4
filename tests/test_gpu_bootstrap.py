"""Bootstrap intervals on the device (tmpnn_bootstrap_metrics, bootstrap.bootstrap_stats) and the front ends on top of it
(bootstrap_metrics, python -m thermompnn_amd.bootstrap, evaluate_datasets(bootstrap=...)) against the numpy restatement of the
contract (tests/bootstrap_restatement.py, whose conditions tests/test_bootstrap_host.py asserts). ``ranks`` and ``status`` are compared
exactly, ``metrics`` within the lines derived there (against exact rational arithmetic at N <= 1000), NaNs in the same places; the two
forms, another split of a batch and a rerun are compared bit for bit."""
import csv
import os

import numpy as np
import pytest
import torch

from bootstrap_restatement import (HOST_SIZES, LDS_N, MAX_N, METRICS, assert_bootstrap_close, assert_metrics_close, bootstrap_exact,
                                   bootstrap_reference, dense_rank, fixture_rows, fixture_values)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(v, gid, idx, force=False, out=None):
    """-> dict of numpy arrays from one call of the binding"""
    from thermompnn_amd.bootstrap import bootstrap_stats
    m, r, s = bootstrap_stats(_dev(v), _dev(gid), _dev(idx), force_workspace=force, out=out)
    torch.cuda.synchronize()
    return dict(metrics=m.cpu().numpy(), ranks=r.cpu().numpy(), status=s.cpu().numpy())


def _bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]) for k in ("metrics", "ranks", "status"))


@pytest.fixture(scope="module")
def refs():
    """{N: (values, gid, idx, restatement)} of the host fixtures (M = 3, eight rows); left unchanged by the tests that share it"""
    out = {}
    for N in HOST_SIZES:
        v, idx = fixture_values(N), fixture_rows(N)
        gid = dense_rank(v)
        out[N] = (v, gid, idx, bootstrap_reference(v, gid, idx))
    return out


@pytest.mark.parametrize("N", HOST_SIZES)
def test_host_fixtures_in_both_forms(refs, N):
    v, gid, idx, want = refs[N]
    exact = np.stack([bootstrap_exact(v, idx[b]) for b in range(idx.shape[0])])
    for force in (False, True):
        got = _run(v, gid, idx, force=force)
        assert (got["status"] == 0).all()
        assert_bootstrap_close(got, want, N)
        worst = assert_metrics_close(got["metrics"], exact, N)
        print(f"N={N} force={force}: worst |device - exact| / line = {worst:.3g}")


@pytest.mark.parametrize("N,rows", [(LDS_N, 8), (LDS_N + 1, 8), (40001, 3)])
def test_at_the_form_threshold_and_above(N, rows):
    v, idx = fixture_values(N, M=1), fixture_rows(N, n_random=1 if rows == 3 else 4)[:rows]
    gid = dense_rank(v)
    got = _run(v, gid, idx)
    assert_bootstrap_close(got, bootstrap_reference(v, gid, idx), N)
    assert (got["status"] == 0).all() and (got["ranks"][0] > N * (N + 1) ** 2).all()


def test_the_largest_n_and_a_count_of_n_in_one_bin():
    """N = 2^20: the largest integer sums (base = N (N + 1)^2 ~ 2^60, a random row beyond it) and, in the all-one-index row, a
    count of N in one bin."""
    N = MAX_N
    v = fixture_values(N, M=1)
    gid = dense_rank(v)
    idx = np.stack([np.random.default_rng(5).integers(0, N, N), np.full(N, N - 7)]).astype(np.int32)
    got = _run(v, gid, idx)
    want = bootstrap_reference(v, gid, idx)
    assert_bootstrap_close(got, want, N)
    base = N * (N + 1) ** 2
    assert (got["ranks"][1] == base).all() and got["ranks"][0, 0, 1] > base + (1 << 57) and np.isnan(got["metrics"][1, 0, [0, 3, 4]]).all()


@pytest.mark.parametrize("M,B", [(1, 1), (3, 5), (8, 37), (1, 300)])
def test_column_and_resample_counts(M, B):
    """B = 300 is more workgroups than the device has CUs: the persistent loop runs"""
    N = 257
    v = fixture_values(N, M=M, seed=M)
    gid = dense_rank(v)
    idx = np.random.default_rng(B).integers(0, N, (B, N)).astype(np.int32)
    want = bootstrap_reference(v, gid, idx)
    for force in (False, True):
        assert_bootstrap_close(_run(v, gid, idx, force=force), want, N)


@pytest.mark.parametrize("N", [19, 257, LDS_N])
def test_the_two_forms_agree_bit_for_bit(N):
    v, idx = fixture_values(N), fixture_rows(N)
    gid = dense_rank(v)
    lds, ws = _run(v, gid, idx), _run(v, gid, idx, force=True)
    assert not np.isnan(lds["metrics"][:4, :2]).any()
    assert _bits_equal(lds, ws)


def test_a_resample_does_not_depend_on_its_slot_or_on_a_rerun():
    N, B = 257, 37
    v = fixture_values(N)
    gid = dense_rank(v)
    idx = np.random.default_rng(37).integers(0, N, (B, N)).astype(np.int32)
    whole = _run(v, gid, idx)
    assert _bits_equal(whole, _run(v, gid, idx))                          # a rerun
    for cut in (1, 20):
        a, b = _run(v, gid, idx[:cut]), _run(v, gid, idx[cut:])
        joined = {k: np.concatenate([a[k], b[k]]) for k in a}
        assert _bits_equal(whole, joined), cut
    alone = _run(v, gid, idx[11:12], force=True)
    assert _bits_equal(alone, {k: whole[k][11:12] for k in whole})


def _sentinel(B, M):
    metrics = torch.full((B, M, 5), 0, dtype=torch.int64, device="cuda").fill_(0x4242424242424242).view(torch.float64)
    ranks = torch.full((B, M, 3), -12345, dtype=torch.int64, device="cuda")
    status = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    return dict(metrics=metrics, ranks=ranks, status=status)


@pytest.mark.parametrize("force", [False, True])
def test_bad_draws_get_status_minus_1_and_write_nothing(force):
    N = 257
    v = fixture_values(N)
    gid = dense_rank(v)
    idx = np.random.default_rng(1).integers(0, N, (7, N)).astype(np.int32)
    idx[1, 100], idx[3, 0], idx[5, N - 1] = -1, N, N + 5
    got = _run(v, gid, idx, force=force, out=_sentinel(7, 3))
    assert got["status"].tolist() == [0, -1, 0, -1, 0, -1, 0]
    want = bootstrap_reference(v, gid, idx)
    assert want["status"].tolist() == got["status"].tolist()
    for b in range(7):
        if b % 2:
            assert (got["metrics"][b].view(np.int64) == 0x4242424242424242).all() and (got["ranks"][b] == -12345).all()
        else:
            one = {k: got[k][b:b + 1] for k in got}
            assert_bootstrap_close(one, {k: want[k][b:b + 1] for k in want}, N)


@pytest.mark.parametrize("force", [False, True])
def test_a_bad_group_gets_status_minus_2_only_where_it_is_drawn(force):
    N = 257
    v = fixture_values(N)
    gid = dense_rank(v)
    idx = np.random.default_rng(2).integers(0, N - 1, (4, N)).astype(np.int32)       # no row draws index N - 1 ...
    idx[2, 50] = N - 1                                                               # ... but row 2
    bad = gid.copy()
    bad[2, N - 1] = N                                                                # a prediction column's group: outside [0, N)
    got = _run(v, bad, idx, force=force, out=_sentinel(4, 3))
    assert got["status"].tolist() == [0, 0, -2, 0]
    assert (got["metrics"][2].view(np.int64) == 0x4242424242424242).all() and (got["ranks"][2] == -12345).all()
    want = bootstrap_reference(v, bad, idx)
    assert want["status"].tolist() == [0, 0, -2, 0]
    keep = [0, 1, 3]
    assert_bootstrap_close({k: got[k][keep] for k in got}, {k: want[k][keep] for k in want}, N)
    bad0 = gid.copy()
    bad0[0, N - 1] = -3                                                              # the measured column's, negative
    assert _run(v, bad0, idx, force=force)["status"].tolist() == [0, 0, -2, 0]


# ---- the front ends -------------------------------------------------------------------------------------------------------------------
def test_bootstrap_metrics_equals_the_binding_on_the_same_draws():
    from thermompnn_amd.bootstrap import bootstrap_metrics, bootstrap_stats, dense_rank as torch_rank, draw_blocks
    from thermompnn_amd.metrics import get_metrics
    N = 1000
    v = fixture_values(N, M=2)
    pred = {"a": np.append(v[1], np.float32(np.nan)), "b": np.append(v[2], np.float32(1.0))}       # a row that is dropped
    truth = np.append(v[0], np.float32(0.5))
    res = bootstrap_metrics(pred, truth, 23, seed=9, draw_block=10)
    assert res.names == ["a", "b"] and res.n == N and res.samples.shape == (23, 2, 5) and res.point.shape == (2, 5)
    dv = _dev(v)
    gid = torch_rank(dv)
    assert np.array_equal(gid.cpu().numpy(), dense_rank(v))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    parts = []
    for rows in (10, 10, 3):
        idx = torch.randint(0, N, (rows, N), dtype=torch.int32, generator=gen, device="cuda")
        parts.append(bootstrap_stats(dv, gid, idx)[0].cpu().numpy())
    assert np.array_equal(np.concatenate(parts).view(np.int64), res.samples.view(np.int64))
    assert [int(b.shape[0]) for b in draw_blocks(N, 23, 9, "cuda", 10)] == [10, 10, 3]
    again = bootstrap_metrics(pred, truth, 23, seed=9, draw_block=10)
    assert np.array_equal(again.samples.view(np.int64), res.samples.view(np.int64))
    want = np.array([[get_metrics(v[m + 1], v[0])[k] for k in METRICS] for m in range(2)])
    assert_metrics_close(res.point, want, N)
    lo, hi = res.summary()["a"]["spearman"]["lo"], res.summary()["a"]["spearman"]["hi"]
    assert lo < res.point[0, 3] < hi and 0.0 <= res.difference("a", "b")["rmse"]["share"] <= 1.0


def test_cli_on_the_device_writes_the_reference_layout(tmp_path):
    from thermompnn_amd.bootstrap import main
    N = 120
    v = fixture_values(N, M=1)
    src, out = str(tmp_path / "m_d_raw_preds.csv"), str(tmp_path / "boot.csv")
    with open(src, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["", "Model", "ddG_true", "ddG_pred"])
        for i in range(N):
            w.writerow([i, "m", "" if i == 7 else float(v[0, i]), float(v[1, i])])
    assert main(["-i", src, "-o", out, "-it", "25", "--seed", "4"]) == 0
    rows = list(csv.reader(open(out)))
    assert rows[0] == ["", *METRICS] and [r[0] for r in rows[1:]] == [str(i) for i in range(25)]
    vals = np.array([[float(x) for x in r[1:]] for r in rows[1:]])
    assert all(r[k + 1] == str(np.float32(vals[i, k])) for i, r in enumerate(rows[1:]) for k in range(5))      # float32, as stored
    keep = np.arange(N) != 7
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    idx = torch.randint(0, N - 1, (25, N - 1), dtype=torch.int32, generator=gen, device="cuda").cpu().numpy()
    want = bootstrap_reference(v[:, keep], dense_rank(v[:, keep]), idx)["metrics"][:, 0]
    # the file holds the float32 rounding of a value within the line (far below a float32 ulp) of the restatement's: the same
    # float32 or, where the two straddle a rounding boundary, its neighbour
    f32 = want.astype(np.float32)
    assert (np.abs(vals.astype(np.float32) - f32) <= np.spacing(np.abs(f32))).all()
    assert (vals.astype(np.float32) == f32).mean() > 0.9


def test_evaluate_datasets_writes_the_bootstrap_file_and_leaves_the_rest(tmp_path):
    from conftest import GOLDEN
    from thermompnn_amd import custom_inference
    from thermompnn_amd.datasets import ddgBenchDataset
    from thermompnn_amd.thermompnn_benchmarking import evaluate_datasets
    ds = ddgBenchDataset(None, GOLDEN, os.path.join(GOLDEN, "ddgbench_sample.csv"))
    model = custom_inference.load_model(None, None, 0)
    plain, boot = tmp_path / "plain", tmp_path / "boot"
    plain.mkdir()
    boot.mkdir()
    a = evaluate_datasets({"ThermoMPNN": model}, {"sample": ds}, out_dir=str(plain))
    b = evaluate_datasets({"ThermoMPNN": model}, {"sample": ds}, out_dir=str(boot), bootstrap=50, seed=3)
    assert a == b and (plain / "ThermoMPNN_metrics.csv").read_bytes() == (boot / "ThermoMPNN_metrics.csv").read_bytes()
    assert not (plain / "ThermoMPNN_metrics_bootstrap.csv").exists()
    rows = list(csv.reader(open(boot / "ThermoMPNN_metrics_bootstrap.csv")))
    assert rows[0] == ["", "Model", "Dataset", "n"] + [f"ddG {k} {s}" for k in METRICS for s in ("mean", "std", "lo", "hi")]
    assert len(rows) == 2 and rows[1][:4] == ["0", "ThermoMPNN", "sample", str(a[0]["n"])]
    mean, std, lo, hi = (float(x) for x in rows[1][8:12])                 # mse
    assert lo <= mean <= hi and std > 0 and lo >= 0
