"""Bootstrap confidence intervals of the benchmark metrics (the reference's analysis/bootstrap.py) on the device.

The reference resamples the rows of ``<model>_<dataset>_raw_preds.csv`` with replacement ``-it`` times and scores every resample with
torchmetrics: a sort per metric column per iteration. Here no resample is sorted: a resample only re-weights the distinct values of a
column, so its tie-averaged ranks follow from one histogram over the tie groups of the ORIGINAL column and one prefix sum
(tmpnn_bootstrap_metrics, csrc/tmpnn_bootstrap.hip; include/tmpnn.h has the contract). One launch scores a block of resamples.

    python -m thermompnn_amd.bootstrap -i IN.csv -o OUT.csv -it N [-gpu y|n] [--pred COL ...] [--seed S] [--summary FILE]
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import BOOT_METRICS as METRICS
from ._lib import TmpnnError, check

IDX_BLOCK_BYTES = 64 << 20          # the default draw_block keeps a block of idx at or below this
HIGHER_IS_BETTER = (True, False, False, True, True)     # r2, mse, rmse, spearman, pearson


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bootstrap_stats(values, gid, idx, force_workspace: bool = False, out: Optional[dict] = None):
    """The thin binding of tmpnn_bootstrap_metrics: ``values`` [C, N] float32 (row 0 the measured column), ``gid`` [C, N] int32 (the
    dense rank of every value among its column's distinct values), ``idx`` [B, N] int32 (the draws), all on the device.
    -> (metrics [B, C - 1, 5] float64, ranks [B, C - 1, 3] int64, status [B] int32) on the device. ``force_workspace`` runs the
    workspace form at any N (the LDS form serves N <= BOOT_LDS_N otherwise). ``out``: dict(metrics, ranks, status) to write into;
    a resample with status != 0 leaves its rows of metrics and ranks as it found them (NaN and 0 in arrays made here)."""
    import torch
    for name, t, dt in (("values", values, torch.float32), ("gid", gid, torch.int32), ("idx", idx, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or t.dim() != 2:
            raise TmpnnError(f"bootstrap_stats: {name} must be a 2-d {dt} tensor on the device (there is no CPU path)")
    values, gid, idx = values.contiguous(), gid.contiguous(), idx.contiguous()
    Cn, N = int(values.shape[0]), int(values.shape[1])
    B = int(idx.shape[0])
    if tuple(gid.shape) != (Cn, N) or int(idx.shape[1]) != N:
        raise TmpnnError(f"bootstrap_stats: values {tuple(values.shape)}, gid {tuple(gid.shape)} and idx {tuple(idx.shape)} do not agree")
    if not 2 <= Cn <= _lib.BOOT_MAX_M + 1:
        raise TmpnnError(f"bootstrap_stats: {Cn} columns; the measured one and 1 to {_lib.BOOT_MAX_M} predictions are served")
    if N > _lib.BOOT_MAX_N or B > _lib.BOOT_MAX_B:
        raise TmpnnError(f"bootstrap_stats: N={N} or B={B} exceeds 2^20 per call")
    dev, M = values.device, Cn - 1
    if out is None:
        out = dict(metrics=torch.full((B, M, 5), float("nan"), dtype=torch.float64, device=dev),
                   ranks=torch.zeros((B, M, 3), dtype=torch.int64, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev))
    metrics, ranks, status = out["metrics"], out["ranks"], out["status"]
    for t, shape, dt in ((metrics, (B, M, 5), torch.float64), (ranks, (B, M, 3), torch.int64), (status, (B,), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise TmpnnError(f"bootstrap_stats: an output must be a contiguous {dt} tensor of shape {shape} on {dev}")
    if B == 0 or N == 0:
        return metrics, ranks, status
    lib = _lib.load()
    flags = _lib.BOOT_FORCE_WORKSPACE if force_workspace else 0
    nbytes = int(lib.tmpnn_bootstrap_workspace_bytes(Cn, N, B, flags))
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib.tmpnn_bootstrap_metrics(_ptr(values), _ptr(gid), Cn, N, _ptr(idx), B, _ptr(metrics), _ptr(ranks), _ptr(status), _ptr(ws),
                                          nbytes, flags, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tmpnn_bootstrap_metrics")
    return metrics, ranks, status


def dense_rank(values):
    """gid [C, N] int32 on ``values``' device: per column the 0-based rank of every value among the column's distinct values
    (torch.unique: equality is IEEE ==, so -0.0 and +0.0 share a group). Plumbing, once per dataset."""
    import torch
    return torch.stack([torch.unique(values[c], sorted=True, return_inverse=True)[1] for c in range(values.shape[0])]).to(torch.int32)


def _columns(pred, truth) -> Tuple[List[str], np.ndarray]:
    """-> names [M], values [1 + M, N] float32 with the rows dropped that hold a non-finite entry in any column"""
    if isinstance(pred, dict):
        names, cols = [str(k) for k in pred], [np.asarray(v, np.float32).reshape(-1) for v in pred.values()]
    else:
        p = np.asarray(pred, np.float32)
        cols = [p.reshape(-1)] if p.ndim <= 1 else [p[m] for m in range(p.shape[0])]
        names = ["ddG_pred"] if len(cols) == 1 else [f"pred{m}" for m in range(len(cols))]
    t = np.asarray(truth, np.float32).reshape(-1)
    if not 1 <= len(cols) <= _lib.BOOT_MAX_M:
        raise ValueError(f"bootstrap: {len(cols)} prediction columns; 1 to {_lib.BOOT_MAX_M} are served")
    if any(c.shape != t.shape for c in cols):
        raise ValueError(f"bootstrap: every prediction column must have the {t.size} entries of the measured one")
    values = np.stack([t] + cols)
    values = np.ascontiguousarray(values[:, np.isfinite(values).all(axis=0)])
    if values.shape[1] == 0:
        raise ValueError("bootstrap: no row with finite values in every column")
    if values.shape[1] > _lib.BOOT_MAX_N:
        raise ValueError(f"bootstrap: {values.shape[1]} rows exceed 2^20")
    return names, values


def default_draw_block(N: int, iterations: int) -> int:
    return max(1, min(max(1, int(iterations)), IDX_BLOCK_BYTES // (4 * max(1, N)), _lib.BOOT_MAX_B))


def draw_blocks(N: int, iterations: int, seed: int, device, draw_block: Optional[int] = None):
    """The blocks of draws ``bootstrap_metrics`` scores, in its order: torch.randint(0, N, (rows, N), int32) from ONE generator of
    ``device`` seeded with ``seed``, ``draw_block`` resamples at a time. (seed, N, draw_block) together fix the draws: another block
    size consumes the generator's stream in other portions."""
    import torch
    block = default_draw_block(N, iterations) if draw_block is None else max(1, min(int(draw_block), _lib.BOOT_MAX_B))
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    done = 0
    while done < iterations:
        rows = min(block, iterations - done)
        yield torch.randint(0, N, (rows, N), dtype=torch.int32, generator=gen, device=device)
        done += rows


@dataclass
class BootstrapResult:
    names: List[str]
    samples: np.ndarray            # [B, M, 5] float64; NaN where a resample left the metric undefined (a constant column)
    point: np.ndarray              # [M, 5]: the dataset as it is
    n: int                         # rows that were resampled

    def _col(self, c) -> int:
        return self.names.index(c) if isinstance(c, str) else int(c)

    def summary(self, level: float = 0.95) -> Dict[str, Dict[str, Dict[str, float]]]:
        """name -> metric -> dict(point, mean, std, lo, hi): mean, standard deviation (ddof = 1) and the percentile interval
        [(1 - level) / 2, (1 + level) / 2] over the resamples in which the metric is defined"""
        q = [50.0 * (1.0 - level), 50.0 * (1.0 + level)]
        out = {}
        for m, name in enumerate(self.names):
            out[name] = {}
            for k, metric in enumerate(METRICS):
                s = self.samples[:, m, k]
                s = s[~np.isnan(s)]
                lo, hi = (np.percentile(s, q) if s.size else (np.nan, np.nan))
                out[name][metric] = dict(point=float(self.point[m, k]), mean=float(s.mean()) if s.size else float("nan"),
                                         std=float(s.std(ddof=1)) if s.size > 1 else float("nan"), lo=float(lo), hi=float(hi))
        return out

    def difference(self, a, b, level: float = 0.95) -> Dict[str, Dict[str, float]]:
        """Paired comparison of two columns (both saw the same resamples): metric -> dict(point, mean, lo, hi) of a - b and
        ``share``, the share of resamples in which a beats b (higher r2, spearman, pearson; lower mse, rmse), over the resamples
        in which the metric is defined for both."""
        ia, ib = self._col(a), self._col(b)
        q = [50.0 * (1.0 - level), 50.0 * (1.0 + level)]
        out = {}
        for k, metric in enumerate(METRICS):
            d = self.samples[:, ia, k] - self.samples[:, ib, k]
            d = d[~np.isnan(d)]
            lo, hi = (np.percentile(d, q) if d.size else (np.nan, np.nan))
            wins = (d > 0) if HIGHER_IS_BETTER[k] else (d < 0)
            out[metric] = dict(point=float(self.point[ia, k] - self.point[ib, k]), mean=float(d.mean()) if d.size else float("nan"),
                               lo=float(lo), hi=float(hi), share=float(wins.mean()) if d.size else float("nan"))
        return out


def bootstrap_metrics(pred, truth, iterations: int, seed: int = 0, device="cuda", draw_block: Optional[int] = None) -> BootstrapResult:
    """``iterations`` resamples with replacement (N draws each, the reference's ``frac=1``) of the rows of ``pred`` ([N], [M, N] or
    a dict name -> array, M <= 8) and ``truth`` [N], scored on the device. Rows with a non-finite entry in any column are dropped,
    as the reference's ``dropna`` and ``get_metrics`` do. The draws are ``draw_blocks``'s: (seed, N, draw_block) together fix them;
    the default block keeps ``idx`` at or below 64 MB. ``point`` comes from one more call with the identity row arange(N)."""
    import torch
    names, values = _columns(pred, truth)
    N, M = values.shape[1], values.shape[0] - 1
    dev = torch.device(device)
    if dev.type != "cuda":
        raise TmpnnError("bootstrap_metrics runs on the device; bootstrap_metrics_host is the host loop")
    v = torch.from_numpy(values).to(dev)
    gid = dense_rank(v)
    iterations = int(iterations)
    samples = np.empty((iterations, M, 5), np.float64)
    done = 0
    for idx in draw_blocks(N, iterations, seed, dev, draw_block):
        metrics, _, status = bootstrap_stats(v, gid, idx)
        if int(status.abs().max()) != 0:
            raise TmpnnError("bootstrap_metrics: a resample was refused (status != 0)")
        samples[done:done + idx.shape[0]] = metrics.cpu().numpy()
        done += idx.shape[0]
    point, _, status = bootstrap_stats(v, gid, torch.arange(N, dtype=torch.int32, device=dev)[None])
    if int(status[0]) != 0:
        raise TmpnnError("bootstrap_metrics: the identity resample was refused (status != 0)")
    return BootstrapResult(names, samples, point[0].cpu().numpy(), N)


def bootstrap_metrics_host(pred, truth, iterations: int, seed: int = 0) -> BootstrapResult:
    """The reference's loop on the host (``-gpu n``): numpy draws, metrics.get_metrics per resample and column."""
    from .metrics import get_metrics
    names, values = _columns(pred, truth)
    N, M = values.shape[1], values.shape[0] - 1
    rng = np.random.default_rng(int(seed))
    samples = np.empty((int(iterations), M, 5), np.float64)
    for b in range(int(iterations)):
        row = rng.integers(0, N, N)
        for m in range(M):
            r = get_metrics(values[m + 1, row], values[0, row])
            samples[b, m] = [r[k] for k in METRICS]
    point = np.array([[get_metrics(values[m + 1], values[0])[k] for k in METRICS] for m in range(M)], np.float64).reshape(M, 5)
    return BootstrapResult(names, samples, point, N)


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def read_columns(path: str, pred: Sequence[str] = ("ddG_pred",), truth: str = "ddG_true"):
    """-> ({name: float32 array}, truth array) of a raw-predictions CSV; an empty or unreadable field is NaN (dropped later)"""
    def num(s):
        try:
            return float(s)
        except (TypeError, ValueError):
            return float("nan")
    with open(path, newline="") as fh:
        rd = csv.DictReader(fh)
        missing = [c for c in (truth, *pred) if c not in (rd.fieldnames or [])]
        if missing:
            raise ValueError(f"{path}: no column {missing[0]!r} (found {rd.fieldnames})")
        rows = list(rd)
    return ({c: np.array([num(r[c]) for r in rows], np.float32) for c in pred}, np.array([num(r[truth]) for r in rows], np.float32))


def _f32(x: float) -> str:
    """How the reference's float32 frame lands in its CSV: the shortest text that reads back as the same float32; NaN empty"""
    return "" if x != x else str(np.float32(x))


def write_samples_csv(path: str, res: BootstrapResult) -> None:
    """The reference's OUT.csv: an unnamed index, then r2, mse, rmse, spearman, pearson, stored as float32. Several prediction
    columns: every metric column carries a ``<col>:`` prefix."""
    many = len(res.names) > 1
    head = [f"{n}:{k}" if many else k for n in res.names for k in METRICS]
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow([""] + head)
        for i in range(res.samples.shape[0]):
            w.writerow([i] + [_f32(x) for x in res.samples[i].reshape(-1)])


def write_summary_csv(path: str, res: BootstrapResult, level: float = 0.95) -> None:
    """column, metric, n, point, mean, std, lo, hi per column and metric; then, for every pair of columns, the paired difference
    rows ``a - b`` with the share of resamples in which a beats b in the last field"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["column", "metric", "n", "point", "mean", "std", "lo", "hi", "share"])
        fmt = lambda x: "" if x != x else repr(float(x))
        for name, per in res.summary(level).items():
            for metric, s in per.items():
                w.writerow([name, metric, res.n] + [fmt(s[k]) for k in ("point", "mean", "std", "lo", "hi")] + [""])
        for i, a in enumerate(res.names):
            for b in res.names[i + 1:]:
                for metric, s in res.difference(a, b, level).items():
                    w.writerow([f"{a} - {b}", metric, res.n, fmt(s["point"]), fmt(s["mean"]), "", fmt(s["lo"]), fmt(s["hi"]), fmt(s["share"])])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="bootstrap sampling of a table of ddG predictions for metric estimation")
    ap.add_argument("-i", type=str, required=True, help="csv input filename")
    ap.add_argument("-o", type=str, help="csv output filename")
    ap.add_argument("-it", type=int, required=True, help="iterations to run bootstrapping")
    ap.add_argument("-gpu", type=str, default="y", help="use gpu or no?")
    ap.add_argument("--pred", nargs="+", default=["ddG_pred"], help="prediction column(s), up to 8")
    ap.add_argument("--truth", type=str, default="ddG_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--summary", type=str, help="csv of mean, std and 95 %% percentile interval per column and metric")
    args = ap.parse_args(argv)
    pred, truth = read_columns(args.i, args.pred, args.truth)
    if args.gpu == "y":
        res = bootstrap_metrics(pred, truth, args.it, seed=args.seed)
    else:
        res = bootstrap_metrics_host(pred, truth, args.it, seed=args.seed)
    if args.o:
        write_samples_csv(args.o, res)
    if args.summary:
        write_summary_csv(args.summary, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
