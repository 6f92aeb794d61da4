"""bench.py's roofline arithmetic and helpers, without a GPU: the numbers the JSON line derives from kernel durations."""
import csv
import io
import os
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, REPO)


def test_both_roofs_of_the_bench_batch():
    """64 x L=256, K=48: the edge update moves 2 E_b + node operands = 825 229 312 algorithmic bytes and 77.3 GFLOP per launch; against
    8 TB/s and 2.5 PF / 3 MFMAs that is 103.15 us (HBM) vs 92.77 us (MFMA): HBM binds, and `frac` is taken against it."""
    import bench
    T, edges = 16384, 16384 * 48
    assert bench.kernel_bytes("enc_edge", T, edges) == 2 * 512.0 * edges + 2 * 512.0 * T + 192.0 * T == 825229312.0
    assert bench.kernel_flops("enc_edge", T, edges) == 2.0 * edges * 3 * 128 * 128
    r = bench.kernel_roofs("enc_edge", T, edges, 0.2933, "f16x2")
    assert r["bound"] == "hbm" and abs(r["t_hbm_us"] - 103.1537) < 1e-3 and abs(r["t_mfma_us"] - 92.7713) < 1e-3
    assert abs(r["frac"] - 103.1537 / 293.3) < 1e-4 and abs(r["hbm"]["achieved_GBps"] - 825229312.0 / 0.2933e-3 / 1e9) < 1e-6
    assert r["mfma"]["terms"] == 3 and abs(r["mfma"]["peak_TFLOPs"] - 2500.0 / 3) < 1e-9
    # the message kernels read h_E once: the matrix cores bind them (61.85 us vs 53.9 us of HBM)
    m = bench.kernel_roofs("enc_msg", T, edges, 0.211, "f16x2")
    assert m["bound"] == "mfma" and abs(m["t_mfma_us"] - 2.0 * edges * 2 * 128 * 128 / (2500e12 / 3) * 1e6) < 1e-6
    # other precisions: bf16x3 = 6 MFMAs per multiply-accumulate on the per-edge kernels, fp32 MFMA everywhere else / in fp32 mode
    assert bench.kernel_roofs("enc_edge", T, edges, 0.55, "bf16x3")["mfma"]["terms"] == 6
    assert bench.kernel_roofs("node_update", T, edges, 0.04, "bf16x3")["mfma"]["terms"] == 0
    f = bench.kernel_roofs("enc_edge", T, edges, 0.77, "fp32")
    assert f["mfma"]["terms"] == 0 and f["mfma"]["peak_TFLOPs"] == bench.FP32_MFMA_PEAK_TFLOPS and f["bound"] == "mfma"
    # a kernel without matrix work is judged on bytes alone
    k = bench.kernel_roofs("knn", T, edges, 0.066, "f16x2")
    assert k["bound"] == "hbm" and k["t_mfma_us"] == 0.0


def test_usable_cpus_and_host_info():
    import bench
    n, quota = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1) and (quota is None or quota > 0)
    info = bench.host_cpu_info()
    assert info["affinity_cpus"] == n and info["host_cpus"] == os.cpu_count()


def test_pmc_traffic_is_refused_for_other_batches_or_sources():
    import bench
    assert bench.pmc_traffic("enc_edge", 12345) is None                  # the PMC passes were taken at T = 16384 only
    got = bench.pmc_traffic("enc_edge", 16384)
    assert got is None or 0.99 < got / 825229312.0 < 1.05                # null (sources changed since the pass) or ~ the algorithmic bytes


def test_live_pmc_pass_never_raises_and_says_why(monkeypatch):
    """bench.py measures the dominant kernel's HBM bytes in two rocprofv3 --pmc child passes inside the default run (round 6). The bench
    line must never depend on them: under a profiler, without rocprofv3, or on a box where the passes fail, the function returns
    (None, reason) and the committed, hash-stamped file is quoted instead."""
    import bench
    monkeypatch.setenv("ROCP_TOOL_LIBRARIES", "/nonexistent/librocprofiler-sdk-tool.so")
    res, why = bench.live_pmc_traffic({"enc_edge": "enc_edge"})
    assert res is None and "profiler" in why
    monkeypatch.delenv("ROCP_TOOL_LIBRARIES")
    monkeypatch.setenv("PATH", "/nonexistent")
    monkeypatch.setattr(bench.os.path, "exists", lambda p: False)
    res, why = bench.live_pmc_traffic({"enc_edge": "enc_edge"})
    assert res is None and "rocprofv3" in why


def test_rocprof_timed_stats_keeps_the_timed_launches_only(tmp_path):
    """tools/rocprof_timed_stats.py: of a kernel trace with slow warm-up launches, only the last steps x launches-per-step count."""
    rows = [("Kernel_Name", "Start_Timestamp", "End_Timestamp")]
    t = 0
    for step in range(7):                                                # 5 slow warm-up steps, then 2 timed ones
        for name, per, dur in (("void enc_edge8_rp_kernel<SplitH2, false, true>(EdgeArgsB)", 3, 400 if step < 5 else 300),
                               ("void knn_kernel<4>(float const*)", 1, 90 if step < 5 else 60), ("unrelated_kernel()", 1, 5)):
            for _ in range(per):
                rows.append((name, t, t + dur))
                t += dur + 10
    p = tmp_path / "trace.csv"
    with open(p, "w", newline="") as fh:
        csv.writer(fh).writerows(rows)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "rocprof_timed_stats.py"), str(p), "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {row["Kernel_Name"]: row for row in csv.DictReader(io.StringIO(r.stdout))}
    edge = out["void enc_edge8_rp_kernel<SplitH2, false, true>"]
    assert int(edge["TimedLaunches"]) == 6 and float(edge["AvgNs"]) == 300.0 and int(edge["AllLaunches"]) == 21
    assert abs(float(edge["AvgNsAllLaunches"]) - (15 * 400 + 6 * 300) / 21) < 0.1
    assert float(out["void knn_kernel<4>"]["AvgNs"]) == 60.0 and "unrelated_kernel" not in out


def test_committed_isa_counts_belong_to_the_committed_kernel_sources():
    """bench.py's issue roof reads profiles/r*_isa_counts.json and refuses a file made from other sources (its `source_stamp` is
    the hash of thermompnn_amd/csrc): regenerate it with `python tools/isa_counts.py` whenever a kernel source changes."""
    import bench
    c = bench.isa_counts("enc_edge")
    assert c is not None, "profiles/r*_isa_counts.json is stale: run python tools/isa_counts.py"
    assert c["mfma:v_mfma_f32_16x16x32_f16"] == 108 and c["valu"] + c["valu_packed"] + c["valu_trans"] > 300
    ir = bench.issue_roof("enc_edge", 16384, 256, 2.3, 0.30)
    assert ir["tiles_per_cu"] == 64 and 0.2 < ir["frac_overlap"] < ir["frac_hetero"] < ir["frac_serial"] < 1.0
    assert abs(ir["t_serial_us"] - (ir["t_valu_us"] + ir["t_mfma_us"])) < 1e-9 and ir["t_overlap_us"] == max(ir["t_valu_us"], ir["t_mfma_us"])
    assert 2.5 <= ir["mean_valu_cost_cycles"] <= 6.6        # priced per opcode (tools/probe/valu_cost_probe.hip)
    assert ir["wavefront_trips_per_tile"] == 8
    # the message kernels of the bench batch: one wavefront per residue, three 16-row blocks = three trips of the counted loop, every
    # trip the whole chain for 16 rows x 128 columns (2 GEMMs x 32 units x 3 partial products)
    for k in ("enc_msg", "dec_msg"):
        cm = bench.isa_counts(k)
        assert cm is not None and "msg8_wave_kernel" in cm["symbol"] and cm["mfma:v_mfma_f32_16x16x32_f16"] == 192 and cm.get("barrier", 0) == 0
        im = bench.issue_roof(k, 16384, 256, 2.05, 0.19)
        assert im["wavefront_trips_per_tile"] == 3 and abs(im["cycles_per_simd_tile"]["mfma"] - 0.75 * 192 * 16) < 1e-6
        assert 0.2 < im["frac_overlap"] < im["frac_serial"] < 1.0


def test_no_shipped_per_edge_or_node_kernel_spills_to_scratch():
    """Round 6: a per-edge kernel that spills even 20 bytes reloads them inside its tile loop, and a scratch reload's vmcnt wait drains every
    prefetch in flight (the fused edge + message kernel did, for one build). The ISA record of the committed sources (tools/isa_counts.py,
    made without a GPU) must show no scratch for the f16x2 / bf16x3 per-edge, node, head and featurizer kernels."""
    import glob
    import json
    import bench
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_isa_counts.json")), reverse=True)
    d = next(x for x in (json.load(open(f)) for f in files) if x.get("source_stamp") == bench.kernel_source_stamp())
    hot = ("enc_edge8_rp_kernel", "msg8_wave_kernel", "msg8_rp_kernel", "edge_msg_fused_kernel", "node_update8_split_kernel", "node_update8_deep_kernel",
           "head8_split_kernel", "featurize_split_kernel")
    seen = set()
    for name, e in d["kernels"].items():
        for h in hot:
            if h in name:
                seen.add(h)
                assert int(e.get("scratch_bytes") or 0) == 0, f"{name} spills {e['scratch_bytes']} bytes of scratch"
    assert seen == set(hot), sorted(set(hot) - seen)


def test_tracked_round_evidence_is_not_empty_and_belongs_to_these_kernels():
    """`profiles/r04_parity_worst_errors.json` was committed as `{}` while DESIGN quoted it. Every tracked JSON of the
    newest round under profiles/ must hold something, the parity record must be the GPU suite's (>= 150 entries), and the files that
    are stamped with the kernel-source hash (ISA counts, PMC traffic) must have been made from the sources in this tree."""
    import glob
    import json
    import re
    import bench
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_*.json")))
    newest = max(re.match(r"r(\d+)_", os.path.basename(f)).group(1) for f in files)
    mine = [f for f in files if os.path.basename(f).startswith(f"r{newest}_")]
    assert len(mine) >= 8, mine
    for f in mine:
        d = json.load(open(f))
        assert d, f"{f} is empty"
    worst = json.load(open(os.path.join(REPO, "profiles", f"r{newest}_parity_worst_errors.json")))
    assert len(worst) >= 150 and all("ratio" in v for v in worst.values()) and max(v["ratio"] for v in worst.values()) <= 1.0
    stamp = bench.kernel_source_stamp()
    assert json.load(open(os.path.join(REPO, "profiles", f"r{newest}_isa_counts.json")))["source_stamp"] == stamp
    assert json.load(open(os.path.join(REPO, "profiles", f"r{newest}_pmc_traffic.json")))["kernel_source_stamp"] == stamp, \
        "profiles/*_pmc_traffic.json was measured on other kernel sources: rerun tools/pmc_traffic.sh (tools/measure_round.sh)"
    line = json.load(open(os.path.join(REPO, "profiles", f"r{newest}_bench_full.json")))
    assert line["roofline"]["traffic"] and line["roofline"]["issue"]["frac_overlap"] < line["roofline"]["issue"]["frac_serial"] < 1.0


def test_dump_outputs_writes_float32_and_keeps_a_fixed_sample_under_the_cap(tmp_path):
    """--dump-outputs: arrays within the cap are written whole as float32; above it every array keeps the same seeded rows, so two
    runs with the same arguments write the same files, and the files hold at most the cap in all."""
    import numpy as np
    import bench
    table = np.arange(1000 * 21, dtype=np.float64).reshape(1000, 21)
    listed = np.linspace(-1.0, 1.0, 3000)
    bench.dump_outputs(str(tmp_path / "whole"), {"ddg": table})
    got = np.load(tmp_path / "whole" / "ddg.npy")
    assert got.dtype == np.float32 and np.array_equal(got, table.astype(np.float32))
    cap = 40000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"ddg": table, "ddg_listed": listed}, cap_bytes=cap)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("ddg", "ddg_listed")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("ddg", "ddg_listed")}
    assert all(np.array_equal(a[n], b[n]) for n in a) and sum(x.nbytes for x in a.values()) <= cap
    assert a["ddg"].shape[1] == 21 and 0 < a["ddg"].shape[0] < 1000 and 0 < a["ddg_listed"].shape[0] < 3000
    rows = a["ddg"][:, 0].astype(np.int64) // 21                      # every kept row is a whole row of the table, in order
    assert np.array_equal(a["ddg"], table[rows].astype(np.float32)) and np.all(np.diff(rows) > 0)
