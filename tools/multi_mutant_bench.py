"""What the beam search over n-point mutants costs: one run on one box, the legs alternated in one process, medians of --rounds rounds
(default 5) with the rounds' min and max. One synthetic protein of L = 256, order 4, beam 64, f16x2; ONE encode, outside every timed
region. Wall clock around each leg with the device drained, and torch.cuda.max_memory_allocated of the leg.

 (a) search:      variant_scan.multi_mutant_search: four decodes (1, 64, 64, 64 sequences) and four steps on the device.
 (b) decodes:     the same four decodes alone, on the sequences the search recorded: what any route pays.
 (c) torch_step:  the same search with the step done in torch: the broadcast add, the masks, 64-bit keys, topk(k d), the k d keys
                  copied to the host, deduplicated there, the rows rebuilt on the host and uploaded. Its sets and bits must equal (a).
 share:           device events around tmpnn_beam_step's three launches on each round's tables (buffers made once) and around the
                  decode of that round: steps / (decodes + steps), per round and over the four.

    python tools/multi_mutant_bench.py [--rounds 5] [--out profiles/multi_mutant_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from hits_bench import alternated, ms_per_call  # noqa: E402


def torch_step(ddg, S_var, score, muts, depth, k, allowed=None, cutoff=None, include_cys=False):
    """Engine.beam_step's contract with torch on the device and the dedupe on the host."""
    dev = ddg.device
    S = torch.as_tensor(S_var).to(dev, torch.int64)
    V, L = S.shape
    score = torch.as_tensor(score).to(dev, torch.float32)
    val = score[:, None, None] + ddg[:, :, :20] + 0.0                       # one fp32 add (and -0.0 taken as +0.0)
    q = torch.arange(L, device=dev)[None, :, None]
    b = torch.arange(20, device=dev)[None, None, :]
    ok = ~torch.isnan(val) & (S[:, :, None] >= 0) & (S[:, :, None] < 20) & (b != S[:, :, None])
    if cutoff is not None:
        ok &= val <= cutoff
    if not include_cys:
        ok &= b != 1
    if allowed is not None:
        ok &= (torch.as_tensor(allowed).to(dev) != 0)[None, :, None]
    m = None if muts is None else torch.as_tensor(muts).to(dev, torch.int64)
    if m is not None:
        ok &= (m >= 0).all(1)[:, None, None]
        for c in range(m.shape[1]):
            ok &= q != (m[:, c] >> 5)[:, None, None]
    bits = val.view(torch.int32).to(torch.int64)
    order = torch.where(bits >= 0, bits, bits ^ 0x7fffffff)                 # signed and monotone in the value
    low = (torch.arange(V, device=dev)[:, None, None] << 16) | (q << 5) | b
    key = torch.where(ok, (order << 32) | low, torch.full_like(low, 2 ** 63 - 1)).reshape(-1)
    n = min(k * depth, key.numel())
    top = torch.topk(key, n, largest=False, sorted=True).values.cpu().numpy()
    S_h, m_h = S.cpu().numpy(), None if m is None else m.cpu().numpy()
    out_m, out_s, out_p, out_S, seen = np.full((k, depth), -1, np.int32), np.full(k, np.nan, np.float32), np.full(k, -1, np.int32), \
        np.full((k, L), 20, np.int32), set()
    for x in top.tolist():
        if x == 2 ** 63 - 1 or len(seen) == k:
            break
        v, qq, bb = (x >> 16) & 0xffff, (x >> 5) & 2047, x & 31
        cs = tuple(sorted(([] if m_h is None else m_h[v].tolist()) + [qq << 5 | bb]))
        if cs in seen:
            continue
        r = len(seen)
        seen.add(cs)
        o = x >> 32
        out_m[r], out_p[r] = cs, v
        out_s[r] = np.array([o if o >= 0 else o ^ 0x7fffffff], np.int64).astype(np.int32).view(np.float32)[0]
        out_S[r] = S_h[v]
        out_S[r, qq] = bb
    up = lambda a: torch.from_numpy(a).to(dev)
    return dict(out_muts=up(out_m), out_score=up(out_s), out_parent=up(out_p), out_S=up(out_S), out_count=torch.tensor([len(seen)], dtype=torch.int32))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from thermompnn_amd import variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.engine import _ptr, _stream
    from thermompnn_amd.synthetic import synthetic_backbone
    L, order, beam = 256, 4, 64
    model = load_model(None, None, 0, precision="f16x2")
    eng = model.engine()
    X, seq = synthetic_backbone(L, 1)
    coords = {f"{n}_chain_A": X[:, i].astype(np.float64).tolist() for i, n in enumerate(("N", "CA", "C", "O"))}
    pdb = [{"resn_list": [str(i + 1) for i in range(L)], "seq_chain_A": seq, "coords_chain_A": coords, "name": "syn_L256", "num_of_chains": 1,
            "seq": seq}]
    out = {"metric": "multi_mutant_search", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "workload": f"L = {L}, order {order}, beam {beam}: four decodes (1, {beam}, {beam}, {beam} sequences) and four steps; one encode, not timed",
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}
    with torch.no_grad():
        enc = model._encode_structure(pdb[0])                              # the one encode
    tables = lambda s: model._tables_over(enc, s)
    recorded = []

    def recording_step(ddg, S_var, score, muts, depth, k, **kw):
        recorded.append((torch.as_tensor(S_var).to("cuda:0", torch.int32).clone(), None if muts is None else muts.clone(),
                         torch.as_tensor(score).to("cuda:0", torch.float32).clone(), depth))
        return eng.beam_step(ddg, S_var, score, muts, depth, k, **kw)

    with torch.no_grad():
        found = variant_scan.multi_mutant_search(model, pdb, order, beam, _tables=tables, _step=recording_step)
        by_torch = variant_scan.multi_mutant_search(model, pdb, order, beam, _tables=tables, _step=torch_step)
    same = [[(h.mutations, np.float32(h.ddG).view(np.uint32), h.parent) for h in lv] for lv in found] == \
        [[(h.mutations, np.float32(h.ddG).view(np.uint32), h.parent) for h in lv] for lv in by_torch]
    out["torch_step_same_sets_bits_parents"] = bool(same)
    out["levels"] = [dict(order=d, mutants=len(lv), best_ddG=lv[0].ddG if lv else None, best_epistasis=lv[0].epistasis if lv else None)
                     for d, lv in enumerate(found, 1)]
    peaks = {}

    def wall(fn, warm):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        peaks.setdefault(id(fn), []).append(torch.cuda.max_memory_allocated())
        return (time.perf_counter() - t0) * 1e3

    def decodes():
        for S, _, _, _ in recorded:
            tables(S)

    legs = {"search": lambda: variant_scan.multi_mutant_search(model, pdb, order, beam, _tables=tables),
            "decodes": decodes,
            "torch_step": lambda: variant_scan.multi_mutant_search(model, pdb, order, beam, _tables=tables, _step=torch_step)}
    res = alternated(legs, a.rounds, wall)
    for name, fn in legs.items():
        res[name]["max_memory_allocated_bytes"] = max(peaks[id(fn)])
    out["legs"] = dict(unit="wall ms per call, device drained before and after", **res)
    out["legs"]["search_over_decodes"] = round(res["search"]["median"] / res["decodes"]["median"], 4)
    out["legs"]["search_over_torch_step"] = round(res["search"]["median"] / res["torch_step"]["median"], 4)

    # the step's share of a round: events around the three launches, buffers made once
    share_legs, shapes = {}, []
    for S, muts, score, depth in recorded:
        V = int(S.shape[0])
        with torch.no_grad():
            t = tables(S)
        bufs = [torch.empty((beam, depth), dtype=torch.int32, device="cuda:0"), torch.empty(beam, dtype=torch.float32, device="cuda:0"),
                torch.empty(beam, dtype=torch.int32, device="cuda:0"), torch.empty((beam, L), dtype=torch.int32, device="cuda:0"),
                torch.empty(1, dtype=torch.int32, device="cuda:0")]
        ws = torch.empty(eng.lib.tmpnn_beam_step_workspace_bytes(V, L, beam, depth), dtype=torch.uint8, device="cuda:0")

        def step_raw(t=t, S=S, muts=muts, score=score, depth=depth, V=V, bufs=bufs, ws=ws):
            rc = eng.lib.tmpnn_beam_step(_ptr(t), int(t.stride(1)), _ptr(S), _ptr(score), _ptr(muts), depth, None, V, L, beam, float("inf"), 0,
                                         *[_ptr(x) for x in bufs], _ptr(ws), ws.numel(), _stream())
            assert rc == 0, rc
        share_legs[f"step_round{depth}_launches_only"] = step_raw
        share_legs[f"decode_round{depth}"] = (lambda S=S: tables(S))
        shapes.append(dict(round=depth, members=V, stage1_workgroups=min(V, 8192 // max(2, 1 << (beam * depth - 1).bit_length()) - 1)))
    with torch.no_grad():
        rs = alternated(share_legs, a.rounds, lambda fn, warm: ms_per_call(fn, 3 if warm else 20))
    out["rounds_of_the_search"] = dict(unit="ms per call (device events, 20 calls)", shapes=shapes, **rs)
    s_all = sum(rs[f"step_round{d}_launches_only"]["median"] for d in range(1, order + 1))
    d_all = sum(rs[f"decode_round{d}"]["median"] for d in range(1, order + 1))
    for d in range(1, order + 1):
        s, dec = rs[f"step_round{d}_launches_only"]["median"], rs[f"decode_round{d}"]["median"]
        out["rounds_of_the_search"][f"step_share_round{d}"] = round(s / (s + dec), 4)
    out["rounds_of_the_search"]["step_share_all_rounds"] = round(s_all / (s_all + d_all), 4)
    out["not_measured"] = ["multi-GPU (single rank)", "L other than 256", "other beam / order shapes"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
