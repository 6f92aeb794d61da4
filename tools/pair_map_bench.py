"""What the per-site-pair map of the double mutants costs: one run on one box, the legs alternated in one process, medians of --rounds
rounds (default 5) with the rounds' min and max. One synthetic protein of L = 256, every single-substitution background (256 x 19 =
4 864, cysteine included), chunks of 256 variants, f16x2. Wall clock around each leg with the device drained, and
torch.cuda.max_memory_allocated of the leg.

 (a) decodes:  one encode, the wild type and the 19 chunks decoded and dropped: what any route pays.
 (b) map:      variant_scan.double_mutant_map: the same decodes, every chunk reduced into the [256, 256] state on the device, the
               state decoded and copied to the host.
 (c) table:    variant_scan.double_mutant_table ([256, 20, 256, 20], one encode per chunk) and the same reductions in torch: the
               wild-type letters of both sites and the first site masked by hand, amin / argmin over the two letter axes for the best
               double mutant, the fp32 epistasis table - (wt[p, a] + wt[q, b]) with amin / argmin, amax / argmax and the mean of its
               absolute value, the eight [256, 256] results copied to the host.
 share:        device events around tmpnn_pair_map's two launches on one chunk of tables (buffers made once) and around the decode of
               that chunk: map / (decode + map).
 agreement:    the two routes' best double mutants have the same bits and letters (the epistasis of (c) is another formula: it takes
               the table's rounded sum apart again, so only (b)'s is the difference of the two tables' own entries).

    python tools/pair_map_bench.py [--rounds 5] [--out profiles/pair_map_bench.json]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from thermompnn_amd import _lib, variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.engine import _ptr, _stream
    from thermompnn_amd.synthetic import synthetic_backbone
    L, chunk = 256, 256
    model = load_model(None, None, 0, precision="f16x2")
    eng = model.engine()
    X, seq = synthetic_backbone(L, 1)
    coords = {f"{n}_chain_A": X[:, i].astype(np.float64).tolist() for i, n in enumerate(("N", "CA", "C", "O"))}
    pdb = [{"resn_list": [str(i + 1) for i in range(L)], "seq_chain_A": seq, "coords_chain_A": coords, "name": "syn_L256", "num_of_chains": 1,
            "seq": seq}]
    wt_idx = variant_scan.sequence_indices(seq)
    pairs = [(p, b) for p in range(L) for b in range(20) if b != wt_idx[p]]
    p_of, a_of = (np.array(x) for x in zip(*pairs))
    S_all = np.tile(wt_idx, (len(pairs), 1))
    S_all[np.arange(len(pairs)), p_of] = a_of
    out = {"metric": "double_mutant_map", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "workload": f"L = {L}, {len(pairs)} single-substitution backgrounds (cysteine included), chunks of {chunk}: "
                       f"{len(pairs) * (L - 1) * 19} double mutants reduced to {L * (L - 1)} site pairs",
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}

    def decodes():
        enc = model._encode_structure(pdb[0])
        model._tables_over(enc, wt_idx[None])
        for v0 in range(0, len(pairs), chunk):
            model._tables_over(enc, S_all[v0:v0 + chunk])

    def pair_map():
        return variant_scan.double_mutant_map(model, pdb, include_cys=True, chunk=chunk)

    own = torch.zeros((L, 20), dtype=torch.bool, device="cuda:0")            # [q, b]: b is the wild type's letter at q
    own[torch.arange(L), torch.as_tensor(wt_idx)] = True
    bad = own[:, :, None, None] | own[None, None, :, :] | torch.eye(L, dtype=torch.bool, device="cuda:0")[:, None, :, None]
    flat = lambda x: x.permute(0, 2, 1, 3).reshape(L, L, 400)                # [p, q, (a, b)]

    def table_torch():
        dm = variant_scan.double_mutant_table(model, pdb, chunk=chunk)      # [L, 20, L, 20]
        wt = model.variant_tables(pdb, wt_idx[None])[0][:, :20]
        eps = dm - (wt[:, :, None, None] + wt[None, None, :, :])            # fp32
        inf = float("inf")
        lo, hi = flat(eps.masked_fill(bad, inf)), flat(eps.masked_fill(bad, -inf))
        best = flat(dm.masked_fill_(bad, inf))
        n = (~bad).sum(dim=(1, 3))
        res = (best.amin(2), best.argmin(2), lo.amin(2), lo.argmin(2), hi.amax(2), hi.argmax(2),
               flat(eps.abs_().masked_fill_(bad, 0.0)).sum(2) / n.clamp(min=1), n)
        return [r.cpu() for r in res]

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

    legs = {"decodes": decodes, "map": pair_map, "table_torch": table_torch}
    res = alternated(legs, a.rounds, wall)
    for name, fn in legs.items():
        res[name]["max_memory_allocated_bytes"] = max(peaks[id(fn)])
    out["legs"] = dict(unit="wall ms per call, device drained before and after", **res)
    out["legs"]["map_over_decodes"] = round(res["map"]["median"] / res["decodes"]["median"], 4)
    out["legs"]["map_over_table_torch"] = round(res["map"]["median"] / res["table_torch"]["median"], 4)
    out["legs"]["memory_map_over_table_torch"] = round(res["map"]["max_memory_allocated_bytes"] / res["table_torch"]["max_memory_allocated_bytes"], 4)
    # the two routes agree on every pair's best double mutant (first minimum in (a, b) order)
    with torch.no_grad():
        m = pair_map()
        t = table_torch()
    live = m.count > 0
    first = (flat(variant_scan.double_mutant_table(model, pdb, chunk=chunk).masked_fill_(bad, float("inf"))) == t[0].cuda()[:, :, None]).int().argmax(2).cpu().numpy()
    out["same_best_bits"] = bool(np.array_equal((m.best_ddG[live] + np.float32(0)).view(np.uint32), (t[0].numpy()[live] + np.float32(0)).view(np.uint32)))
    out["same_best_letters"] = bool(np.array_equal(m.best_a[live] * 20 + m.best_b[live], first[live]))
    out["same_counts"] = bool(np.array_equal(m.count, t[7].numpy()))
    out["site_pairs"] = int(live.sum())

    # the reduction's share of a chunk: events around the two launches, buffers made once
    with torch.no_grad():
        enc = model._encode_structure(pdb[0])
        wt = model._tables_over(enc, wt_idx[None])[0]
        tab = model._tables_over(enc, S_all[:chunk])
    S_dev = torch.as_tensor(S_all[:chunk]).to("cuda:0", torch.int32)
    base = wt[torch.as_tensor(p_of[:chunk], device="cuda:0"), torch.as_tensor(a_of[:chunk], device="cuda:0")].contiguous()
    row, letter = (torch.as_tensor(x[:chunk]).to("cuda:0", torch.int32) for x in (p_of, a_of))
    state = [torch.empty((L, L), dtype=getattr(torch, dt), device="cuda:0") for _, dt in _lib.PMAP_STATE]
    ws = torch.empty(eng.lib.tmpnn_pair_map_workspace_bytes(chunk, L), dtype=torch.uint8, device="cuda:0")

    def raw(flags):
        def run():
            rc = eng.lib.tmpnn_pair_map(_ptr(tab), 21, _ptr(S_dev), _ptr(base), _ptr(row), _ptr(letter), _ptr(row), _ptr(wt), 21, chunk, L, L,
                                        flags, *[_ptr(x) for x in state], _ptr(ws), ws.numel(), _stream())
            assert rc == 0, rc
        return run

    share_legs = {"decode_chunk": lambda: model._tables_over(enc, S_dev), "map_launches_only_first_chunk": raw(1), "map_launches_only_continue": raw(5)}
    with torch.no_grad():
        rs = alternated(share_legs, a.rounds, lambda fn, warm: ms_per_call(fn, 3 if warm else 20))
    out["chunk"] = dict(workload=f"one chunk: {chunk} variants x L = {L} ({chunk * L * 21 * 4} bytes of tables, {ws.numel()} of workspace)",
                        unit="ms per call (device events, 20 calls)", **rs)
    s, d = rs["map_launches_only_continue"]["median"], rs["decode_chunk"]["median"]
    out["chunk"]["map_share"] = round(s / (s + d), 4)
    out["chunk"]["table_bytes_per_s_continue"] = round(chunk * L * 21 * 4 / s * 1e3)
    out["not_measured"] = ["L other than 256", "R L near 2^31 (a state of 2^31 entries is 69 GB)", "real checkpoints (synthetic weights)",
                           "multi-GPU (single rank)", "chunks other than 256"]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
