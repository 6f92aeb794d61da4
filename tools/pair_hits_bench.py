"""What the double-mutant hit list costs: one run on one box, the legs alternated in one process, medians of --rounds rounds (default
5) with the rounds' min and max. One synthetic protein of L = 256, every single-substitution background (256 x 19 = 4 864, cysteine
included), chunks of 256 variants, f16x2, at k = 32 and k = 256. Wall clock around each leg with the device drained, and
torch.cuda.max_memory_allocated of the leg.

 (a) decodes:  one encode, the wild type and the 19 chunks decoded and dropped: what any route pays.
 (b) hits:     variant_scan.double_mutant_hits: the same decodes, every chunk reduced to k keys on the device.
 (c) table:    variant_scan.double_mutant_table ([256, 20, 256, 20], one encode per chunk), the wild-type letters of both sites and
               the first site masked by hand, torch.topk on the flattened table (values and flat indices, no tie order).
 share:        device events around tmpnn_select_variant_hits' two launches on one chunk of tables (buffers made once) and around
               the decode of that chunk: selection / (decode + selection). At k = 256 only 31 stage-1 workgroups run.
 headline:     with --parent-lib PATH (a libtmpnn.so built from the parent commit) the fused forward of bench.py's batch through
               both libraries, alternated (tools/hits_bench.py's LibForward): the forward must not move beyond the rounds' spread.

    python tools/pair_hits_bench.py [--rounds 5] [--parent-lib PATH] [--out profiles/pair_hits_bench.json]
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
from hits_bench import LibForward, alternated, ms_per_call  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import bench
    from thermompnn_amd import variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.engine import _ptr, _stream
    from thermompnn_amd.synthetic import AA20, synthetic_backbone
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
    out = {"metric": "double_mutant_hits", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "workload": f"L = {L}, {len(pairs)} single-substitution backgrounds (cysteine included), chunks of {chunk}: "
                       f"{len(pairs) * (L - 1) * 19} double mutants",
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}

    def decodes():
        enc = model._encode_structure(pdb[0])
        model._tables_over(enc, wt_idx[None])
        for v0 in range(0, len(pairs), chunk):
            model._tables_over(enc, S_all[v0:v0 + chunk])

    own = torch.zeros((L, 20), dtype=torch.bool, device="cuda:0")            # [q, b]: b is the wild type's letter at q
    own[torch.arange(L), torch.as_tensor(wt_idx)] = True

    def table_topk(k):
        def run():
            dm = variant_scan.double_mutant_table(model, pdb, chunk=chunk)  # [L, 20, L, 20]
            bad = own[:, :, None, None] | own[None, None, :, :] | torch.eye(L, dtype=torch.bool, device="cuda:0")[:, None, :, None] | torch.isnan(dm)
            return torch.topk(dm.masked_fill_(bad, float("inf")).reshape(-1), k, largest=False)
        return run

    peaks = {}

    def wall(name):
        def measure(fn, warm):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            with torch.no_grad():
                fn()
            torch.cuda.synchronize()
            peaks.setdefault(id(fn), []).append(torch.cuda.max_memory_allocated())
            return (time.perf_counter() - t0) * 1e3
        return measure

    legs = {"decodes": decodes}
    for k in (32, 256):
        legs[f"hits_k{k}"] = (lambda k: lambda: variant_scan.double_mutant_hits(model, pdb, k, include_cys=True, chunk=chunk))(k)
        legs[f"table_topk_k{k}"] = table_topk(k)
    res = alternated(legs, a.rounds, wall(None))
    for name, fn in legs.items():
        res[name]["max_memory_allocated_bytes"] = max(peaks[id(fn)])
    out["legs"] = dict(unit="wall ms per call, device drained before and after", **res)
    for k in (32, 256):
        out["legs"][f"hits_over_decodes_k{k}"] = round(res[f"hits_k{k}"]["median"] / res["decodes"]["median"], 4)
        out["legs"][f"hits_over_table_k{k}"] = round(res[f"hits_k{k}"]["median"] / res[f"table_topk_k{k}"]["median"], 4)
    # the two routes agree on the values (the table route has no tie order)
    with torch.no_grad():
        hits = variant_scan.double_mutant_hits(model, pdb, 256, include_cys=True, chunk=chunk)
        vals = table_topk(256)().values.cpu().numpy()
    out["same_values_k256"] = bool(np.array_equal(np.array([h.ddG for h in hits], np.float32), vals))

    # the selection's share of a chunk: events around the two launches, buffers made once
    with torch.no_grad():
        enc = model._encode_structure(pdb[0])
        wt = model._tables_over(enc, wt_idx[None])[0]
        t = model._tables_over(enc, S_all[:chunk])
    S_dev = torch.as_tensor(S_all[:chunk]).to("cuda:0", torch.int32)
    base = wt[torch.as_tensor(p_of[:chunk], device="cuda:0"), torch.as_tensor(a_of[:chunk], device="cuda:0")].contiguous()
    tag = torch.as_tensor(p_of[:chunk] * 32 + a_of[:chunk]).to("cuda:0", torch.int32)
    skip = torch.as_tensor(p_of[:chunk]).to("cuda:0", torch.int32)
    share_legs = {"decode_chunk": lambda: model._tables_over(enc, S_dev)}
    for k in (32, 256):
        bufs = [torch.empty(k, dtype=dt, device="cuda:0") for dt in (torch.int64, torch.float32, torch.int32, torch.int32, torch.int32)] + \
               [torch.empty(1, dtype=torch.int32, device="cuda:0")]
        ws = torch.empty(eng.lib.tmpnn_variant_hits_workspace_bytes(chunk, L, k), dtype=torch.uint8, device="cuda:0")

        def sel_raw(k=k, bufs=bufs, ws=ws):
            rc = eng.lib.tmpnn_select_variant_hits(_ptr(t), 21, _ptr(S_dev), _ptr(base), _ptr(tag), _ptr(skip), chunk, L, k, float("inf"), 1,
                                                   *[_ptr(x) for x in bufs], _ptr(ws), ws.numel(), _stream())
            assert rc == 0, rc
        share_legs[f"select_k{k}_launches_only"] = sel_raw
    with torch.no_grad():
        rs = alternated(share_legs, a.rounds, lambda fn, warm: ms_per_call(fn, 3 if warm else 20))
    out["chunk"] = dict(workload=f"one chunk: {chunk} variants x L = {L}", unit="ms per call (device events, 20 calls)", **rs)
    for k in (32, 256):
        s, d = rs[f"select_k{k}_launches_only"]["median"], rs["decode_chunk"]["median"]
        out["chunk"][f"selection_share_k{k}"] = round(s / (s + d), 4)
        out["chunk"][f"stage1_workgroups_k{k}"] = min(chunk, 8192 // k - 1)

    if a.parent_lib:
        from thermompnn_amd import _lib
        P = 64
        b = bench.build_batch(P, L, 0, "cuda:0")
        this_out = torch.empty((b["T"], 21), dtype=torch.float32, device="cuda:0")
        parent_out = torch.empty_like(this_out)
        from thermompnn_amd.engine import Engine
        from thermompnn_amd.weights import synthetic_state_dict
        e2 = Engine(synthetic_state_dict(0), "cuda:0", 48)
        this, parent = LibForward(_lib.LIB_PATH, e2, b, this_out), LibForward(a.parent_lib, e2, b, parent_out)
        rh = alternated({"headline_this_library": this, "headline_parent_library": parent}, a.rounds,
                        lambda fn, warm: ms_per_call(fn, 3 if warm else 30))
        this()
        parent()
        torch.cuda.synchronize()
        t_ms, p_ms = rh["headline_this_library"]["median"], rh["headline_parent_library"]["median"]
        out["headline"] = dict(workload=f"{P} proteins x L = {L}, the fused forward", unit="ms per call (device events, 30 calls)", **rh,
                               this_over_parent=round(t_ms / p_ms, 4),
                               same_bits=bool(torch.equal(this_out.view(torch.int32), parent_out.view(torch.int32))),
                               preds_per_s_this=round(P * L * 20 / t_ms * 1e3), preds_per_s_parent=round(P * L * 20 / p_ms * 1e3))
    out["not_measured"] = ["L other than 256", "k other than 32 and 256", "a two-level merge of stage 1", "multi-GPU (single rank)"] + \
        ([] if a.parent_lib else ["the headline against the parent library"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
