"""What the beam search costs for MANY proteins: one packed search against the per-protein loop. One run on one box, the legs alternated
in one process, medians of --rounds rounds (default 5) with the rounds' min and max. P = 64 synthetic backbones of L = 256, order 4,
beam 64, f16x2; the encodes are INSIDE both legs. Wall clock around each leg with the device drained, and
torch.cuda.max_memory_allocated of the leg.

 (a) each:   ONE variant_scan.multi_mutant_search_each over the 64 structures: one encode of the pack, four decodes of (1, 64, 64, 64)
             rows over 16 384 packed residues, four Engine.beam_step_each.
 (b) loop:   64 calls of variant_scan.multi_mutant_search: the capability of the commit before.
 agreement:  whether the two legs' sets, parents and score bits are equal, structure by structure.
 step:       device events around tmpnn_beam_step_each's three launches on each round's packed tables (buffers made once) against 64
             tmpnn_beam_step calls on the proteins' slices of the same tables (copied out once, outside the timing).

 headline:   with --headline FILE: the JSON lines of `python bench.py --gpus 1 --steps 50 --warmup 20` in this tree and in a checkout of
             the parent commit, three runs each per pass ({"tree": "this" | "parent", "pass": ..., ...bench.py's line} per line; a pass
             names which tree ran first in every pair): preds/s per run and the range per tree and pass.

    python tools/multi_mutant_each_bench.py [--rounds 5] [--headline FILE] [--out profiles/multi_mutant_each_bench.json]
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
    ap.add_argument("--proteins", type=int, default=64)
    ap.add_argument("--headline", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from thermompnn_amd import variant_scan
    from thermompnn_amd.custom_inference import load_model
    from thermompnn_amd.engine import _ptr, _stream
    from thermompnn_amd.synthetic import synthetic_backbone
    P, L, order, beam = a.proteins, 256, 4, 64
    model = load_model(None, None, 0, precision="f16x2")
    eng = model.engine()
    pdbs = []
    for p in range(P):
        X, seq = synthetic_backbone(L, 1 + p)
        coords = {f"{n}_chain_A": X[:, i].astype(np.float64).tolist() for i, n in enumerate(("N", "CA", "C", "O"))}
        pdbs.append([{"resn_list": [str(i + 1) for i in range(L)], "seq_chain_A": seq, "coords_chain_A": coords, "name": f"syn{p}_L{L}",
                      "num_of_chains": 1, "seq": seq}])
    out = {"metric": "multi_mutant_search_each", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "precision": eng.precision,
           "workload": f"P = {P} synthetic backbones of L = {L}, order {order}, beam {beam}; encodes inside both legs",
           "unit": "median over rounds, with the rounds' min and max; legs alternated inside every round, one process"}
    each = lambda: variant_scan.multi_mutant_search_each(model, pdbs, order, beam, pack_residues=P * L)
    loop = lambda: [variant_scan.multi_mutant_search(model, pdb, order, beam) for pdb in pdbs]
    flat = lambda res: [[[(h.mutations, int(np.float32(h.ddG).view(np.uint32)), h.parent) for h in lv] for lv in levels] for levels in res]
    with torch.no_grad():
        packed, single = each(), loop()
    a_flat, b_flat = flat(packed), flat(single)
    out["same_sets_parents_score_bits"] = bool(a_flat == b_flat)
    out["structures_that_differ"] = [p for p in range(P) if a_flat[p] != b_flat[p]]
    out["mutants_per_level_first_structure"] = [len(lv) for lv in packed[0]]
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

    legs = {"each": each, "loop": loop}
    res = alternated(legs, a.rounds, wall)
    for name, fn in legs.items():
        res[name]["max_memory_allocated_bytes"] = max(peaks[id(fn)])
    out["legs"] = dict(unit="wall ms per call (all structures), device drained before and after", **res)
    out["legs"]["loop_over_each"] = round(res["loop"]["median"] / res["each"]["median"], 4)
    out["legs"]["each_ms_per_structure"] = round(res["each"]["median"] / P, 5)
    out["legs"]["loop_ms_per_structure"] = round(res["loop"]["median"] / P, 5)

    # the step alone: the packed entry's three launches against P single steps on the same tables
    recorded = []

    def recording_step(ddg, S_var, score, muts, offsets, depth, k, **kw):
        r = eng.beam_step_each(ddg, S_var, score, muts, offsets, depth, k, **kw)
        recorded.append((torch.as_tensor(S_var).to("cuda:0", torch.int32).clone(), None if muts is None else muts.clone(),
                         torch.as_tensor(score).to("cuda:0", torch.float32).clone(), depth))
        return r

    with torch.no_grad():
        enc = model._encode_structures([p[0] for p in pdbs])
        tables = lambda s, _o=None: model._tables_over(enc, s)
        variant_scan.multi_mutant_search_each(model, pdbs, order, beam, pack_residues=P * L, _tables=tables, _step=recording_step)
    T = P * L
    offsets = torch.arange(0, T + 1, L, dtype=torch.int32, device="cuda:0")
    step_legs, shapes = {}, []
    for S, muts, score, depth in recorded:
        V = int(S.shape[0])
        with torch.no_grad():
            t = tables(S)
        ld = int(t.stride(1))
        bufs = [torch.empty((P, beam, depth), dtype=torch.int32, device="cuda:0"), torch.empty((P, beam), dtype=torch.float32, device="cuda:0"),
                torch.empty((P, beam), dtype=torch.int32, device="cuda:0"), torch.empty((beam, T), dtype=torch.int32, device="cuda:0"),
                torch.empty(P, dtype=torch.int32, device="cuda:0")]
        ws = torch.empty(eng.lib.tmpnn_beam_step_each_workspace_bytes(P, V, L, beam, depth), dtype=torch.uint8, device="cuda:0")

        def step_each(t=t, S=S, muts=muts, score=score, depth=depth, V=V, bufs=bufs, ws=ws, ld=ld):
            rc = eng.lib.tmpnn_beam_step_each(_ptr(t), ld, _ptr(S), _ptr(score), _ptr(muts), depth, None, _ptr(offsets), P, T, V, L, beam,
                                              float("inf"), 0, *[_ptr(x) for x in bufs], _ptr(ws), ws.numel(), _stream())
            assert rc == 0, rc
        own = [(t[:, p * L:(p + 1) * L].contiguous(), S[:, p * L:(p + 1) * L].contiguous(), score[p].contiguous(),
                None if muts is None else muts[p].contiguous()) for p in range(P)]
        one = [torch.empty((beam, depth), dtype=torch.int32, device="cuda:0"), torch.empty(beam, dtype=torch.float32, device="cuda:0"),
               torch.empty(beam, dtype=torch.int32, device="cuda:0"), torch.empty((beam, L), dtype=torch.int32, device="cuda:0"),
               torch.empty(1, dtype=torch.int32, device="cuda:0")]
        ws1 = torch.empty(eng.lib.tmpnn_beam_step_workspace_bytes(V, L, beam, depth), dtype=torch.uint8, device="cuda:0")

        def step_loop(own=own, depth=depth, V=V, one=one, ws1=ws1):
            for t_p, S_p, score_p, muts_p in own:
                rc = eng.lib.tmpnn_beam_step(_ptr(t_p), int(t_p.stride(1)), _ptr(S_p), _ptr(score_p), _ptr(muts_p), depth, None, V, L, beam,
                                             float("inf"), 0, *[_ptr(x) for x in one], _ptr(ws1), ws1.numel(), _stream())
                assert rc == 0, rc
        step_legs[f"step_each_round{depth}"] = step_each
        step_legs[f"step_loop_round{depth}"] = step_loop
        W = min(V, 8192 // max(2, 1 << (beam * depth - 1).bit_length()) - 1)
        shapes.append(dict(round=depth, members=V, stage1_workgroups_each=P * W, stage1_workgroups_single=W))
        del t
    with torch.no_grad():
        rs = alternated(step_legs, a.rounds, lambda fn, warm: ms_per_call(fn, 2 if warm else 10))
    out["step_launches_only"] = dict(unit=f"ms per call for all {P} proteins (device events, 10 calls)", shapes=shapes, **rs)
    e_all = sum(rs[f"step_each_round{d}"]["median"] for _, _, _, d in recorded)
    l_all = sum(rs[f"step_loop_round{d}"]["median"] for _, _, _, d in recorded)
    for _, _, _, d in recorded:
        out["step_launches_only"][f"loop_over_each_round{d}"] = round(rs[f"step_loop_round{d}"]["median"] / rs[f"step_each_round{d}"]["median"], 4)
    out["step_launches_only"]["loop_over_each_all_rounds"] = round(l_all / e_all, 4)
    if a.headline:
        runs = [json.loads(ln) for ln in open(a.headline) if ln.strip().startswith("{")]
        runs = [{"tree": r["tree"], "pass": r.get("pass", ""), "preds_per_s": round(r["value"]), "ms_per_step": round(r["ms_per_step"], 4)} for r in runs]
        passes = sorted({r["pass"] for r in runs})
        out["headline_bench_py"] = dict(what="python bench.py --gpus 1 --steps 50 --warmup 20 in this tree and in a checkout of the parent commit, in "
                                             "pairs, three pairs per pass, one process per run, one box; a pass names the tree that ran first in "
                                             "every pair", runs=runs,
                                        preds_per_s_range={ps: {t: [min(r["preds_per_s"] for r in runs if r["tree"] == t and r["pass"] == ps),
                                                                    max(r["preds_per_s"] for r in runs if r["tree"] == t and r["pass"] == ps)]
                                                                for t in ("parent", "this")} for ps in passes})
    out["not_measured"] = ["multi-GPU (single rank)", "L other than 256, P other than 64, ragged packs", "other beam / order shapes",
                           "real structure files (parsing is outside both legs)"] + ([] if a.headline else ["bench.py against the parent commit"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
