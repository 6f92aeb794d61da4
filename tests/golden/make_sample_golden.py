"""Generate the autoregressive-sampling fixtures by IMPORTING THE REFERENCE (runs only in the build container, on the CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sample_golden.py

Runs the reference's ProteinMPNN.sample (seed-0 Xavier weights installed through the reference's own loading path,
make_golden.build_reference_model) on N copies of a fixture's structure, with torch.multinomial replaced FOR THE DURATION OF THE CALL
by the project's draw rule on recorded uniforms:

    c_a = fp32 running sum of probs in index order; the pick is the smallest a with c_a > u * c_20 (none: the largest a with
    probs_a > 0); u is indexed by (member, RESIDUE).

A uniform whose u * c_20 lies within MARGIN = 1e-3 (100 x the project's 1e-5 line) of any cumulative boundary (0 and every c_a) is
redrawn from the seeded generator, so every stored draw has min_margin >= 1e-3 and no step is left out. The reference makes no
draw at a step where every member's residue is masked; the step -> residue bookkeeping below follows its decoding_order (recorded
from its own torch.argsort call). Stores only tensors in sample_<case>.npz: randn, chain_mask, chain_M_pos, free, u, temperature,
omit_AAs, bias_AAs, bias_by_res, omit_AA_mask (where used), S_true, S, probs, decoding_order, min_margin, n_redraws, and for the
masked layout the reference's E_idx (as the ordered fixtures store it).

    case         N  temperature  extras
    syn_L32      3  1.0          nothing else (K_eff 31 < 48)
    2OCJ_A_gap   2  0.5          letter 20 omitted, non-zero bias_AAs, bias_by_res and omit_AA_mask on a few positions, every fifth
                                 position fixed
    msk_L40      2  1.0          the reference's E_idx stored
"""
import os
import sys
import tempfile

import numpy as np
import torch

import make_golden as mg          # the same directory: imports the reference

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
from masked_backbones import layout_arrays          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-3
CASES = {"syn_L32": (3, 1.0), "2OCJ_A_gap": (2, 0.5), "msk_L40": (2, 1.0)}


def inputs_of(case):
    if case.startswith("msk_"):
        X, S, mask, ridx, cenc = layout_arrays(case)
        return dict(X=X, S=S, mask=mask, residue_idx=ridx, chain_enc=cenc)
    with np.load(os.path.join(HERE, case + ".npz")) as z:
        return {k: z[k] for k in z.files}


def cumulative(p):
    """fp32 running sum in index order."""
    c, run = np.zeros(len(p), np.float32), np.float32(0.0)
    for a in range(len(p)):
        run = np.float32(run + np.float32(p[a]))
        c[a] = run
    return c


def draw(p, u):
    """-> (pick, margin) of the draw rule for probabilities p [21] (fp32) and one uniform."""
    c = cumulative(p)
    thr = np.float32(np.float32(u) * c[-1])
    above = np.nonzero(c > thr)[0]
    pick = int(above[0]) if len(above) else int(np.nonzero(np.asarray(p) > 0)[0][-1])
    margin = float(np.abs(np.concatenate([[0.0], c.astype(np.float64)]) - float(thr)).min())
    return pick, margin


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mp = mg.build_reference_model(tmp).prot_mpnn
    for n, (case, (N, temperature)) in enumerate(CASES.items()):
        g = inputs_of(case)
        t = torch.from_numpy
        L = len(g["S"])
        rep = lambda a: a[None].repeat(N, *([1] * a.dim()))
        X, mask = rep(t(g["X"])), rep(t(g["mask"]))
        S_true = rep(t(g["S"].astype(np.int64)))
        ridx, cenc = rep(t(g["residue_idx"].astype(np.int64))), rep(t(g["chain_enc"].astype(np.int64)))
        gen = torch.Generator().manual_seed(500 + n)
        randn = torch.randn(N, L, generator=gen)
        u = torch.rand(N, L, generator=gen).numpy()
        chain_mask, chain_M_pos = torch.ones(N, L), torch.ones(N, L)
        omit, bias_aa = np.zeros(21, np.float32), np.zeros(21, np.float32)
        by_res, omit_mask = torch.zeros(N, L, 21), None
        if case == "2OCJ_A_gap":
            omit[20] = 1.0
            bias_aa = (0.5 * torch.randn(21, generator=gen)).numpy().astype(np.float32)
            for pos in (3, 50, 51, 120, 190):
                by_res[:, pos] = 1.5 * torch.randn(21, generator=gen)
            omit_mask = torch.zeros(N, L, 21)
            for pos in (7, 50, 88, 151):
                omit_mask[:, pos, torch.randperm(20, generator=gen)[:6]] = 1.0
            chain_M_pos[:, ::5] = 0.0
        state = dict(order=None, steps=None, calls=0, redraws=0, min_margin=np.inf)
        real_argsort, real_multinomial = torch.argsort, torch.multinomial

        def recording_argsort(*a, **k):
            out = real_argsort(*a, **k)
            if state["order"] is None:
                state["order"] = out.clone().numpy()
                m = g["mask"][state["order"]]                   # [N, steps]: the mask of each member's residue at each step
                state["steps"] = [s for s in range(L) if not (m[:, s] == 0).all()]
            return out

        def rule_multinomial(probs, num_samples, *a, **k):
            assert num_samples == 1 and probs.shape == (N, 21)
            step = state["steps"][state["calls"]]
            state["calls"] += 1
            picks = []
            for b in range(N):
                res = int(state["order"][b, step])
                p = probs[b].numpy().astype(np.float32)
                pick, margin = draw(p, u[b, res])
                while margin < MARGIN:
                    u[b, res] = float(torch.rand(1, generator=gen))
                    state["redraws"] += 1
                    pick, margin = draw(p, u[b, res])
                state["min_margin"] = min(state["min_margin"], margin)
                picks.append(pick)
            return torch.tensor(picks, dtype=torch.int64)[:, None]

        graph = {}
        hook = mp.features.register_forward_hook(lambda m, i, o: graph.update(E_idx=o[1][0].numpy().astype(np.int16)))
        with torch.no_grad():
            torch.argsort, torch.multinomial = recording_argsort, rule_multinomial
            try:
                out = mp.sample(X, randn, S_true, chain_mask, cenc, ridx, mask=mask, temperature=temperature, omit_AAs_np=omit,
                                bias_AAs_np=bias_aa, chain_M_pos=chain_M_pos, omit_AA_mask=omit_mask, bias_by_res=by_res)
            finally:
                torch.argsort, torch.multinomial = real_argsort, real_multinomial
        hook.remove()
        assert state["calls"] == len(state["steps"]) and state["min_margin"] >= MARGIN
        assert np.array_equal(out["decoding_order"].numpy(), state["order"])
        extra = dict(graph) if case.startswith("msk_") else {}
        if omit_mask is not None:
            extra["omit_AA_mask"] = omit_mask.numpy().astype(np.float32)
        path = os.path.join(HERE, f"sample_{case}.npz")
        np.savez_compressed(path, randn=randn.numpy(), chain_mask=chain_mask.numpy(), chain_M_pos=chain_M_pos.numpy(),
                            free=(chain_mask * chain_M_pos).numpy(), u=u.astype(np.float32), temperature=np.float32(temperature),
                            omit_AAs=omit, bias_AAs=bias_aa, bias_by_res=by_res.numpy(), S_true=S_true.numpy().astype(np.int32),
                            S=out["S"].numpy().astype(np.int32), probs=out["probs"].numpy(),
                            decoding_order=out["decoding_order"].numpy().astype(np.int32), min_margin=np.float64(state["min_margin"]),
                            n_redraws=np.int32(state["redraws"]), **extra)
        print(f"sample_{case}: N={N}, L={L}, T={temperature}: {state['calls']} steps, {state['redraws']} redraws, "
              f"min margin {state['min_margin']:.2e} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
