"""Generate the tied-sampling and PSSM fixtures by IMPORTING THE REFERENCE (runs only in the build container, on the CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tied_sample_golden.py

Runs the reference's ProteinMPNN.tied_sample / sample (seed-0 Xavier weights through make_golden.build_reference_model) on N copies
of a structure, with torch.multinomial replaced FOR THE DURATION OF THE CALL by the project's draw rule on recorded uniforms (see
make_sample_golden.py); in tied_sample u is indexed by (member, CLOSING residue of the group). A uniform within MARGIN = 1e-3 of a
cumulative boundary is redrawn. torch.sum is watched for the duration of the call too: min_den is the smallest renormalising
denominator (log-odds and omit_AA_mask) the reference met, 1 when it met none. The generator asserts min_margin >= 1e-3 and
min_den >= 0.25. Stores only tensors: the inputs, S, probs, decoding_order, tied_pos (padded with -1), tied_beta, min_margin, min_den.

    fixture               N  temperature  content
    tied_syn_L32          3  1.0          pairs [i, 16+i] for i < 10, the triple [10, 11, 27]; tied_beta[16..18] = 0.5, [27] = -0.5;
                                          chain_M_pos = 0 at 5 (not closing) and 20 (closing)
    tied_2OCJ_AB          2  0.5          [i, 194+i] for all 194; letter 20 omitted, bias_AAs, bias_by_res and omit_AA_mask on a few
                                          positions, every fifth position fixed, both PSSM flags (pssm_multi 0.3, pssm_coef on every
                                          third position, 3 letters dropped on every fourth)
    tied_msk_L56_2ch      2  0.5          [i, 28+i] for all 28 on the masked two-chain layout; the reference's E_idx stored
    sample_pssm_syn_L32   3  1.0          the reference's `sample` with both PSSM flags
    tied_featurize_2OCJ_AB                the reference's tied_featurize 20-tuple on the two-chain parse with all four dictionaries
                                          (stored with the dictionaries, as JSON text and arrays)
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

import make_golden as mg          # the same directory: imports the reference
from make_sample_golden import MARGIN, draw, inputs_of

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_DEN = 0.25
PAIRS_SYN = [[i, 16 + i] for i in range(10)] + [[10, 11, 27]]
CASES = {
    "tied_syn_L32": dict(struct="syn_L32", N=3, temperature=1.0, tied=PAIRS_SYN, beta={16: 0.5, 17: 0.5, 18: 0.5, 27: -0.5}, fixed=(5, 20)),
    "tied_2OCJ_AB": dict(struct="2OCJ_AB", N=2, temperature=0.5, tied=[[i, 194 + i] for i in range(194)], extras=True, pssm=True),
    "tied_msk_L56_2ch": dict(struct="msk_L56_2ch", N=2, temperature=0.5, tied=[[i, 28 + i] for i in range(28)], store_graph=True),
    "sample_pssm_syn_L32": dict(struct="syn_L32", N=3, temperature=1.0, tied=None, pssm=True),
}


def regroup(order_row, tied):
    """The reference's regrouping (:1405-1414), restated with lists -> list of groups in decoding order."""
    groups, seen = [], set()
    for t in order_row:
        if int(t) in seen:
            continue
        grp = next((g for g in tied if int(t) in g), [int(t)])
        groups.append(list(grp))
        seen.update(grp)
    return groups


def pssm_tables(N, L, gen):
    coef = torch.zeros(N, L)
    coef[:, ::3] = torch.rand(L, generator=gen)[::3]
    pb = torch.softmax(2 * torch.randn(L, 21, generator=gen), -1)[None].repeat(N, 1, 1)
    keep = torch.ones(N, L, 21)
    for pos in range(0, L, 4):
        keep[:, pos, torch.randperm(21, generator=gen)[:3]] = 0
    return coef, pb, keep


def run_case(mp, name, cfg, n):
    g = inputs_of(cfg["struct"])
    t = torch.from_numpy
    N, temperature, tied = cfg["N"], cfg["temperature"], cfg["tied"]
    L = len(g["S"])
    rep = lambda a: a[None].repeat(N, *([1] * a.dim()))
    X, mask = rep(t(g["X"]).float()), rep(t(g["mask"]).float())
    S_true = rep(t(g["S"].astype(np.int64)))
    ridx, cenc = rep(t(g["residue_idx"].astype(np.int64))), rep(t(g["chain_enc"].astype(np.int64)))
    gen = torch.Generator().manual_seed(700 + n)
    randn = torch.randn(N, L, generator=gen)
    u = torch.rand(N, L, generator=gen).numpy()
    chain_mask, chain_M_pos = torch.ones(N, L), torch.ones(N, L)
    omit, bias_aa = np.zeros(21, np.float32), np.zeros(21, np.float32)
    by_res, omit_mask = torch.zeros(N, L, 21), None
    tied_beta = torch.ones(L)
    for k, v in cfg.get("beta", {}).items():
        tied_beta[k] = v
    for pos in cfg.get("fixed", ()):
        chain_M_pos[:, pos] = 0.0
    if cfg.get("extras"):
        omit[20] = 1.0
        bias_aa = (0.5 * torch.randn(21, generator=gen)).numpy().astype(np.float32)
        for pos in (3, 50, 120, 197, 244, 380):
            by_res[:, pos] = 1.5 * torch.randn(21, generator=gen)
        omit_mask = torch.zeros(N, L, 21)
        for pos in (7, 88, 201, 282, 345):
            omit_mask[:, pos, torch.randperm(20, generator=gen)[:3]] = 1.0
        chain_M_pos[:, ::5] = 0.0
    kw = {}
    if cfg.get("pssm"):
        coef, pb, keep = pssm_tables(N, L, gen)
        kw = dict(pssm_coef=coef, pssm_bias=pb, pssm_multi=0.3, pssm_log_odds_flag=True, pssm_log_odds_mask=keep, pssm_bias_flag=True)
    state = dict(order=None, draws=None, calls=0, redraws=0, min_margin=np.inf, min_den=1.0)
    real_argsort, real_multinomial, real_sum = torch.argsort, torch.multinomial, torch.sum

    def recording_argsort(*a, **k):
        out = real_argsort(*a, **k)
        if state["order"] is None:
            state["order"] = out.clone().numpy()
            if tied is None:        # sample: a draw at every step where some member's residue is unmasked; u by (member, residue)
                m = g["mask"][state["order"]]
                state["draws"] = [state["order"][:, s] for s in range(L) if not (m[:, s] == 0).all()]
            else:                   # tied_sample: a draw per live group; u by (member, the group's last listed residue)
                state["groups"] = regroup(state["order"][0], tied)
                state["draws"] = [np.full(N, grp[-1]) for grp in state["groups"] if all(g["mask"][k] != 0 for k in grp)]
        return out

    def rule_multinomial(probs, num_samples, *a, **k):
        assert num_samples == 1 and probs.shape == (N, 21)
        where = state["draws"][state["calls"]]
        state["calls"] += 1
        picks = []
        for b in range(N):
            res = int(where[b])
            p = probs[b].numpy().astype(np.float32)
            pick, margin = draw(p, u[b, res])
            while margin < MARGIN:
                u[b, res] = float(torch.rand(1, generator=gen))
                state["redraws"] += 1
                pick, margin = draw(p, u[b, res])
            state["min_margin"] = min(state["min_margin"], margin)
            picks.append(pick)
        return torch.tensor(picks, dtype=torch.int64)[:, None]

    def watching_sum(x, *a, **k):
        out = real_sum(x, *a, **k)
        if x.dim() == 2 and x.shape[-1] == 21 and k.get("keepdim"):
            state["min_den"] = min(state["min_den"], float(out.min()))
        return out

    graph = {}
    hook = mp.features.register_forward_hook(lambda m, i, o: graph.update(E_idx=o[1][0].numpy().astype(np.int16)))
    with torch.no_grad():
        torch.argsort, torch.multinomial, torch.sum = recording_argsort, rule_multinomial, watching_sum
        try:
            common = dict(mask=mask, temperature=temperature, omit_AAs_np=omit, bias_AAs_np=bias_aa, chain_M_pos=chain_M_pos,
                          omit_AA_mask=omit_mask, bias_by_res=by_res, **kw)
            if tied is None:
                out = mp.sample(X, randn, S_true, chain_mask, cenc, ridx, **common)
            else:
                out = mp.tied_sample(X, randn, S_true, chain_mask, cenc, ridx, tied_pos=tied, tied_beta=tied_beta, **common)
        finally:
            torch.argsort, torch.multinomial, torch.sum = real_argsort, real_multinomial, real_sum
    hook.remove()
    assert state["calls"] == len(state["draws"]), (state["calls"], len(state["draws"]))
    assert state["min_margin"] >= MARGIN and state["min_den"] >= MIN_DEN, (state["min_margin"], state["min_den"])
    S, P = out["S"].numpy(), out["probs"].numpy()
    extra = dict(graph) if cfg.get("store_graph") else {}
    if tied is not None:
        flat = [k for grp in state["groups"] for k in grp]
        assert (out["decoding_order"].numpy() == np.asarray(flat)[None]).all()
        assert all(len(set(S[b, grp].tolist())) == 1 for b in range(N) for grp in tied)
        width = max(len(grp) for grp in tied)
        extra["tied_pos"] = np.array([list(grp) + [-1] * (width - len(grp)) for grp in tied], np.int32)
        extra["tied_beta"] = tied_beta.numpy()
    if omit_mask is not None:
        extra["omit_AA_mask"] = omit_mask.numpy().astype(np.float32)
    if kw:
        extra.update(pssm_coef=kw["pssm_coef"].numpy(), pssm_bias=kw["pssm_bias"].numpy(), pssm_multi=np.float32(kw["pssm_multi"]),
                     pssm_log_odds_mask=kw["pssm_log_odds_mask"].numpy())
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, randn=randn.numpy(), chain_mask=chain_mask.numpy(), chain_M_pos=chain_M_pos.numpy(),
                        free=(chain_mask * chain_M_pos).numpy(), u=u.astype(np.float32), temperature=np.float32(temperature),
                        omit_AAs=omit, bias_AAs=bias_aa, bias_by_res=by_res.numpy(), S_true=S_true.numpy().astype(np.int32),
                        S=S.astype(np.int32), probs=P, decoding_order=out["decoding_order"].numpy().astype(np.int32),
                        min_margin=np.float64(state["min_margin"]), min_den=np.float64(state["min_den"]),
                        n_redraws=np.int32(state["redraws"]), **extra)
    print(f"{name}: N={N}, L={L}, T={temperature}: {state['calls']} draws, {state['redraws']} redraws, min margin "
          f"{state['min_margin']:.2e}, min den {state['min_den']:.3f}, non-zero probs rows {int((P.sum(-1) > 0).sum())} of {N * L} -> "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def featurize_case():
    """The reference's tied_featurize on 2OCJ chains A + B with all four dictionaries; the dictionaries are stored beside the tuple."""
    pdb = mg.ref_utils.alt_parse_PDB(os.path.join(HERE, "2OCJ.pdb"), ["A", "B"])[0]
    name = pdb["name"]
    rng = np.random.default_rng(11)
    nA, nB = len(pdb["seq_chain_A"]), len(pdb["seq_chain_B"])
    spec = dict(chain_dict={name: [["A", "B"], []]},
                fixed_position_dict={name: {"A": [1, 2, 50], "B": [10]}},
                omit_AA_dict={name: {"A": [[[1, 2, 3], "GPC"], [[40], "W"]], "B": [[[5, 6], "AC"]]}},
                tied_positions_dict={name: [{"A": [1], "B": [1]}, {"A": [[2, 3], [0.5, -0.25]], "B": [[2], [1.5]]}, {"A": [10, 11], "B": [12]}]})
    arrays = {}
    pssm, by_res = {name: {}}, {name: {}}
    for letter, n in (("A", nA), ("B", nB)):
        arrays[f"pssm_coef_{letter}"] = rng.random(n).astype(np.float32)
        arrays[f"pssm_bias_{letter}"] = rng.dirichlet(np.ones(21), n).astype(np.float32)
        arrays[f"pssm_log_odds_{letter}"] = rng.normal(size=(n, 21)).astype(np.float32)
        arrays[f"bias_by_res_{letter}"] = rng.normal(size=(n, 21)).astype(np.float32)
        pssm[name][letter] = {k: arrays[f"{k}_{letter}"] for k in ("pssm_coef", "pssm_bias", "pssm_log_odds")}
        by_res[name][letter] = arrays[f"bias_by_res_{letter}"]
    out = mg.ref_utils.tied_featurize([pdb], "cpu", spec["chain_dict"], spec["fixed_position_dict"], spec["omit_AA_dict"],
                                      spec["tied_positions_dict"], pssm, by_res)
    stored = {}
    for i, v in enumerate(out):
        if isinstance(v, torch.Tensor):
            stored[f"out{i}"] = v.numpy()
        elif isinstance(v, np.ndarray):
            stored[f"out{i}"] = v
    lists = {str(i): out[i] for i in (6, 7, 8, 9)}
    lists["14"] = [[[int(k) for k in grp] for grp in member] for member in out[14]]
    path = os.path.join(HERE, "tied_featurize_2OCJ_AB.npz")
    np.savez_compressed(path, spec=np.array(json.dumps(spec)), lists=np.array(json.dumps(lists)), **arrays, **stored)
    print(f"tied_featurize_2OCJ_AB: L={nA}+{nB}, tied {lists['14']} -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mp = mg.build_reference_model(tmp).prot_mpnn
    for n, (name, cfg) in enumerate(CASES.items()):
        run_case(mp, name, cfg, n)
    featurize_case()


if __name__ == "__main__":
    main()
