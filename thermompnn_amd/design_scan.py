"""Sequence design for MANY backbones: a few sampled sequences per structure, all structures of a batch inside one launch
(Engine.sample_each, csrc/tmpnn_sample.hip), scored by one order-masked decode over the same context.

    python -m thermompnn_amd.design_scan a.pdb b.pdb ... --num_seq 8 --temperature 0.1 --seed 0 [--chain A] [--fixed 1,5,10-20]
                                         --out designs.fa [--synthetic_weights 0 | --model_path CKPT] [--precision f16x2] [--ca_only]

The files are parsed with the native reader and packed into batches of at most ``--max_residues`` residues. Per batch: one
``encode``, one ``sample_each`` (``num_seq`` chains per structure, each with its own random decoding order inside its structure)
and one ``decode_ordered`` under the sampler's own orders, whose log-probabilities give the reference's score
(protein_mpnn_utils.py:20-29: the mean -log p of the chosen letters over the designed, unmasked positions). ``--fixed`` lists
1-based positions of the parsed sequence kept at the native letter in every file. The letter X is never drawn (the reference
driver's default omit_AAs). FASTA: per file the native sequence, then ``num_seq`` records
``>name, sample=k, T=temperature, seed=seed, score=..., seq_recovery=...``; residues without a full backbone are written as X.
``--seed`` fixes the decoding orders and the uniforms through one ``torch.Generator`` consumed file by file, so a file's
designs do not depend on how the files were batched.
``--ca_only`` designs on the C-alpha trace alone with a ProteinMPNN(ca_only=True) weight set (``--model_path`` then names a
ca_model_weights checkpoint): only the CA atoms are read, and a residue counts as present when its CA atom is.
Not here: tied positions and PSSM terms (Engine.sample_tied_each), per-file fixed positions, multi-GPU sharding of the files."""
from __future__ import annotations

import argparse
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .datasets import ALPHABET


def scores(S: torch.Tensor, log_probs: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The reference's ``_scores``: S [..., L] letters, log_probs [..., L, 21], mask [..., L] -> [...] the mean negative
    log-probability of the chosen letters over the positions with mask 1 (sum(loss * mask) / sum(mask); NaN where none)."""
    loss = -torch.gather(log_probs, -1, S.to(torch.int64)[..., None])[..., 0]
    mask = mask.to(loss.dtype)
    return (loss * mask).sum(-1) / mask.sum(-1)


def parse_positions(text: Optional[str]) -> List[int]:
    """'1,5,10-20' (1-based, inclusive ranges) -> sorted 0-based positions."""
    out = set()
    for part in (text or "").split(","):
        part = part.strip()
        if not part:
            continue
        a, _, b = part.partition("-")
        lo, hi = int(a), int(b or a)
        if lo < 1 or hi < lo:
            raise ValueError(f"--fixed: bad range {part!r} (1-based positions, a-b with a <= b)")
        out.update(range(lo - 1, hi))
    return sorted(out)


def pack_batches(lengths: Sequence[int], max_residues: int) -> List[List[int]]:
    """File indices in consecutive batches of at most ``max_residues`` residues (a longer file gets a batch of its own)."""
    batches, cur, used = [], [], 0
    for i, L in enumerate(lengths):
        if cur and used + L > max_residues:
            batches.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += L
    if cur:
        batches.append(cur)
    return batches


def draw_chains(entry: dict, num_seq: int, fixed: Sequence[int], generator: torch.Generator) -> dict:
    """The chains of one structure (local indices): the reference's decoding order — argsort of (designed + 0.0001) * |randn|,
    fixed and masked positions first — from ``num_seq`` rows of ``torch.randn``, then the uniforms from ``torch.rand``, both
    from ``generator`` -> dict(order int64 [N,L], S_fixed int64 [N,L], free float32 [N,L], u float32 [N,L])."""
    L = len(entry["S"])
    free = np.ones(L, np.float32)
    free[[p for p in fixed if p < L]] = 0
    randn = torch.randn((num_seq, L), generator=generator)
    u = torch.rand((num_seq, L), generator=generator)
    designed = torch.from_numpy(free * np.asarray(entry["mask"], np.float32))
    order = torch.argsort((designed[None] + 0.0001) * randn.abs(), dim=1)
    return dict(order=order.numpy().astype(np.int64), S_fixed=np.tile(np.asarray(entry["S"], np.int64), (num_seq, 1)),
                free=np.tile(free, (num_seq, 1)), u=u.numpy().astype(np.float32))


def join_chains(chains: Sequence[dict]) -> dict:
    """Per-structure chains -> the arrays of one packed batch ([N, T]; orders shifted to packed indices)."""
    starts = np.concatenate([[0], np.cumsum([c["order"].shape[1] for c in chains])])
    out = {k: np.concatenate([c[k] for c in chains], axis=1) for k in ("S_fixed", "free", "u")}
    out["order"] = np.concatenate([c["order"] + starts[b] for b, c in enumerate(chains)], axis=1)
    return out


def ranks_of(order: torch.Tensor) -> torch.Tensor:
    """order [N,T] (a permutation per row) -> rank [N,T] int32 with rank[n, order[n, s]] = s."""
    N, T = order.shape
    rank = torch.empty((N, T), dtype=torch.int32, device=order.device)
    rank.scatter_(1, order.to(torch.int64), torch.arange(T, dtype=torch.int32, device=order.device)[None].expand(N, T).contiguous())
    return rank


def design_batch(eng, entries: Sequence[dict], chains: Sequence[dict], temperature: float, max_rows: Optional[int] = None) -> List[dict]:
    """One batch: encode, sample_each, decode_ordered -> per structure dict(S int64 [N,L], score [N], seq_recovery [N])."""
    cat = lambda k: np.concatenate([np.asarray(e[k]) for e in entries])
    starts = np.concatenate([[0], np.cumsum([len(e["S"]) for e in entries])])
    c = join_chains(chains)
    T = int(starts[-1])
    bias = np.zeros((T, 21), np.float32)
    bias[:, 20] = -1e8                                                 # X is never drawn
    enc = eng.encode(cat("X"), cat("mask"), cat("residue_idx"), cat("chain_enc"), torch.tensor(starts, dtype=torch.int32))
    res = eng.sample_each(enc, c["order"], c["S_fixed"], c["free"], c["u"], temperature=temperature, bias=bias, max_rows=max_rows)
    order = torch.as_tensor(c["order"], device=eng.device)
    lp = eng.decode_ordered(enc, res["S"], ranks_of(order), max_rows=max_rows)["log_probs"]
    designed = torch.as_tensor(c["free"] * cat("mask")[None], device=eng.device)
    native = torch.as_tensor(cat("S"), device=eng.device)[None]
    out = []
    for b in range(len(entries)):
        t0, t1 = int(starts[b]), int(starts[b + 1])
        S, d = res["S"][:, t0:t1], designed[:, t0:t1]
        out.append(dict(S=S.to(torch.int64).cpu().numpy(), score=scores(S, lp[:, t0:t1].double(), d.double()).cpu().numpy(),
                        seq_recovery=(((S == native[:, t0:t1]).to(d.dtype) * d).sum(-1) / d.sum(-1)).cpu().numpy()))
    return out


def letters(S: Sequence[int], mask: Sequence[float]) -> str:
    """Letters of one sequence; a residue with mask 0 (no full backbone) is written as X."""
    return "".join(ALPHABET[int(s)] if m > 0 else "X" for s, m in zip(S, mask))


def fasta_records(name: str, entry: dict, result: dict, temperature: float, seed: int) -> str:
    """The records of one file: the native sequence, then one record per sample."""
    mask = entry["mask"]
    lines = [f">{name}, native, L={len(mask)}, unmasked={int(np.sum(np.asarray(mask) > 0))}", letters(entry["S"], mask)]
    for k, row in enumerate(result["S"]):
        lines.append(f">{name}, sample={k + 1}, T={temperature:g}, seed={seed}, score={float(result['score'][k]):.6f}, "
                     f"seq_recovery={float(result['seq_recovery'][k]):.4f}")
        lines.append(letters(row, mask))
    return "\n".join(lines) + "\n"


def main(argv=None):
    from . import weights
    from .engine import Engine
    from .native_pdb import parse_pdbs
    ap = argparse.ArgumentParser(description="ProteinMPNN sequence design for many backbones on MI355X: all structures of a batch in one launch")
    ap.add_argument("pdb", nargs="+")
    ap.add_argument("--chain", default=None, help="chain ids to design, e.g. A or AB (default: every chain)")
    ap.add_argument("--num_seq", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fixed", default=None, help="1-based positions kept at the native letter, e.g. 1,5,10-20")
    ap.add_argument("--out", required=True, help="output FASTA")
    ap.add_argument("--model_path", default="")
    ap.add_argument("--synthetic_weights", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--max_residues", type=int, default=4096, help="residue budget of one batch")
    ap.add_argument("--ca_only", action="store_true", help="C-alpha-only model (ca_model_weights/v_48_*): reads the CA atoms alone")
    a = ap.parse_args(argv)
    if a.num_seq < 1 or not a.temperature > 0:
        ap.error("--num_seq must be >= 1 and --temperature positive")
    if a.synthetic_weights is None and not a.model_path:
        ap.error("give --model_path or --synthetic_weights")
    if a.ca_only:
        sd = weights.synthetic_state_dict(a.synthetic_weights, "mpnn_ca") if a.synthetic_weights is not None else \
            weights.load_vanilla_checkpoint(a.model_path)[1]
    else:
        sd = weights.synthetic_state_dict(a.synthetic_weights) if a.synthetic_weights is not None else weights.load_thermompnn_checkpoint(a.model_path)
    eng = Engine(sd, "cuda", 48, precision=a.precision, ca_only=a.ca_only)
    fixed = parse_positions(a.fixed)
    entries = parse_pdbs(a.pdb, [a.chain] * len(a.pdb) if a.chain else None)
    if a.ca_only:
        for e in entries:
            e["mask"] = e["ca_mask"]          # (tied_featurize(ca_only=True): present = the CA atom is)
    gen = torch.Generator().manual_seed(a.seed)
    chains = [draw_chains(e, a.num_seq, fixed, gen) for e in entries]
    names = [os.path.splitext(os.path.basename(p))[0] for p in a.pdb]
    with open(a.out, "w") as fh, torch.no_grad():
        for batch in pack_batches([len(e["S"]) for e in entries], a.max_residues):
            results = design_batch(eng, [entries[i] for i in batch], [chains[i] for i in batch], a.temperature)
            for i, r in zip(batch, results):
                fh.write(fasta_records(names[i], entries[i], r, a.temperature, a.seed))
    print(f"{len(entries)} structures x {a.num_seq} sequences -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
