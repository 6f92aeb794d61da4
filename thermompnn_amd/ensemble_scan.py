"""Scan conformer ensembles: per-mutation ddG statistics across NMR models, AF2 ranks or MD frames, reduced on the GPU.

    python -m thermompnn_amd.ensemble_scan nmr.pdb [more.pdb ...] --chain A --out stats.npz   (or stats.csv)
    python -m thermompnn_amd.ensemble_scan rank_0.pdb rank_1.pdb rank_2.pdb --members --chain A --out stats.npz
    python -m thermompnn_amd.ensemble_scan nmr.pdb --chain A --top 20 --rank worst [--cutoff X] [--min_members N] --out hits.csv

Every multi-MODEL file is one ensemble (``pdb_io.parse_pdb_models``; a file without MODEL records is an ensemble of one); with
``--members`` all files together are the members of ONE ensemble. All ensembles of a call go through one fused forward per chunk of
``--chunk_residues`` residues and ONE reduction on the device (``ensemble.scan_ensembles``, csrc/tmpnn_ensemble.hip).
``.npz``: mean, spread, lo, hi (float32), lo_member, hi_member, count, below (int32), [sum(L), 20] each, rows ``offsets[e] ..
offsets[e + 1]`` being ensemble e; ``seqs``, ``names``, ``members`` (M per ensemble) and ``member_names``.
``.csv``: one line per (ensemble, position, letter other than the wild type; positions without a residue in any member have none)
with the columns ``TABLE_COLUMNS``.
``--top K``: the K best substitutions of every ensemble by ``--rank`` (mean; worst = the largest ddG over the members, so a hit is
stabilising in every conformer; best), as a CSV with ``ssm_scan.HIT_COLUMNS`` plus the statistics (``ensemble.select_ensemble_hits``).
``--align``: members of unequal length (construct boundaries, numbering, missing termini, tags, a point substitution) are aligned on
the device to ``--reference`` (a sequence or a one-record FASTA file; default: member 0's sequence) by the rule of
``datasets.global_alignment_map``; a member below ``--min_identity`` (default 0.9; 0 disables it) is refused. The ``.npz`` gains
``aligned`` (int32, flat: ensemble e's block of members[e] x L_e entries, member-local residue index or -1, the blocks in order) and
``identity`` (float64, one per member); the CSV layouts do not change.
``--superpose``: before the forward every member is laid on member ``--fit_to`` (default 0) of its ensemble by the optimal proper
rotation of the C-alpha atoms both have (``Engine.superpose``, csrc/tmpnn_superpose.hip); a member whose RMSD exceeds ``--max_rmsd``
is refused by name before any forward. The ``.npz`` gains ``rmsd`` (float32) and ``n_fit`` (int32), one per member, ``xform``
(float64 [members, 12]: R row-major, then t), ``deviation`` (float32, flat like ``aligned``) and ``rmsf`` (float32 [sum(L)], rows like
the statistics); the ``--top`` CSV gains an ``rmsf`` column. Without the flag every layout is as it was.
Limits: without --align members of equal length and sequence; L <= 8192, 65 535 ensembles, K <= 256, the released head, one rank, the
Python parser."""
from __future__ import annotations

import argparse
import csv
import os
from typing import List, Sequence

import numpy as np
import torch

from .datasets import ALPHABET
from .ensemble import RANKS, STAT_NAMES, scan_ensembles, select_ensemble_hits
from .ssm_scan import HIT_COLUMNS

SUPERPOSE_ARRAYS = dict(rmsd="rmsd", n_fit="n_fit", xform="xform", deviation="dev", rmsf="rmsf")    # .npz name -> Engine.superpose's
TABLE_COLUMNS = ["Model", "Dataset", "pdb", "position", "wildtype", "mutation"] + list(STAT_NAMES)


def _num(v) -> str:
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v))


def write_ensemble_npz(path: str, res: dict) -> None:
    arrays = {name: res["stats"][name].cpu().numpy() for name in STAT_NAMES}
    if "aligned" in res:
        arrays["aligned"] = np.concatenate([a.cpu().numpy().reshape(-1) for a in res["aligned"]] + [np.zeros(0, np.int32)]).astype(np.int32)
        arrays["identity"] = np.concatenate(list(res["identity"]) + [np.zeros(0, np.float64)])
    if "superposed" in res:
        arrays.update({name: res["superposed"][key].cpu().numpy() for name, key in SUPERPOSE_ARRAYS.items()})
    with open(path, "wb") as fh:
        np.savez(fh, **arrays, offsets=res["stats"]["offsets"].cpu().numpy(), seqs=np.array(res["seqs"]), names=np.array(res["ensemble_names"]),
                 members=np.array(res["members"], np.int32), member_names=np.array([n for group in res["names"] for n in group]))


def write_ensemble_csv(path: str, res: dict, model_name: str = "ThermoMPNN", dataset: str = "custom") -> int:
    """-> rows written. Floats as repr(float(v)), '\\n' line ends, a running index first, as the other CSVs of the package."""
    arrays = {name: res["stats"][name].cpu().numpy() for name in STAT_NAMES}
    offsets = res["stats"]["offsets"].cpu().numpy()
    n = 0
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow([""] + TABLE_COLUMNS)
        for e, (seq, name) in enumerate(zip(res["seqs"], res["ensemble_names"])):
            for q, wt in enumerate(seq):
                if wt not in ALPHABET[:20]:
                    continue
                row = int(offsets[e]) + q
                for b in range(20):
                    if ALPHABET[b] == wt:
                        continue
                    w.writerow([n, model_name, dataset, name, q, wt, ALPHABET[b]] + [_num(arrays[s][row, b]) for s in STAT_NAMES])
                    n += 1
    return n


def write_ensemble_hits_csv(path: str, hits: Sequence[Sequence], names: Sequence[str], model_name: str = "ThermoMPNN",
                            dataset: str = "custom", rmsf: bool = False) -> int:
    """``rmsf``: a last column with the RMSF of the hit's position (a superposed scan)."""
    n = 0
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow([""] + HIT_COLUMNS + list(STAT_NAMES) + (["rmsf"] if rmsf else []))
        for name, group in zip(names, hits):
            for r, h in enumerate(group):
                w.writerow([n, model_name, dataset, repr(h.ddG), h.position, h.wildtype, h.mutation, r, name] +
                           [_num(getattr(h, s)) if s in ("lo_member", "hi_member", "count", "below") else repr(getattr(h, s)) for s in STAT_NAMES] +
                           ([repr(h.rmsf)] if rmsf else []))
                n += 1
    return n


def read_ensembles(paths: Sequence[str], chain, members: bool):
    """-> (ensembles: lists of parsed members, ensemble names)."""
    from .pdb_io import parse_pdb_models
    stem = lambda p: os.path.basename(p)[:-4]
    parsed = [parse_pdb_models(p, chain) for p in paths]
    if members:
        return [[e for group in parsed for e in group]], [stem(paths[0])]
    return parsed, [stem(p) for p in paths]


def main(argv=None) -> int:
    from .custom_inference import load_model
    ap = argparse.ArgumentParser(description="ThermoMPNN ddG statistics over conformer ensembles on MI355X")
    ap.add_argument("pdbs", nargs="+", help="multi-MODEL PDB files, one ensemble each (--members: the members of one ensemble)")
    ap.add_argument("--chain", default="A")
    ap.add_argument("--members", action="store_true", help="all files together are the members of ONE ensemble")
    ap.add_argument("--out", required=True, help="output .npz or .csv (--top: .csv)")
    ap.add_argument("--top", type=int, default=None, metavar="K", help="the K best substitutions of every ensemble as a CSV (1 <= K <= 256)")
    ap.add_argument("--rank", default=None, choices=sorted(RANKS), help="--top: the statistic to rank by (default mean)")
    ap.add_argument("--cutoff", type=float, default=None, help="`below` counts the members with ddG <= cutoff; --top: keep hits <= cutoff")
    ap.add_argument("--min_members", type=int, default=None, help="--top: only entries in which at least N members take part")
    ap.add_argument("--include_cys", action="store_true", help="--top: substitutions to cysteine take part")
    ap.add_argument("--one_per_position", action="store_true", help="--top: each position's best substitution only")
    ap.add_argument("--model_name", default="ThermoMPNN")
    ap.add_argument("--dataset", default="custom")
    ap.add_argument("--model_path", default="")
    ap.add_argument("--thermompnn_dir", default=".")
    ap.add_argument("--synthetic_weights", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--chunk_residues", type=int, default=1 << 18, help="residues per forward")
    ap.add_argument("--align", action="store_true", help="align members of unequal length to the axis on the device")
    ap.add_argument("--reference", default=None, metavar="SEQ|FASTA", help="--align: the axis, a sequence or a one-record FASTA file (default: member 0)")
    ap.add_argument("--min_identity", type=float, default=None, metavar="F", help="--align: refuse members below this identity (default 0.9; 0: none)")
    ap.add_argument("--superpose", action="store_true", help="superpose the members on the device: RMSD, deviations and RMSF beside the statistics")
    ap.add_argument("--fit_to", type=int, default=None, metavar="I", help="--superpose: the member every other one is laid on (default 0)")
    ap.add_argument("--max_rmsd", type=float, default=None, metavar="X", help="--superpose: refuse members further than X A (C-alpha RMSD) from it")
    a = ap.parse_args(argv)
    if not a.superpose and (a.fit_to is not None or a.max_rmsd is not None):
        ap.error("--fit_to and --max_rmsd belong to --superpose")
    if not a.align and (a.reference is not None or a.min_identity is not None):
        ap.error("--reference and --min_identity belong to --align")
    if a.top is None and (a.rank or a.min_members is not None or a.include_cys or a.one_per_position):
        ap.error("--rank, --min_members, --include_cys and --one_per_position belong to --top")
    if a.top is not None and not 1 <= a.top <= 256:
        ap.error(f"--top {a.top}: a hit list holds 1 to 256 mutations per ensemble")
    if a.top is not None and not a.out.endswith(".csv"):
        ap.error("--top writes a CSV (name the output *.csv)")
    if a.top is None and not a.out.endswith((".npz", ".csv")):
        ap.error("--out: name the output *.npz or *.csv")
    if a.cutoff is not None and a.cutoff != a.cutoff:
        ap.error("--cutoff is NaN")
    ensembles, names = read_ensembles(a.pdbs, a.chain, a.members)
    model = load_model(a.model_path or None, a.thermompnn_dir, a.synthetic_weights, precision=a.precision)
    with torch.no_grad():
        res = scan_ensembles(model, ensembles, cutoff=a.cutoff, chunk_residues=a.chunk_residues, align=a.align, reference=a.reference,
                             min_identity=0.9 if a.min_identity is None else a.min_identity, superpose=a.superpose, fit_to=a.fit_to or 0,
                             max_rmsd=a.max_rmsd)
        res["ensemble_names"] = names
        if a.top is not None:
            hits: List[list] = select_ensemble_hits(model.engine(), res["stats"], res["seqs"], a.top, a.rank or "mean", a.cutoff,
                                                    a.include_cys, a.one_per_position, a.min_members,
                                                    rmsf=res["superposed"]["rmsf"] if a.superpose else None)
            rows = write_ensemble_hits_csv(a.out, hits, names, a.model_name, a.dataset, rmsf=a.superpose)
            print(f"{rows} hits of {len(names)} ensembles ({sum(res['members'])} members) -> {a.out}")
            return 0
    if a.out.endswith(".npz"):
        write_ensemble_npz(a.out, res)
        print(f"{len(names)} ensembles, {sum(res['members'])} members, {sum(len(s) for s in res['seqs'])} positions -> {a.out}")
    else:
        rows = write_ensemble_csv(a.out, res, a.model_name, a.dataset)
        print(f"{rows} rows of {len(names)} ensembles ({sum(res['members'])} members) -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
