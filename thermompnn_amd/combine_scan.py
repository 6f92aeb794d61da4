"""The beam search for multi-point mutants (``variant_scan --combine``) for MANY structures in one run: the files are packed, a pack is
encoded once, and every round is one decode of the pack's beams plus one step on the device for all of its proteins
(variant_scan.multi_mutant_search_each, Engine.beam_step_each, csrc/tmpnn_beam.hip).

    python -m thermompnn_amd.combine_scan a.pdb b.pdb ... --chain A --combine N --beam K --out hits.csv [--cutoff X] [--include_cys]
                                          [--synthetic_weights S | --model_path CKPT] [--precision P] [--pack_residues R]

The CSV holds ``variant_scan``'s --combine columns behind a leading ``pdb`` column (the file's base name without its extension),
structures in argument order; for one file the rows behind the first column are byte for byte what ``variant_scan --combine`` writes.
Limits: every structure <= 2048 residues, N <= 8, K * N <= 256, one N and one K for all files, one rank."""
from __future__ import annotations

import argparse
import csv
import os
from typing import Callable, Optional, Sequence

import torch

from .variant_scan import BEAM_MAX_KD, BEAM_MAX_ORDER, MULTI_CSV_HEADER, MultiHit, multi_mutant_search_each


def write_multi_hits_each_csv(path: str, names: Sequence[str], results: Sequence[Sequence[Sequence[MultiHit]]]) -> int:
    """``variant_scan.write_multi_hits_csv``'s rows for every structure, behind a leading ``pdb`` column."""
    sub = lambda m: f"{m.wildtype}{m.position + 1}{m.mutation}"
    rows = 0
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["pdb"] + MULTI_CSV_HEADER)
        for name, levels in zip(names, results):
            for d, hits in enumerate(levels, 1):
                for r, h in enumerate(hits):
                    w.writerow([name, d, r, ":".join(sub(m) for m in h.mutations), repr(h.ddG), repr(h.ddG_additive), repr(h.epistasis)])
                    rows += 1
    return rows


def main(argv=None, _tables: Optional[Callable] = None, _step: Optional[Callable] = None):
    """(``_tables`` / ``_step``: the hooks of ``multi_mutant_search_each``; with ``_tables`` no model is loaded.)"""
    from .custom_inference import load_model
    from .pdb_io import alt_parse_PDB
    ap = argparse.ArgumentParser(description="Beam search for the most stabilising multi-point mutants of many structures on MI355X")
    ap.add_argument("pdb", nargs="+")
    ap.add_argument("--chain", default="A")
    ap.add_argument("--combine", type=int, required=True, metavar="N", help="mutants of 1 .. N substitutions")
    ap.add_argument("--beam", type=int, required=True, metavar="K", help="mutants kept per level and structure (K * N <= 256)")
    ap.add_argument("--out", required=True, help="output .csv")
    ap.add_argument("--cutoff", type=float, default=None, help="keep mutants with ddG <= cutoff")
    ap.add_argument("--include_cys", action="store_true", help="substitutions to cysteine take part")
    ap.add_argument("--model_path", default="")
    ap.add_argument("--thermompnn_dir", default=".")
    ap.add_argument("--synthetic_weights", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--pack_residues", type=int, default=16384, help="residue budget of one pack")
    a = ap.parse_args(argv)
    if not 1 <= a.combine <= BEAM_MAX_ORDER:
        ap.error(f"--combine {a.combine}: outside [1, {BEAM_MAX_ORDER}]")
    if a.beam < 1 or a.beam * a.combine > BEAM_MAX_KD:
        ap.error(f"--beam {a.beam}: at least 1, and --beam times --combine at most {BEAM_MAX_KD}")
    if a.pack_residues < 1:
        ap.error(f"--pack_residues {a.pack_residues}: at least 1")
    model = None if _tables is not None else load_model(a.model_path or None, a.thermompnn_dir, a.synthetic_weights, precision=a.precision)
    pdbs = [alt_parse_PDB(path, a.chain) for path in a.pdb]
    with torch.no_grad():
        results = multi_mutant_search_each(model, pdbs, a.combine, a.beam, cutoff=a.cutoff, include_cys=a.include_cys,
                                           pack_residues=a.pack_residues, _tables=_tables, _step=_step)
    names = [os.path.splitext(os.path.basename(path))[0] for path in a.pdb]
    rows = write_multi_hits_each_csv(a.out, names, results)
    print(f"{rows} mutants of 1 .. {a.combine} substitutions of {len(pdbs)} structures -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
