"""ddG tables of one backbone under many sequences: the encoder runs once (Engine.encode), the decoder and the head once per
variant with the backbone's edge tiles shared between variants (Engine.decode_variants, csrc/tmpnn_variants.hip).

    python -m thermompnn_amd.variant_scan a.pdb --chain A (--variants FILE | --all-singles) --out x.npz [--synthetic_weights N]

FILE holds one variant per line: a full one-letter sequence of the parsed length, or a comma-separated list of substitutions
such as ``A12G,K45E`` (wild type, 1-based position in the parsed sequence, new residue). Writes ``tables`` float32 [V, L, 21]
(entry [v, pos, a]: ddG of mutating position pos of variant v to ALPHABET[a], relative to the variant's own residue),
``variants`` (the V sequences) and ``wild_type``.
Not here: CSV output and the native writer, multi-GPU sharding of the variants, hipGraph capture, the training paths,
ProteinMPNN.forward and examples/."""
from __future__ import annotations

import argparse
import re
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .datasets import ALPHABET, Mutation

_CODE = {a: i for i, a in enumerate(ALPHABET)}
_SUB = re.compile(r"^([A-Za-z])(\d+)([A-Za-z])$")


def sequence_indices(seq: str) -> np.ndarray:
    """The parser's one-letter sequence -> ALPHABET indices; '-' (numbering gap / unknown residue) and unknown letters -> 20."""
    return np.array([_CODE.get(c, 20) for c in seq], dtype=np.int64)


def variant_matrix(seq: str, variants: Sequence) -> np.ndarray:
    """``variants``: each a full one-letter sequence of len(seq), or a list of Mutation applied to ``seq`` -> int64 [V, L].
    ValueError on a wrong length, an unknown letter, a position out of range, a stated wild type that differs from the parsed
    residue, or a substitution at a '-' position."""
    L, base = len(seq), sequence_indices(seq)
    out = np.empty((len(variants), L), dtype=np.int64)
    for v, var in enumerate(variants):
        if isinstance(var, str):
            if len(var) != L:
                raise ValueError(f"variant {v}: sequence of length {len(var)}, the structure has {L} residues")
            for k, c in enumerate(var):
                if c not in _CODE and c != "-":
                    raise ValueError(f"variant {v}: unknown residue {c!r} at position {k}")
                if (c == "-") != (seq[k] == "-") and "-" in (c, seq[k]):
                    raise ValueError(f"variant {v}: position {k} is {seq[k]!r} in the structure and {c!r} in the variant "
                                     "(a '-' position has no residue to substitute)")
            out[v] = sequence_indices(var)
            continue
        row = base.copy()
        for m in var:
            if not 0 <= int(m.position) < L:
                raise ValueError(f"variant {v}: position {m.position} outside [0, {L})")
            if seq[m.position] == "-":
                raise ValueError(f"variant {v}: position {m.position} is '-' in the structure (no residue to substitute)")
            if m.wildtype and m.wildtype != seq[m.position]:
                raise ValueError(f"variant {v}: stated wild type {m.wildtype}{m.position} but the structure has {seq[m.position]}")
            if m.mutation not in _CODE:
                raise ValueError(f"variant {v}: unknown residue {m.mutation!r}")
            row[m.position] = _CODE[m.mutation]
        out[v] = row
    return out


def parse_variant_line(line: str):
    """'A12G,K45E' (1-based positions) -> [Mutation, ...]; anything else is taken as a full sequence."""
    parts = [p.strip() for p in line.strip().split(",")]
    subs = [_SUB.match(p) for p in parts]
    if all(subs):
        return [Mutation(int(m.group(2)) - 1, m.group(1).upper(), m.group(3).upper()) for m in subs]
    return line.strip()


def read_variants(path: str) -> List:
    with open(path) as fh:
        return [parse_variant_line(l) for l in fh if l.strip() and not l.startswith("#")]


def single_backgrounds(seq: str, positions: Optional[Sequence[int]] = None, mask: Optional[np.ndarray] = None):
    """Every single-substitution background at ``positions`` (default: all residues that are not '-' and, with ``mask``, unmasked)
    -> (positions [P], S int64 [P, 20, L]): S[k, a] is the parsed sequence with residue a at positions[k] (20 rows per position; the
    row whose residue is the wild type's is the parsed sequence itself)."""
    base = sequence_indices(seq)
    if positions is None:
        positions = [k for k, c in enumerate(seq) if c != "-" and (mask is None or mask[k] > 0)]
    positions = [int(p) for p in positions]
    for p in positions:
        if not 0 <= p < len(seq) or seq[p] == "-":
            raise ValueError(f"position {p}: outside the sequence or a '-' position")
    S = np.tile(base, (len(positions), 20, 1))
    for k, p in enumerate(positions):
        S[k, np.arange(20), p] = np.arange(20)
    return positions, S


def double_mutant_table(model, pdb, positions: Optional[Sequence[int]] = None, chunk: int = 256,
                        _tables: Optional[Callable] = None) -> torch.Tensor:
    """ddG of every double mutant (p:a, q:b) relative to the wild type, [P, 20, L, 20] on the model's device:
        ddG(p:a, q:b) = table_wt[p, a] + table_{p:a}[q, b]
    where table_{p:a} is the site-saturation table on the backbone with the single substitution p:a as background (row a = wild
    type of p is the wild-type table itself). ``positions`` default: every residue of the parsed sequence that is not '-'.
    Backgrounds are decoded ``chunk`` at a time; the encoder runs once. (``_tables(S [V, L]) -> [V, L, 21]``: the table function,
    default ``model.variant_tables`` on index matrices.)"""
    entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
    seq = entry["seq"]
    positions, S = single_backgrounds(seq, positions)
    tables = _tables if _tables is not None else (lambda s: model.variant_tables(pdb, s))
    P, L = len(positions), len(seq)
    wt = tables(sequence_indices(seq)[None])[0]                        # [L, 21]
    out = torch.empty((P, 20, L, 20), dtype=wt.dtype, device=wt.device)
    flat = S.reshape(P * 20, L)
    pos_of = torch.as_tensor(np.repeat(positions, 20), device=wt.device)
    aa_of = torch.as_tensor(np.tile(np.arange(20), P), device=wt.device)
    view = out.view(P * 20, L, 20)
    for v0 in range(0, P * 20, chunk):
        v1 = min(P * 20, v0 + chunk)
        t = tables(flat[v0:v1])                                        # [n, L, 21]
        view[v0:v1] = wt[pos_of[v0:v1], aa_of[v0:v1]][:, None, None] + t[:, :, :20]
    return out


def main(argv=None):
    from .custom_inference import load_model
    from .pdb_io import alt_parse_PDB
    ap = argparse.ArgumentParser(description="ThermoMPNN ddG tables of one backbone under many sequence variants on MI355X")
    ap.add_argument("pdb")
    ap.add_argument("--chain", default="A")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--variants", help="file with one variant per line: a full sequence or a list like A12G,K45E")
    src.add_argument("--all-singles", action="store_true", help="every single-substitution background (19 per residue)")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--model_path", default="")
    ap.add_argument("--thermompnn_dir", default=".")
    ap.add_argument("--synthetic_weights", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--chunk", type=int, default=256, help="variants decoded per call")
    a = ap.parse_args(argv)
    model = load_model(a.model_path or None, a.thermompnn_dir, a.synthetic_weights, precision=a.precision)
    pdb = alt_parse_PDB(a.pdb, a.chain)
    seq = pdb[0]["seq"]
    if a.all_singles:
        _, S = single_backgrounds(seq)
        base = sequence_indices(seq)
        S = S.reshape(-1, len(seq))
        S = S[(S != base[None]).any(1)]                                # drop the 1-in-20 rows that are the wild type itself
    else:
        S = variant_matrix(seq, read_variants(a.variants))
    with torch.no_grad():
        tables = torch.cat([model.variant_tables(pdb, S[v0:v0 + a.chunk]) for v0 in range(0, len(S), a.chunk)]) if len(S) else \
            torch.empty((0, len(seq), 21))
    gap = np.array([c == "-" for c in seq])
    seqs = np.array(["".join("-" if gap[k] else ALPHABET[i] for k, i in enumerate(row)) for row in S])
    with open(a.out, "wb") as fh:
        np.savez(fh, tables=tables.cpu().numpy().astype(np.float32), variants=seqs, wild_type=np.array(seq))
    print(f"{len(S)} variants x {len(seq)} residues -> {a.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
