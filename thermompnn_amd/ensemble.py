"""Conformer ensembles: per-mutation ddG statistics across the members of an ensemble (NMR models, AF2 ranks, MD frames).

ThermoMPNN's table depends on the backbone, so one table answers for one conformer only. Here the members of an ensemble go through
the fused forward as what they are, a ragged packed batch (a member's table does not depend on its batch), and ONE launch reduces the
packed table across the members (Engine.ensemble_stats, csrc/tmpnn_ensemble.hip): for every (position, letter) the mean, the
population spread, the smallest and the largest ddG with the members that hold them, the number of members that take part and the
number of those at or below a cutoff. No table goes to the host. The mean is a chain of fp32 adds in ascending member order and the
spread is taken around it (include/tmpnn.h has the contract to the operation), so every bit is reproducible.

Members must parse to the same length and to the same letter wherever both have a residue (``align_members``; alignment is out of
scope). A member's own '-', 'X' and rows with a missing backbone atom drop out of that position only. Limits: L <= 8192, 65 535
ensembles per call, the released head configuration with ``subtract_mut``, one rank. Multi-MODEL files are read by the Python parser
(``pdb_io.parse_pdb_models``) only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._lib import ENS_ARRAYS, ENS_MAX_LEN
from .datasets import ALPHABET
from .pdb_io import BACKBONE, _chain_letters, tied_featurize

_CODE = {a: i for i, a in enumerate(ALPHABET) if a != "X"}
STAT_NAMES = tuple(name for name, _ in ENS_ARRAYS)
RANKS = {"mean": "mean", "worst": "hi", "best": "lo"}      # the table a hit list is ranked by; "worst": stabilising in every conformer


def _backbone_complete(entry: dict) -> np.ndarray:
    """[L] bool: every stored backbone atom of the row is finite (the forward's own mask, pdb_io.tied_featurize)."""
    rows = []
    for letter in _chain_letters(entry):
        coords = entry[f"coords_chain_{letter}"]
        atoms = [a for a in BACKBONE if f"{a}_chain_{letter}" in coords]
        n = len(entry[f"seq_chain_{letter}"])
        xyz = np.stack([np.asarray(coords[f"{a}_chain_{letter}"], dtype=np.float64).reshape(n, 3) for a in atoms], 1)
        rows.append(np.isfinite(xyz.sum(axis=(1, 2))))
    return np.concatenate(rows) if rows else np.zeros(0, bool)


def align_members(entries: Sequence[dict]):
    """The parsed members of ONE ensemble -> (seq, S): the ensemble's sequence (at every position the letter of the first member
    that has one there, '-' where none has) and S [M, L] int32, each member's own letters as the statistics take them: 20 — the row
    takes no part — at the member's own '-', 'X' and rows with a missing backbone atom. ValueError, naming the member and the
    position, when a member's length differs from the first member's or two members hold different letters at one position."""
    if not entries:
        raise ValueError("an ensemble needs at least one member")
    first = entries[0]
    L = len(first["seq"])
    seq = ["-"] * L
    owner = [0] * L
    S = np.full((len(entries), L), 20, np.int32)
    for m, e in enumerate(entries):
        name = e.get("name", "")
        if len(e["seq"]) != L:
            raise ValueError(f"ensemble member {m} ({name}) has {len(e['seq'])} residues, member 0 ({first.get('name', '')}) has {L}: "
                             "members must parse to the same length (alignment is out of scope)")
        for q, c in enumerate(e["seq"]):
            if c not in _CODE:
                continue
            if seq[q] == "-":
                seq[q], owner[q] = c, m
            elif seq[q] != c:
                raise ValueError(f"ensemble member {m} ({name}) holds {c} at position {q}, member {owner[q]} holds {seq[q]}: "
                                 "members must have the same sequence (alignment is out of scope)")
            S[m, q] = _CODE[c]
        S[m, ~_backbone_complete(e)] = 20
    return "".join(seq), S


@dataclass
class EnsembleTable:
    """The statistics of one ensemble, [L, 20] each, on the device: entry [q, b] is over the members' ddG of mutating position q to
    ALPHABET[b]. ``lo_member`` / ``hi_member``: the member (index into ``names``) that holds the extreme, ties to the first; -1 and
    NaN where no member takes part (``count`` 0)."""
    mean: torch.Tensor
    spread: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    lo_member: torch.Tensor
    hi_member: torch.Tensor
    count: torch.Tensor
    below: torch.Tensor
    seq: str
    names: List[str]


@dataclass
class EnsembleHit:
    position: int
    wildtype: str
    mutation: str
    ddG: float          # the ranked statistic
    mean: float
    spread: float
    lo: float
    hi: float
    count: int
    below: int
    lo_member: int = -1
    hi_member: int = -1


def _check_model(model) -> None:
    if model.generic_head or not model.subtract_mut:
        raise NotImplementedError("ensemble statistics serve the released head configuration (hidden_dims [64, 32], num_final_layers 2, "
                                  "lightattn) with subtract_mut only; run ssm_table per member for other configurations")


def scan_ensembles(model, ensembles: Sequence[Sequence[dict]], cutoff: Optional[float] = None, chunk_residues: int = 1 << 18) -> dict:
    """Ensembles (each a list of parsed members) -> dict(stats: what ``Engine.ensemble_stats`` returns over ALL ensembles, rows
    ``offsets[e] .. offsets[e + 1]`` being ensemble e; seqs; names: per ensemble its members' names; members: M per ensemble).
    One ``tied_featurize`` per ensemble, ONE forward per chunk of whole members of at most ``chunk_residues`` residues (a chunk may
    end inside an ensemble: a member's table does not depend on its batch) into one packed device table, and ONE ``ensemble_stats``."""
    _check_model(model)
    device = next(model.parameters()).device
    eng = model.engine()
    seqs, names, S_stat, pieces, M_of, L_of = [], [], [], [], [], []
    for entries in ensembles:
        entries = list(entries)
        seq, S = align_members(entries)
        if len(seq) > ENS_MAX_LEN:
            raise ValueError(f"an ensemble of {len(seq)} residues exceeds {ENS_MAX_LEN}, the forward's own bound")
        seqs.append(seq)
        names.append([e.get("name", "") for e in entries])
        S_stat.append(S.reshape(-1))
        M_of.append(len(entries))
        L_of.append(len(seq))
        feats = tied_featurize(entries, device, None, None, None, None, None, None, ca_only=False)
        X, S_fwd, mask, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[5], feats[12]
        pieces.extend((X[m], S_fwd[m], mask[m], residue_idx[m], chain_enc[m]) for m in range(len(entries)))
    T = sum(m * l for m, l in zip(M_of, L_of))
    with torch.cuda.device(eng.device):
        table = torch.empty((T, 21), dtype=torch.float32, device=eng.device)
        pos, k = 0, 0
        while k < len(pieces):
            chunk, tot = [], 0
            while k < len(pieces) and (not chunk or tot + pieces[k][0].shape[0] <= chunk_residues):
                chunk.append(pieces[k])
                tot += pieces[k][0].shape[0]
                k += 1
            if tot == 0:
                continue
            lens = [p[0].shape[0] for p in chunk]
            offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
            X, S_fwd, mask, ridx, cenc = (torch.cat([p[i] for p in chunk]) for i in range(5))
            eng.ssm_forward(X, S_fwd, mask, ridx, cenc, offsets, max_len=max(lens), out={"ddg": table[pos:pos + tot]})
            pos += tot
        S_all = np.concatenate(S_stat) if S_stat else np.zeros(0, np.int32)
        stats = eng.ensemble_stats(table, S_all, M_of, L_of, cutoff=cutoff)
    return dict(stats=stats, seqs=seqs, names=names, members=M_of)


def ensemble_table(model, members: Sequence[dict], cutoff: Optional[float] = None) -> EnsembleTable:
    """``TransferModel.ensemble_table``: one ensemble -> its ``EnsembleTable``."""
    res = scan_ensembles(model, [members], cutoff=cutoff)
    return EnsembleTable(**{name: res["stats"][name] for name in STAT_NAMES}, seq=res["seqs"][0], names=res["names"][0])


def select_ensemble_hits(engine, stats: Dict[str, torch.Tensor], seqs: Sequence[str], k: int, rank: str = "mean",
                         cutoff: Optional[float] = None, include_cys: bool = False, one_per_position: bool = False,
                         min_members: Optional[int] = None) -> List[List[EnsembleHit]]:
    """Ranked hit lists of every ensemble of a ``scan_ensembles`` result, best first: ONE ``Engine.select_hits`` on the [sum(L), 20]
    table that ``rank`` names ("mean"; "worst": the largest ddG over the members, so a hit is stabilising in every conformer;
    "best": the smallest), with ld = 20. ``min_members``: entries in which fewer members take part are set to NaN in the ranked copy
    (one masked fill on the device), so they are no candidates. Only the hits and their statistics are copied back."""
    if rank not in RANKS:
        raise ValueError(f"rank={rank!r}: one of {sorted(RANKS)}")
    ranked = stats[RANKS[rank]]
    if min_members is not None:
        ranked = ranked.masked_fill(stats["count"] < int(min_members), float("nan"))
    S = np.concatenate([[_CODE.get(c, 20) for c in seq] for seq in seqs]).astype(np.int32) if seqs else np.zeros(0, np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    with torch.cuda.device(engine.device):
        res = engine.select_hits(ranked, S, offsets, k, cutoff=cutoff, include_cys=include_cys, one_per_position=one_per_position)
        counts = res["hit_count"].cpu().numpy()
        live = torch.arange(int(k), device=engine.device)[None, :] < res["hit_count"][:, None]
        pos, aa = res["hit_pos"].clamp(min=0).long(), res["hit_aa"].clamp(min=0).long()
        rows = torch.as_tensor(offsets[:-1], device=engine.device).long()[:, None] + pos
        picked = {name: stats[name][rows[live], aa[live]].cpu().numpy() for name in STAT_NAMES}
        val, pos, aa = res["hit_ddg"][live].cpu().numpy(), res["hit_pos"][live].cpu().numpy(), res["hit_aa"][live].cpu().numpy()
    out, at = [], 0
    for e, seq in enumerate(seqs):
        hits = []
        for i in range(at, at + int(counts[e])):
            p = int(pos[i])
            hits.append(EnsembleHit(p, seq[p], ALPHABET[int(aa[i])], float(val[i]), float(picked["mean"][i]), float(picked["spread"][i]),
                                    float(picked["lo"][i]), float(picked["hi"][i]), int(picked["count"][i]), int(picked["below"][i]),
                                    int(picked["lo_member"][i]), int(picked["hi_member"][i])))
        at += int(counts[e])
        out.append(hits)
    return out


def ensemble_hits(model, members: Sequence[dict], k: int, rank: str = "mean", cutoff: Optional[float] = None, include_cys: bool = False,
                  one_per_position: bool = False, min_members: Optional[int] = None) -> List[EnsembleHit]:
    """``TransferModel.ensemble_hits``: the ``k`` best substitutions of one ensemble by ``rank``. ``cutoff`` keeps hits whose ranked
    statistic is <= cutoff, and is the cutoff of ``below`` as well."""
    if rank not in RANKS:
        raise ValueError(f"rank={rank!r}: one of {sorted(RANKS)}")
    res = scan_ensembles(model, [members], cutoff=cutoff)
    return select_ensemble_hits(model.engine(), res["stats"], res["seqs"], k, rank, cutoff, include_cys, one_per_position, min_members)[0]
