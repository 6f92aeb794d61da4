"""Conformer ensembles: per-mutation ddG statistics across the members of an ensemble (NMR models, AF2 ranks, MD frames).

ThermoMPNN's table depends on the backbone, so one table answers for one conformer only. Here the members of an ensemble go through
the fused forward as what they are, a ragged packed batch (a member's table does not depend on its batch), and ONE launch reduces the
packed table across the members (Engine.ensemble_stats, csrc/tmpnn_ensemble.hip): for every (position, letter) the mean, the
population spread, the smallest and the largest ddG with the members that hold them, the number of members that take part and the
number of those at or below a cutoff. No table goes to the host. The mean is a chain of fp32 adds in ascending member order and the
spread is taken around it (include/tmpnn.h has the contract to the operation), so every bit is reproducible.

By default members must parse to the same length and to the same letter wherever both have a residue (``align_members``). With
``align=True`` members of unequal length — several PDB entries or predicted models of one protein that differ in construct
boundaries, numbering, missing termini, tags or a point substitution — are laid on one axis first: ONE ``Engine.align_global`` per
scan aligns every member to the axis (``reference`` if given, else member 0's parsed sequence) by the rule of
``datasets.global_alignment_map`` (identical columns count 1, gaps are free: the reference's ``pairwise2.align.globalxx``), the
members are featurized at their own lengths and packed ragged, and the kernel's output is, as it is, the row map the statistics read
through (``Engine.ensemble_stats(rows=)``). Only matching letters align, so a substituted residue is out at its column, and without a
``reference`` the columns where member 0 holds '-' or 'X' get no participants: pass a reference to cover them. A member whose
identity (aligned columns / its residues that carry one of the 20 letters) is below ``min_identity`` is refused.
A member's own '-', 'X' and rows with a missing backbone atom drop out of that position only. Limits: L <= 8192, 65 535
ensembles per call, the released head configuration with ``subtract_mut``, one rank. Multi-MODEL files are read by the Python parser
(``pdb_io.parse_pdb_models``) only.

``superpose=True`` says why a spread is large and refuses a member that is another conformation: ONE ``Engine.superpose`` per scan
(csrc/tmpnn_superpose.hip, two small launches before the forward, after the alignment and through its row map as it is) lays every
member on member ``fit_to`` of its ensemble by the optimal proper rotation of the C-alpha atoms both have, and gives per member the
RMSD, the number of fitted columns and the transform, per (member, column) the deviation after the fit and per column the RMSF of the
superposed members. A member whose RMSD exceeds ``max_rmsd`` is refused by name before any forward. The ddG statistics do not change.

Out of scope: substitution matrices and gap penalties, multiple-sequence alignment; in the superposition, iterating to the mean
structure, other atoms than C-alpha, weights."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import os

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
    aligned: Optional[torch.Tensor] = None      # align=True: [M, L] int32, the member's own residue index at every axis column, or -1
    identity: Optional[torch.Tensor] = None     # align=True: [M] float64, aligned columns / the member's residues with one of the 20 letters
    rmsd: Optional[torch.Tensor] = None         # superpose=True: [M] float32, C-alpha RMSD to member fit_to after the optimal fit (NaN: n_fit 0)
    n_fit: Optional[torch.Tensor] = None        # superpose=True: [M] int32, the columns valid in the member and in member fit_to
    rmsf: Optional[torch.Tensor] = None         # superpose=True: [L] float32, per column over the superposed members (NaN: none there)
    deviation: Optional[torch.Tensor] = None    # superpose=True: [M, L] float32, the distance to member fit_to's atom after the fit, or NaN
    xform: Optional[torch.Tensor] = None        # superpose=True: [M, 12] float64, R row-major then t: x' = R x + t


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
    rmsf: float = float("nan")      # superpose=True: the RMSF of the hit's position


def _check_model(model) -> None:
    if model.generic_head or not model.subtract_mut:
        raise NotImplementedError("ensemble statistics serve the released head configuration (hidden_dims [64, 32], num_final_layers 2, "
                                  "lightattn) with subtract_mut only; run ssm_table per member for other configurations")


def read_reference(reference: str) -> str:
    """``reference``: a sequence as a plain string, or the path of a FASTA file with one record -> the axis sequence (upper case,
    the 20 letters, 'X' and '-'; ValueError for anything else)."""
    text = str(reference)
    if os.path.isfile(text):
        with open(text) as fh:
            lines = [ln.strip() for ln in fh if ln.strip()]
        if sum(ln.startswith(">") for ln in lines) > 1:
            raise ValueError(f"{text}: a reference is ONE sequence, the file holds {sum(ln.startswith('>') for ln in lines)} records")
        text = "".join(ln for ln in lines if not ln.startswith(">"))
    seq = "".join(text.split()).upper()
    bad = sorted(set(seq) - set(ALPHABET) - {"-"})
    if not seq or bad:
        raise ValueError(f"reference: {'an empty sequence' if not seq else 'letters ' + ''.join(bad)} (expected the 20 letters, X or -)")
    return seq


def _letter_codes(seq: str) -> np.ndarray:
    """The letters as the alignment takes them: 0 .. 19, 'X' 20, '-' (anything else) 21: 20 and 21 match nothing."""
    return np.array([_CODE.get(c, 20 if c == "X" else 21) for c in seq], np.int32).reshape(-1)


def scan_ensembles(model, ensembles: Sequence[Sequence[dict]], cutoff: Optional[float] = None, chunk_residues: int = 1 << 18,
                   align: bool = False, reference: Optional[str] = None, min_identity: float = 0.9, superpose: bool = False,
                   fit_to: int = 0, max_rmsd: Optional[float] = None) -> dict:
    """Ensembles (each a list of parsed members) -> dict(stats: what ``Engine.ensemble_stats`` returns over ALL ensembles, rows
    ``offsets[e] .. offsets[e + 1]`` being ensemble e; seqs; names: per ensemble its members' names; members: M per ensemble).
    One ``tied_featurize`` per ensemble, ONE forward per chunk of whole members of at most ``chunk_residues`` residues (a chunk may
    end inside an ensemble: a member's table does not depend on its batch) into one packed device table, and ONE ``ensemble_stats``.
    ``align=True``: members of unequal length. Every member, member 0 included, is aligned to the ensemble's axis — ``reference`` (a
    plain string or a one-record FASTA file, the same for every ensemble) or member 0's parsed sequence — in ONE
    ``Engine.align_global`` whose output is the row map of the statistics; ``seqs`` are the axes, and the dict gains ``aligned``
    (per ensemble an int32 [M, L] device tensor: the member's own residue index at every axis column, or -1) and ``identity`` (per
    ensemble a float64 [M] array: aligned columns / the member's residues that carry one of the 20 letters). ValueError, naming the
    member and the value, for a member below ``min_identity`` (0 disables it). Only ``aligned`` counts and ``status`` come back.
    ``superpose=True``: the packed X and mask of all members go through ONE ``Engine.superpose`` before the forward (after the
    alignment, through its row map as it is): every member is laid on member ``fit_to`` of its ensemble, and the dict gains
    ``superposed``: what ``Engine.superpose`` returns over all ensembles (n_fit, rmsd, xform per member, the members in order; dev
    per map entry; rmsf, col_count per column). ValueError, naming the member and the value, for a member whose RMSD exceeds
    ``max_rmsd`` or that shares no column with member ``fit_to`` (None: no member is refused); only ``rmsd`` comes back for it."""
    _check_model(model)
    if not align and reference is not None:
        raise ValueError("reference= belongs to align=True")
    if not superpose and (fit_to != 0 or max_rmsd is not None):
        raise ValueError("fit_to= and max_rmsd= belong to superpose=True")
    if max_rmsd is not None and not max_rmsd >= 0:
        raise ValueError(f"max_rmsd={max_rmsd}: a distance, >= 0")
    device = next(model.parameters()).device
    eng = model.engine()
    seqs, names, S_stat, pieces, M_of, L_of = [], [], [], [], [], []
    axis = read_reference(reference) if reference is not None else None
    A_codes, B_codes, pair_desc, first_row = [], [], [], []
    a0 = b0 = map0 = 0
    for entries in ensembles:
        entries = list(entries)
        if superpose and not 0 <= fit_to < len(entries):
            raise ValueError(f"fit_to={fit_to}: ensemble {len(seqs)} has {len(entries)} members")
        if align:
            if not entries:
                raise ValueError("an ensemble needs at least one member")
            seq = axis if axis is not None else entries[0]["seq"]
            L = len(seq)
            for m, e in enumerate(entries):
                n_m = len(e["seq"])
                if n_m > ENS_MAX_LEN:
                    raise ValueError(f"ensemble member {m} ({e.get('name', '')}) has {n_m} residues, more than {ENS_MAX_LEN}, the forward's own bound")
                letters = _letter_codes(e["seq"])
                own = np.where(letters < 20, letters, 20).astype(np.int32)
                own[~_backbone_complete(e)] = 20
                S_stat.append(own)
                B_codes.append(letters)
                pair_desc.append((a0, L, b0, n_m, map0 + m * L, b0))          # add = the member's first table row = b0: the same packing
                first_row.append(b0)
                b0 += n_m
            A_codes.append(_letter_codes(seq))
            a0, map0 = a0 + L, map0 + len(entries) * L
        else:
            seq, S = align_members(entries)
            S_stat.append(S.reshape(-1))
        if len(seq) > ENS_MAX_LEN:
            raise ValueError(f"an ensemble of {len(seq)} residues exceeds {ENS_MAX_LEN}, the forward's own bound")
        seqs.append(seq)
        names.append([e.get("name", "") for e in entries])
        M_of.append(len(entries))
        L_of.append(len(seq))
        feats = tied_featurize(entries, device, None, None, None, None, None, None, ca_only=False)
        X, S_fwd, mask, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[5], feats[12]
        own_len = [len(e["seq"]) for e in entries]                              # (the pack pads behind a member's own rows)
        pieces.extend((X[m][:n], S_fwd[m][:n], mask[m][:n], residue_idx[m][:n], chain_enc[m][:n]) for m, n in enumerate(own_len))
    T = sum(p[0].shape[0] for p in pieces)
    with torch.cuda.device(eng.device):
        if align:                                                                # before the forward: a refusal costs one small launch
            cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int32)
            rows_out = torch.full((map0,), -1, dtype=torch.int32, device=eng.device)
            al = eng.align_global(cat(A_codes), cat(B_codes), np.array(pair_desc, np.int64).reshape(-1, 6), out=rows_out)
            counts, status = al["aligned"].cpu().numpy(), al["status"].cpu().numpy()
            if (status != 0).any():
                raise RuntimeError(f"align_global refused pair {int(np.flatnonzero(status)[0])}")
            identity, aligned, k, at = [], [], 0, 0
            first = torch.as_tensor(np.array(first_row, np.int32), device=eng.device)
            for e, (M, L) in enumerate(zip(M_of, L_of)):
                letters = np.array([max(int((B_codes[k + m] < 20).sum()), 1) for m in range(M)], np.float64)
                ident = counts[k:k + M].astype(np.float64) / letters
                for m in range(M):
                    if ident[m] < min_identity:
                        raise ValueError(f"ensemble member {m} ({names[e][m]}) aligns to the axis of ensemble {e} with identity {ident[m]:.3f}, "
                                         f"below min_identity {min_identity}: {int(counts[k + m])} of its {int(letters[m])} residues")
                block = rows_out[at:at + M * L].view(M, L)
                aligned.append(torch.where(block >= 0, block - first[k:k + M, None], block))
                identity.append(ident)
                k, at = k + M, at + M * L
        if superpose:                                                            # before the forward too: a refusal costs two small launches
            X_all = torch.cat([p[0] for p in pieces]) if pieces else torch.zeros((0, 4, 3))
            mask_all = torch.cat([p[2] for p in pieces]) if pieces else torch.zeros(0)
            sup = eng.superpose(X_all.to(device=eng.device, dtype=torch.float32), mask_all, M_of, L_of, rows=rows_out if align else None,
                                fit_to=fit_to)
            if (sup["status"] != 0).any():
                raise RuntimeError(f"superpose refused ensemble {int(torch.nonzero(sup['status'])[0])}")
            if max_rmsd is not None:
                rmsd, k = sup["rmsd"].cpu().numpy(), 0
                for e, M in enumerate(M_of):
                    for m in range(M):
                        if not rmsd[k + m] <= max_rmsd:
                            raise ValueError(f"ensemble member {m} ({names[e][m]}) lies {rmsd[k + m]:.3f} A (C-alpha RMSD) from member {fit_to} "
                                             f"({names[e][fit_to]}) of ensemble {e}, above max_rmsd {max_rmsd}")
                    k += M
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
        extra = dict(superposed=sup) if superpose else {}
        if not align:
            stats = eng.ensemble_stats(table, S_all, M_of, L_of, cutoff=cutoff)
            return dict(stats=stats, seqs=seqs, names=names, members=M_of, **extra)
        stats = eng.ensemble_stats(table, S_all, M_of, L_of, cutoff=cutoff, rows=rows_out)
    return dict(stats=stats, seqs=seqs, names=names, members=M_of, aligned=aligned, identity=identity, **extra)


def ensemble_table(model, members: Sequence[dict], cutoff: Optional[float] = None, align: bool = False, reference: Optional[str] = None,
                   min_identity: float = 0.9, superpose: bool = False, fit_to: int = 0, max_rmsd: Optional[float] = None) -> EnsembleTable:
    """``TransferModel.ensemble_table``: one ensemble -> its ``EnsembleTable`` (``align``, ``reference``, ``min_identity``,
    ``superpose``, ``fit_to``, ``max_rmsd``: ``scan_ensembles``)."""
    res = scan_ensembles(model, [members], cutoff=cutoff, align=align, reference=reference, min_identity=min_identity, superpose=superpose,
                         fit_to=fit_to, max_rmsd=max_rmsd)
    extra = dict(aligned=res["aligned"][0], identity=torch.from_numpy(res["identity"][0])) if align else {}
    if superpose:
        sup, M = res["superposed"], res["members"][0]
        extra.update(rmsd=sup["rmsd"], n_fit=sup["n_fit"], rmsf=sup["rmsf"], deviation=sup["dev"].view(M, -1), xform=sup["xform"])
    return EnsembleTable(**{name: res["stats"][name] for name in STAT_NAMES}, seq=res["seqs"][0], names=res["names"][0], **extra)


def select_ensemble_hits(engine, stats: Dict[str, torch.Tensor], seqs: Sequence[str], k: int, rank: str = "mean",
                         cutoff: Optional[float] = None, include_cys: bool = False, one_per_position: bool = False,
                         min_members: Optional[int] = None, rmsf: Optional[torch.Tensor] = None) -> List[List[EnsembleHit]]:
    """Ranked hit lists of every ensemble of a ``scan_ensembles`` result, best first: ONE ``Engine.select_hits`` on the [sum(L), 20]
    table that ``rank`` names ("mean"; "worst": the largest ddG over the members, so a hit is stabilising in every conformer;
    "best": the smallest), with ld = 20. ``min_members``: entries in which fewer members take part are set to NaN in the ranked copy
    (one masked fill on the device), so they are no candidates. ``rmsf``: the [sum(L)] RMSF of a superposed scan
    (``res["superposed"]["rmsf"]``); every hit then carries its position's. Only the hits and their statistics are copied back."""
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
        at_hit = rmsf[rows[live]].cpu().numpy() if rmsf is not None else None
        val, pos, aa = res["hit_ddg"][live].cpu().numpy(), res["hit_pos"][live].cpu().numpy(), res["hit_aa"][live].cpu().numpy()
    out, at = [], 0
    for e, seq in enumerate(seqs):
        hits = []
        for i in range(at, at + int(counts[e])):
            p = int(pos[i])
            hits.append(EnsembleHit(p, seq[p], ALPHABET[int(aa[i])], float(val[i]), float(picked["mean"][i]), float(picked["spread"][i]),
                                    float(picked["lo"][i]), float(picked["hi"][i]), int(picked["count"][i]), int(picked["below"][i]),
                                    int(picked["lo_member"][i]), int(picked["hi_member"][i]),
                                    **({} if at_hit is None else dict(rmsf=float(at_hit[i])))))
        at += int(counts[e])
        out.append(hits)
    return out


def ensemble_hits(model, members: Sequence[dict], k: int, rank: str = "mean", cutoff: Optional[float] = None, include_cys: bool = False,
                  one_per_position: bool = False, min_members: Optional[int] = None, align: bool = False, reference: Optional[str] = None,
                  min_identity: float = 0.9, superpose: bool = False, fit_to: int = 0, max_rmsd: Optional[float] = None) -> List[EnsembleHit]:
    """``TransferModel.ensemble_hits``: the ``k`` best substitutions of one ensemble by ``rank``. ``cutoff`` keeps hits whose ranked
    statistic is <= cutoff, and is the cutoff of ``below`` as well. ``align``, ``reference``, ``min_identity``: ``scan_ensembles``;
    positions and wild-type letters are then the axis'. ``superpose``, ``fit_to``, ``max_rmsd``: ``scan_ensembles``; every hit then
    carries the RMSF of its position."""
    if rank not in RANKS:
        raise ValueError(f"rank={rank!r}: one of {sorted(RANKS)}")
    res = scan_ensembles(model, [members], cutoff=cutoff, align=align, reference=reference, min_identity=min_identity, superpose=superpose,
                         fit_to=fit_to, max_rmsd=max_rmsd)
    return select_ensemble_hits(model.engine(), res["stats"], res["seqs"], k, rank, cutoff, include_cys, one_per_position, min_members,
                                rmsf=res["superposed"]["rmsf"] if superpose else None)[0]
