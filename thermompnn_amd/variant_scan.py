"""ddG tables of one backbone under many sequences: the encoder runs once (Engine.encode), the decoder and the head once per
variant with the backbone's edge tiles shared between variants (Engine.decode_variants, csrc/tmpnn_variants.hip).

    python -m thermompnn_amd.variant_scan a.pdb --chain A (--variants FILE | --all-singles) --out x.npz [--synthetic_weights N]
    python -m thermompnn_amd.variant_scan a.pdb --chain A --top-pairs K [--cutoff X] [--include_cys] [--unordered] --out hits.csv
    python -m thermompnn_amd.variant_scan a.pdb --chain A --pair-map [--include_cys] [--unordered] --out map.npz
    python -m thermompnn_amd.variant_scan a.pdb --chain A --combine N --beam K [--cutoff X] [--include_cys] --out hits.csv

FILE holds one variant per line: a full one-letter sequence of the parsed length, or a comma-separated list of substitutions
such as ``A12G,K45E`` (wild type, 1-based position in the parsed sequence, new residue). Writes ``tables`` float32 [V, L, 21]
(entry [v, pos, a]: ddG of mutating position pos of variant v to ALPHABET[a], relative to the variant's own residue),
``variants`` (the V sequences) and ``wild_type``.
``--top-pairs K`` writes the K most stabilising double mutants instead, one CSV row per hit (``double_mutant_hits``): every
single-substitution background is decoded, a chunk at a time, and each chunk of tables is reduced to K keys on the device
(Engine.select_variant_hits, csrc/tmpnn_variant_hits.hip), so the [P, 20, L, 20] table of ``double_mutant_table`` never exists.
Limits of the pair selection: L <= 2048, K <= 256, one protein, one rank; the one-per-site-pair reduction is ``--pair-map``.
``--pair-map`` writes, for every site pair (p, q), its best double mutant with its letters, the most negative and the most positive
epistasis with theirs, the mean |epistasis| and the number of double mutants, as [L, L] arrays (``double_mutant_map`` / ``PairMap``):
the same chunk loop, each chunk reduced into the [L, L] state on the device (Engine.pair_map, csrc/tmpnn_pair_map.hip).
Limits of the pair map: L <= 2048, one protein, one rank; the state is five [L, L] arrays (32 bytes per site pair).
``--combine N --beam K`` writes the most stabilising mutants of 1 .. N substitutions found by a beam search of width K, one CSV row
per mutant, levels ascending (``multi_mutant_search`` / ``MultiHit``): every round decodes the beam's sequences in their own
backgrounds and one step on the device keeps the K best distinct children with their sequence rows (Engine.beam_step,
csrc/tmpnn_beam.hip); no table goes to the host and no sequence comes back.
Limits of the beam search: L <= 2048, N <= 8, K * N <= 256, one protein, one rank. Many structures in one search:
``multi_mutant_search_each`` (one encode per pack, one decode and one Engine.beam_step_each per round for all of its proteins), with
its own command line, ``python -m thermompnn_amd.combine_scan``.
Not here: the native writer, multi-GPU sharding of the variants, hipGraph capture, the training paths, ProteinMPNN.forward and
examples/."""
from __future__ import annotations

import argparse
import csv
import re
from dataclasses import dataclass
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


@dataclass
class PairHit:
    """One double mutant: ``first`` is the background substitution p:a, ``second`` the substitution q:b made on that background
    (``Mutation.ddG`` of ``first`` is table_wt[p, a]; ``second`` carries none: table_{p:a}[q, b] stays on the device, only its sum
    with the first comes back). ``ddG`` is that fp32 sum, table_wt[p, a] + table_{p:a}[q, b], which the device ranked;
    ``ddG_first`` = table_wt[p, a], ``ddG_additive`` = table_wt[p, a] + table_wt[q, b] and ``epistasis`` = ddG - ddG_additive are
    computed on the host, in double precision, from the fp32 table entries."""
    first: Mutation
    second: Mutation
    ddG: float
    ddG_first: float
    ddG_additive: float
    epistasis: float


PAIR_MAX_LEN, PAIR_MAX_K, CYS = 2048, 256, _CODE["C"]


def pair_tag(p, a):
    """The selection's tag of background p:a, p * 32 + a: 11 + 5 bits, so it fits the key's 16 tag bits up to L = 2048."""
    return p * 32 + a


def split_tag(tag):
    return tag >> 5, tag & 31


def double_mutant_hits(model, pdb, k: int, positions: Optional[Sequence[int]] = None, cutoff: Optional[float] = None,
                       include_cys: bool = False, unordered: bool = False, chunk: int = 256,
                       _tables: Optional[Callable] = None, _select: Optional[Callable] = None) -> List[PairHit]:
    """The ``k`` most stabilising double mutants (p:a, q:b) of one parsed structure, best first: the smallest
        ddG(p:a, q:b) = table_wt[p, a] + table_{p:a}[q, b]                                     (``double_mutant_table``'s entries)
    in ascending (ddG, p, a, q, b) order with -0.0 taken as +0.0, without the [P, 20, L, 20] table: the backbone is encoded ONCE,
    the wild type is decoded, then the single-substitution backgrounds ``chunk`` at a time, and every chunk of tables is reduced to
    k keys on the device while the next one reuses its memory (``Engine.select_variant_hits`` with base = table_wt[p, a],
    tag = p * 32 + a, skip = p; the k keys are carried from chunk to chunk). Never more than one chunk of tables is allocated.
    Backgrounds: every a != the wild type's letter (those are single mutants) at ``positions`` (default: every residue with one of
    the 20 letters), cysteine only with ``include_cys`` — which holds for the second substitution too. Second sites: every q != p
    with a letter, b != its letter, ddG not NaN and <= ``cutoff``. The default keeps both orders of a site pair (p:a then q:b, and
    q:b then p:a: different numbers); ``unordered`` keeps q > p only, one path per site pair. L <= 2048, 1 <= k <= 256.
    (``_tables(S [V, L]) -> [V, L, 21]`` and ``_select(ddg, S_var, base, tag, k, skip=, cutoff=, include_cys=, upper=, state=)``:
    the table function and the selection, defaults the model's and its engine's.)"""
    entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
    seq = entry["seq"]
    L, wt_idx = len(seq), sequence_indices(seq)
    if not 1 <= int(k) <= PAIR_MAX_K:
        raise ValueError(f"double_mutant_hits: k={k} outside [1, {PAIR_MAX_K}]")
    if L > PAIR_MAX_LEN:
        raise ValueError(f"double_mutant_hits: {L} residues exceed {PAIR_MAX_LEN} (the selection's key holds 11 position bits)")
    if int(chunk) < 1:
        raise ValueError(f"double_mutant_hits: chunk={chunk}")
    if positions is None:
        positions = [p for p in range(L) if wt_idx[p] < 20]
    positions = sorted({int(p) for p in positions})
    for p in positions:
        if not 0 <= p < L or wt_idx[p] >= 20:
            raise ValueError(f"position {p}: outside the sequence or a residue without one of the 20 letters")
    if _tables is None:
        enc = model._encode_structure(entry)                           # the only encoder run
        _tables = lambda s: model._tables_over(enc, s)
    if _select is None:
        _select = model.engine().select_variant_hits
    pairs = [(p, a) for p in positions for a in range(20) if a != wt_idx[p] and (include_cys or a != CYS)]
    wt = _tables(wt_idx[None])[0]                                      # [L, 21]
    if not pairs:
        return []
    pos_of, aa_of = (np.array(x, dtype=np.int64) for x in zip(*pairs))
    res = state = None
    for v0 in range(0, len(pairs), int(chunk)):
        p_c, a_c = pos_of[v0:v0 + int(chunk)], aa_of[v0:v0 + int(chunk)]
        S = np.tile(wt_idx, (len(p_c), 1))
        S[np.arange(len(p_c)), p_c] = a_c
        t = _tables(S)                                                 # [n, L, 21]: the previous chunk's tables are free by now
        base = wt[torch.as_tensor(p_c, device=wt.device), torch.as_tensor(a_c, device=wt.device)]
        res = _select(t, S, base, pair_tag(p_c, a_c), int(k), skip=p_c, cutoff=cutoff, include_cys=include_cys, upper=unordered,
                      state=state)
        state = res["state"]
        del t
    n = int(res["hit_count"][0])
    val, tag, q_h, b_h = (np.asarray(res[key][:n].cpu()) for key in ("hit_ddg", "hit_tag", "hit_pos", "hit_aa"))
    table = np.asarray(wt.cpu(), dtype=np.float32)
    name = entry.get("name", "")
    hits = []
    for v, tg, q, b in zip(val, tag, q_h, b_h):
        p, a = (int(x) for x in split_tag(int(tg)))
        q, b = int(q), int(b)
        first, add = float(table[p, a]), float(table[p, a]) + float(table[q, b])
        hits.append(PairHit(Mutation(p, seq[p], ALPHABET[a], first, name), Mutation(q, seq[q], ALPHABET[b], None, name),
                            float(v), first, add, float(v) - add))
    return hits


PAIR_CSV_HEADER = ["rank", "first", "second", "ddG", "ddG_first", "ddG_additive", "epistasis"]


def write_pair_hits_csv(path: str, hits: Sequence[PairHit]) -> int:
    """One row per hit, best first: rank (0-based), the two substitutions in the variant file's notation (``A12G``: wild type,
    1-based position, new residue), then ddG, ddG_first, ddG_additive and epistasis as ``repr`` of the Python floats."""
    sub = lambda m: f"{m.wildtype}{m.position + 1}{m.mutation}"
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(PAIR_CSV_HEADER)
        for r, h in enumerate(hits):
            w.writerow([r, sub(h.first), sub(h.second), repr(h.ddG), repr(h.ddG_first), repr(h.ddG_additive), repr(h.epistasis)])
    return len(hits)


@dataclass
class PairMap:
    """Every site pair's best double mutant and its coupling, [R, L] numpy arrays on the host: row r is the first site
    ``positions[r]`` (p), column q the second site. With ddG(p:a, q:b) = table_wt[p, a] + table_{p:a}[q, b] and the epistasis
    e = table_{p:a}[q, b] - table_wt[q, b] (what q:b does on the background p:a, less what it does on the wild type; both fp32):
    ``best_ddG`` the smallest ddG of the pair and ``best_a`` / ``best_b`` its letters (ALPHABET indices; ties: the smallest (a, b));
    ``eps_min`` / ``eps_max`` the most negative and the most positive e with their letters; ``eps_abs_mean`` the mean |e| over the
    pair's ``count`` double mutants — near zero: an additive pair. NaN and -1 where a pair has no double mutant (q = p, a '-' or 'X'
    residue, q < p with ``unordered``). ``wt`` is the wild type's table [L, 21], ``seq`` the parsed sequence."""
    positions: np.ndarray
    best_ddG: np.ndarray
    best_a: np.ndarray
    best_b: np.ndarray
    eps_min: np.ndarray
    eps_min_a: np.ndarray
    eps_min_b: np.ndarray
    eps_max: np.ndarray
    eps_max_a: np.ndarray
    eps_max_b: np.ndarray
    eps_abs_mean: np.ndarray
    count: np.ndarray
    wt: np.ndarray
    seq: str

    ARRAYS = ("positions", "best_ddG", "best_a", "best_b", "eps_min", "eps_min_a", "eps_min_b", "eps_max", "eps_max_a", "eps_max_b",
              "eps_abs_mean", "count", "wt")


def double_mutant_map(model, pdb, positions: Optional[Sequence[int]] = None, include_cys: bool = False, unordered: bool = False,
                      chunk: int = 256, _tables: Optional[Callable] = None, _reduce: Optional[Callable] = None) -> PairMap:
    """For EVERY site pair (p, q) of one parsed structure its best double mutant, the extremes of its epistasis and the mean size of
    it (``PairMap``), without the [P, 20, L, 20] table: ``double_mutant_hits``' loop — the backbone is encoded ONCE, the wild type is
    decoded, then the single-substitution backgrounds ``chunk`` at a time in ascending (p, a) order — with every chunk of tables
    reduced on the device into an [R, L] state (``Engine.pair_map`` with base = table_wt[p, a], row = the index of p in
    ``positions``, letter = a, skip = p; the state is carried from chunk to chunk and its bits do not depend on ``chunk``). Never
    more than one chunk of tables plus the state is allocated. Backgrounds and second substitutions as in ``double_mutant_hits``:
    every a != the wild type's letter at ``positions`` (sorted; default: every residue with one of the 20 letters), every q != p
    with a letter (``unordered``: q > p only), b != its letter, cysteine on either side only with ``include_cys``. L <= 2048.
    (``_tables(S [V, L]) -> [V, L, 21]`` and ``_reduce(ddg, S_var, base, row, letter, wt, R, skip=, include_cys=, upper=, state=)``:
    the table function and the reduction, defaults the model's and its engine's.)"""
    from .engine import decode_pair_map
    entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
    seq = entry["seq"]
    L, wt_idx = len(seq), sequence_indices(seq)
    if L > PAIR_MAX_LEN:
        raise ValueError(f"double_mutant_map: {L} residues exceed {PAIR_MAX_LEN}")
    if int(chunk) < 1:
        raise ValueError(f"double_mutant_map: chunk={chunk}")
    if positions is None:
        positions = [p for p in range(L) if wt_idx[p] < 20]
    positions = sorted({int(p) for p in positions})
    for p in positions:
        if not 0 <= p < L or wt_idx[p] >= 20:
            raise ValueError(f"position {p}: outside the sequence or a residue without one of the 20 letters")
    if _tables is None:
        enc = model._encode_structure(entry)                           # the only encoder run
        _tables = lambda s: model._tables_over(enc, s)
    if _reduce is None:
        _reduce = model.engine().pair_map
    R = len(positions)
    pairs = [(r, p, a) for r, p in enumerate(positions) for a in range(20) if a != wt_idx[p] and (include_cys or a != CYS)]
    wt = _tables(wt_idx[None])[0]                                      # [L, 21]
    row_of, pos_of, aa_of = (np.array(x, dtype=np.int64) for x in zip(*pairs)) if pairs else (np.zeros(0, np.int64),) * 3
    state = None
    for v0 in range(0, max(len(pairs), 1), int(chunk)):                # (no background: one empty call makes the empty state)
        r_c, p_c, a_c = row_of[v0:v0 + int(chunk)], pos_of[v0:v0 + int(chunk)], aa_of[v0:v0 + int(chunk)]
        S = np.tile(wt_idx, (len(p_c), 1))
        S[np.arange(len(p_c)), p_c] = a_c
        t = _tables(S) if len(p_c) else wt.new_zeros((0, L, wt.shape[1]))   # [n, L, 21]: the previous chunk's tables are free by now
        base = wt[torch.as_tensor(p_c, device=wt.device), torch.as_tensor(a_c, device=wt.device)]
        state = _reduce(t, S, base, r_c, a_c, wt, R, skip=p_c, include_cys=include_cys, upper=unordered, state=state)
        del t
    dec = decode_pair_map(state)
    host = {k: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in dec.items()}
    return PairMap(positions=np.array(positions, dtype=np.int64), wt=np.asarray(wt.cpu(), dtype=np.float32), seq=seq, **host)


def write_pair_map_npz(path: str, m: PairMap) -> None:
    """``PairMap``'s arrays under their own names, plus ``seq``."""
    with open(path, "wb") as fh:
        np.savez(fh, seq=np.array(m.seq), **{name: getattr(m, name) for name in PairMap.ARRAYS})


@dataclass
class MultiHit:
    """One n-point mutant found by ``multi_mutant_search``: ``mutations`` its substitutions, a tuple of ``Mutation`` ascending by
    position (``Mutation.ddG``: the wild-type table's entry, what the substitution does alone). ``ddG`` is the fp32 sum of the steps'
    ddG along the best path found, each step decoded in its own background, which the device ranked; ``ddG_additive`` the sum of the
    wild-type table's entries and ``epistasis`` = ddG - ddG_additive are computed on the host, in double precision, from the fp32
    numbers. ``parent``: the rank, in the level below, of the member this one was made from (level 1: 0, the wild type)."""
    mutations: tuple
    ddG: float
    ddG_additive: float
    epistasis: float
    parent: int


BEAM_MAX_ORDER, BEAM_MAX_KD = 8, 256


def multi_mutant_search(model, pdb, order: int, beam: int, positions: Optional[Sequence[int]] = None, cutoff: Optional[float] = None,
                        include_cys: bool = False, _tables: Optional[Callable] = None, _step: Optional[Callable] = None) -> List[List[MultiHit]]:
    """A beam search for the most stabilising mutants of 1 .. ``order`` substitutions of one parsed structure -> one list of
    ``MultiHit`` per level, best first, at most ``beam`` each.
    What the number is: a mutant's ddG is the SUM OF THE STEPS' ddG ALONG THE BEST PATH FOUND, each step decoded in its own
    background: level d's members are decoded as they are (the backbone is encoded ONCE; every round is one decode of the beam's
    sequences plus one ``Engine.beam_step``), and a child's value is its parent's value plus the parent's table entry [q, b], one
    fp32 add. It is not a sum of single-mutant numbers; ``ddG_additive`` is that sum, and ``epistasis`` the difference.
    What the search covers: level 1 is exhaustive. A higher level is exhaustive only when the level below held EVERY candidate
    (its list is shorter than ``beam``); otherwise it holds the best children of the ``beam`` members kept, and a mutant whose every
    sub-mutant fell out of the beam is never seen.
    Paths: a set of substitutions can be reached from each of its sub-mutants in the beam, in a different order and with a different
    sum. All orders whose parent is in the beam are considered and the SMALLEST sum is kept (for a pair: p:a then q:b, and q:b then
    p:a); ties go to the better-ranked parent.
    Candidates: every position in ``positions`` (default: every residue with one of the 20 letters) that the member has not mutated,
    every letter but the member's own, cysteine only with ``include_cys``, a sum that is not NaN and <= ``cutoff``. The tables and the
    beam stay on the device between rounds; the host reads one count per round and the lists at the end.
    ValueError: order outside [1, 8], beam < 1, beam * order > 256, more than 2048 residues, a position outside the sequence or
    without one of the 20 letters.
    (``_tables(S [V, L]) -> [V, L, 21]`` and ``_step(ddg, S_var, score, muts, depth, k, allowed=, cutoff=, include_cys=)``: the table
    function and the step, defaults the model's and its engine's.)"""
    entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
    seq = entry["seq"]
    L, wt_idx = len(seq), sequence_indices(seq)
    order, beam = int(order), int(beam)
    if not 1 <= order <= BEAM_MAX_ORDER:
        raise ValueError(f"multi_mutant_search: order={order} outside [1, {BEAM_MAX_ORDER}]")
    if beam < 1 or beam * order > BEAM_MAX_KD:
        raise ValueError(f"multi_mutant_search: beam={beam} at order {order}: beam must be at least 1 and beam * order at most {BEAM_MAX_KD}")
    if L > PAIR_MAX_LEN:
        raise ValueError(f"multi_mutant_search: {L} residues exceed {PAIR_MAX_LEN} (the step's key holds 11 position bits)")
    allowed = None
    if positions is not None:
        allowed = np.zeros(L, dtype=np.int32)
        for p in positions:
            if not 0 <= int(p) < L or wt_idx[int(p)] >= 20:
                raise ValueError(f"position {p}: outside the sequence or a residue without one of the 20 letters")
            allowed[int(p)] = 1
    if _tables is None:
        enc = model._encode_structure(entry)                           # the only encoder run
        _tables = lambda s: model._tables_over(enc, s)
    if _step is None:
        _step = model.engine().beam_step
    S, score, muts, wt, rounds = wt_idx[None], np.zeros(1, dtype=np.float32), None, None, []
    for d in range(1, order + 1):
        t = _tables(S)                                                 # [V, L, 21]: the previous round's tables are free by now
        if d == 1:
            wt = t[0]
        res = _step(t, S, score, muts, d, beam, allowed=allowed, cutoff=cutoff, include_cys=include_cys)
        del t
        n = int(res["out_count"][0])                                   # the round's one read on the host
        if n == 0:
            break
        S, score, muts = res["out_S"][:n], res["out_score"][:n], res["out_muts"][:n]
        rounds.append((res["out_muts"][:n], res["out_score"][:n], res["out_parent"][:n]))
    table = np.asarray(wt.cpu(), dtype=np.float32)
    name = entry.get("name", "")
    levels = [_multi_hits(table, seq, name, *(np.asarray(x.cpu()) for x in rnd)) for rnd in rounds]
    return levels + [[] for _ in range(order - len(levels))]


def _multi_hits(table: np.ndarray, seq: str, name: str, m_h, s_h, p_h) -> List[MultiHit]:
    """One level's rows on the host (substitution words [n, d], fp32 sums [n], parents [n]) -> its ``MultiHit``s; ``table`` is the
    wild type's [L, 21]."""
    hits = []
    for row, val, par in zip(m_h, s_h, p_h):
        subs = [(int(e) >> 5, int(e) & 31) for e in row]
        add = sum(float(table[q, b]) for q, b in subs)
        hits.append(MultiHit(tuple(Mutation(q, seq[q], ALPHABET[b], float(table[q, b]), name) for q, b in subs), float(val), add,
                             float(val) - add, int(par)))
    return hits


def multi_mutant_search_each(model, pdbs, order: int, beam: int, positions: Optional[Sequence[Optional[Sequence[int]]]] = None,
                             cutoff: Optional[float] = None, include_cys: bool = False, pack_residues: int = 16384,
                             _tables: Optional[Callable] = None, _step: Optional[Callable] = None) -> List[List[List[MultiHit]]]:
    """``multi_mutant_search`` for many parsed structures in one call -> one list of levels per structure, each equal to what
    ``multi_mutant_search`` returns for that structure alone: the same sets, parents and score bits (the step's contract is per
    protein and the forward's tables do not depend on the batch).
    ``pdbs``: parsed structures (an entry, or ``alt_parse_PDB``'s one-entry list, each). ``positions``: None, or one list (or None)
    per structure, local positions. The structures are grouped in argument order into packs of at most ``pack_residues`` residues
    (``design_scan.pack_batches``; a longer structure gets a pack of its own). Per pack the backbones are encoded ONCE, together;
    round d is ONE decode of the ``beam`` rows (round 1: one row, the wild types) — row v holds beam slot v of every protein — and ONE
    ``Engine.beam_step_each``, whose outputs are the next round's rows, scores and substitutions as they stand. The host reads the
    pack's counts once per round, stops when no protein has a child left, and builds the lists at the end as
    ``multi_mutant_search`` does. A protein whose beam dies keeps empty levels while the others go on.
    ValueError, naming the structure: as ``multi_mutant_search``; and a ``positions`` list of another length than ``pdbs``.
    (``_tables(S [V, T], offsets [P + 1]) -> [V, T, 21]`` over a pack and ``_step(ddg, S_var, score, muts, offsets, depth, k,
    allowed=, cutoff=, include_cys=, max_len=)``: the table function and the step, defaults the model's and its engine's.)"""
    from .design_scan import pack_batches
    entries = [p[0] if isinstance(p, (list, tuple)) else p for p in pdbs]
    order, beam = int(order), int(beam)
    if not 1 <= order <= BEAM_MAX_ORDER:
        raise ValueError(f"multi_mutant_search_each: order={order} outside [1, {BEAM_MAX_ORDER}]")
    if beam < 1 or beam * order > BEAM_MAX_KD:
        raise ValueError(f"multi_mutant_search_each: beam={beam} at order {order}: beam must be at least 1 and beam * order at most "
                         f"{BEAM_MAX_KD}")
    if positions is not None and len(positions) != len(entries):
        raise ValueError(f"multi_mutant_search_each: positions has {len(positions)} lists for {len(entries)} structures")
    if int(pack_residues) < 1:
        raise ValueError(f"multi_mutant_search_each: pack_residues={pack_residues}")
    label = lambda i: f"structure {i} ({entries[i].get('name', '')})"
    wt_idx = [sequence_indices(e["seq"]) for e in entries]
    allowed = [None] * len(entries)
    for i, e in enumerate(entries):
        L = len(e["seq"])
        if L > PAIR_MAX_LEN:
            raise ValueError(f"multi_mutant_search_each: {label(i)}: {L} residues exceed {PAIR_MAX_LEN} (the step's key holds 11 position bits)")
        if positions is not None and positions[i] is not None:
            allowed[i] = np.zeros(L, dtype=np.int32)
            for p in positions[i]:
                if not 0 <= int(p) < L or wt_idx[i][int(p)] >= 20:
                    raise ValueError(f"{label(i)}: position {p}: outside the sequence or a residue without one of the 20 letters")
                allowed[i][int(p)] = 1
    results: List[Optional[List[List[MultiHit]]]] = [None] * len(entries)
    for pack in pack_batches([len(e["seq"]) for e in entries], int(pack_residues)):
        lens = [len(entries[i]["seq"]) for i in pack]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        P, T = len(pack), int(offsets[-1])
        al = None
        if any(allowed[i] is not None for i in pack):
            al = np.concatenate([np.ones(n, np.int32) if allowed[i] is None else allowed[i] for i, n in zip(pack, lens)])
        if _tables is None:
            enc = model._encode_structures([entries[i] for i in pack])     # the pack's only encoder run
            tables = lambda s, _o, enc=enc: model._tables_over(enc, s)
        else:
            tables = _tables
        step = model.engine().beam_step_each if _step is None else _step
        S = np.concatenate([wt_idx[i] for i in pack])[None] if pack else np.zeros((1, 0), np.int64)
        score, muts, wt, rounds = np.zeros((P, 1), dtype=np.float32), None, None, []
        for d in range(1, order + 1):
            t = tables(S, offsets)                                         # [V, T, 21]: the previous round's tables are free by now
            if d == 1:
                wt = t[0]
            res = step(t, S, score, muts, offsets, d, beam, allowed=al, cutoff=cutoff, include_cys=include_cys, max_len=max(lens))
            del t
            counts = np.asarray(res["out_count"].cpu()).reshape(P)         # the round's one read on the host
            if (counts <= 0).all():
                break
            S, score, muts = res["out_S"], res["out_score"], res["out_muts"]
            rounds.append((counts, res["out_muts"], res["out_score"], res["out_parent"]))
        table = np.asarray(wt.cpu(), dtype=np.float32)
        host = [(c, *(np.asarray(x.cpu()) for x in rest)) for c, *rest in rounds]
        for j, i in enumerate(pack):
            own, seq, name = table[offsets[j]:offsets[j + 1]], entries[i]["seq"], entries[i].get("name", "")
            levels = [_multi_hits(own, seq, name, m[j, :c[j]], s[j, :c[j]], p[j, :c[j]]) if c[j] > 0 else [] for c, m, s, p in host]
            results[i] = levels + [[] for _ in range(order - len(levels))]
    return results


MULTI_CSV_HEADER = ["order", "rank", "mutations", "ddG", "ddG_additive", "epistasis"]


def write_multi_hits_csv(path: str, levels: Sequence[Sequence[MultiHit]]) -> int:
    """One row per mutant, levels ascending and best first within a level: order (the number of substitutions), rank (0-based within
    the level), the substitutions in the variant file's notation joined by ':' (``A12G:K45E``: wild type, 1-based position, new
    residue, ascending by position), then ddG, ddG_additive and epistasis as ``repr`` of the Python floats."""
    sub = lambda m: f"{m.wildtype}{m.position + 1}{m.mutation}"
    rows = 0
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(MULTI_CSV_HEADER)
        for d, hits in enumerate(levels, 1):
            for r, h in enumerate(hits):
                w.writerow([d, r, ":".join(sub(m) for m in h.mutations), repr(h.ddG), repr(h.ddG_additive), repr(h.epistasis)])
                rows += 1
    return rows


def main(argv=None, _tables: Optional[Callable] = None, _select: Optional[Callable] = None, _reduce: Optional[Callable] = None,
         _step: Optional[Callable] = None):
    """(``_tables`` / ``_select`` / ``_reduce`` / ``_step``: the hooks of ``double_mutant_hits`` for --top-pairs, of
    ``double_mutant_map`` for --pair-map and of ``multi_mutant_search`` for --combine; with ``_tables`` no model is loaded.)"""
    from .custom_inference import load_model
    from .pdb_io import alt_parse_PDB
    ap = argparse.ArgumentParser(description="ThermoMPNN ddG tables of one backbone under many sequence variants on MI355X")
    ap.add_argument("pdb")
    ap.add_argument("--chain", default="A")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--variants", help="file with one variant per line: a full sequence or a list like A12G,K45E")
    src.add_argument("--all-singles", action="store_true", help="every single-substitution background (19 per residue)")
    src.add_argument("--top-pairs", type=int, default=None, metavar="K",
                     help="the K most stabilising double mutants, selected on the GPU, as a CSV (1 <= K <= 256)")
    src.add_argument("--pair-map", action="store_true",
                     help="every site pair's best double mutant and epistasis, reduced on the GPU, as an .npz of [L, L] maps")
    src.add_argument("--combine", type=int, default=None, metavar="N",
                     help="beam search for the most stabilising mutants of 1 .. N substitutions, on the GPU, as a CSV (needs --beam)")
    ap.add_argument("--beam", type=int, default=None, metavar="K", help="--combine: mutants kept per level (K * N <= 256)")
    ap.add_argument("--out", required=True, help="output .npz (--top-pairs, --combine: .csv)")
    ap.add_argument("--cutoff", type=float, default=None, help="--top-pairs, --combine: keep mutants with ddG <= cutoff")
    ap.add_argument("--include_cys", action="store_true", help="--top-pairs, --pair-map, --combine: substitutions to cysteine take part")
    ap.add_argument("--unordered", action="store_true",
                    help="--top-pairs, --pair-map: one path per site pair (second site behind the first)")
    ap.add_argument("--model_path", default="")
    ap.add_argument("--thermompnn_dir", default=".")
    ap.add_argument("--synthetic_weights", type=int, default=None)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--chunk", type=int, default=256, help="variants decoded per call")
    a = ap.parse_args(argv)
    if a.top_pairs is None and a.combine is None and a.cutoff is not None:
        ap.error("--cutoff belongs to --top-pairs and --combine")
    if a.top_pairs is None and not a.pair_map and (a.unordered or (a.include_cys and a.combine is None)):
        ap.error("--include_cys and --unordered belong to --top-pairs and --pair-map (--include_cys to --combine too)")
    if (a.combine is None) != (a.beam is None):
        ap.error("--combine N and --beam K go together")
    if a.combine is not None and not 1 <= a.combine <= BEAM_MAX_ORDER:
        ap.error(f"--combine {a.combine}: outside [1, {BEAM_MAX_ORDER}]")
    if a.combine is not None and (a.beam < 1 or a.beam * a.combine > BEAM_MAX_KD):
        ap.error(f"--beam {a.beam}: at least 1, and --beam times --combine at most {BEAM_MAX_KD}")
    if a.combine is not None and a.out.endswith(".npz"):
        ap.error("--combine writes a CSV, not an .npz")
    if a.top_pairs is not None and not 1 <= a.top_pairs <= PAIR_MAX_K:
        ap.error(f"--top-pairs {a.top_pairs}: outside [1, {PAIR_MAX_K}]")
    if a.top_pairs is not None and a.out.endswith(".npz"):
        ap.error("--top-pairs writes a CSV, not an .npz")
    model = None if _tables is not None else load_model(a.model_path or None, a.thermompnn_dir, a.synthetic_weights, precision=a.precision)
    pdb = alt_parse_PDB(a.pdb, a.chain)
    seq = pdb[0]["seq"]
    if a.top_pairs is not None:
        with torch.no_grad():
            hits = double_mutant_hits(model, pdb, a.top_pairs, cutoff=a.cutoff, include_cys=a.include_cys, unordered=a.unordered,
                                      chunk=a.chunk, _tables=_tables, _select=_select)
        write_pair_hits_csv(a.out, hits)
        print(f"{len(hits)} double mutants of {len(seq)} residues -> {a.out}")
        return 0
    if a.combine is not None:
        with torch.no_grad():
            levels = multi_mutant_search(model, pdb, a.combine, a.beam, cutoff=a.cutoff, include_cys=a.include_cys, _tables=_tables,
                                         _step=_step)
        rows = write_multi_hits_csv(a.out, levels)
        print(f"{rows} mutants of 1 .. {a.combine} substitutions of {len(seq)} residues -> {a.out}")
        return 0
    if a.pair_map:
        with torch.no_grad():
            m = double_mutant_map(model, pdb, include_cys=a.include_cys, unordered=a.unordered, chunk=a.chunk, _tables=_tables,
                                  _reduce=_reduce)
        write_pair_map_npz(a.out, m)
        print(f"{int((m.count > 0).sum())} site pairs of {len(seq)} residues, {int(m.count.sum())} double mutants -> {a.out}")
        return 0
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
