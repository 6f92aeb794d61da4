"""Sequence design on top of the sampler: the reference's ``tied_sample`` (protein_mpnn_utils.py:1385-1494), the PSSM terms of both
reference samplers (:1354-1367, :1472-1481) and the design dictionaries of ``tied_featurize`` (:483-526).

    from thermompnn_amd.design import ProteinMPNNDesign as ProteinMPNN, tied_featurize

``ProteinMPNNDesign`` is ``protein_mpnn_utils.ProteinMPNN`` plus ``tied_sample`` and a ``sample`` that takes the PSSM flags; both run
whole chains inside one launch (``Engine.sample_tied``, tmpnn_sample_tied). Everything else here is host-side packing."""
from __future__ import annotations

import numpy as np
import torch

from . import pdb_io
from .protein_mpnn_utils import ProteinMPNN, pack_sample_args

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"


def tied_decoding_order(order_row, tied_pos):
    """The reference's regrouping of a decoding order (:1405-1414) in O(T): walk ``order_row``; a residue not yet placed pulls in
    its whole group in the group's listed order, or itself alone -> (order [T] int64, close [T] int32), close[s] = 1 where step s
    is the last member of its group. Groups must not overlap, repeat a member or leave [0, T) (ValueError)."""
    base = [int(t) for t in np.asarray(torch.as_tensor(order_row).cpu()).reshape(-1)]
    T = len(base)
    group_of = [-1] * T
    groups = [[int(t) for t in grp] for grp in tied_pos if len(grp)]
    for g, grp in enumerate(groups):
        for t in grp:
            if not 0 <= t < T:
                raise ValueError(f"tied_pos: position {t} of group {g} lies outside [0, {T})")
            if group_of[t] == g:
                raise ValueError(f"tied_pos: position {t} is repeated in group {g}")
            if group_of[t] >= 0:
                raise ValueError(f"tied_pos: position {t} belongs to groups {group_of[t]} and {g} (groups must not overlap)")
            group_of[t] = g
    placed = [False] * T
    order, close = [], []
    for t in base:
        if placed[t]:
            continue
        members = groups[group_of[t]] if group_of[t] >= 0 else [t]
        for k in members:
            placed[k] = True
        order.extend(members)
        close.extend([0] * (len(members) - 1) + [1])
    if len(order) != T:
        raise ValueError("tied_decoding_order: order_row is not a permutation of 0..T-1")
    return torch.tensor(order, dtype=torch.int64), torch.tensor(close, dtype=torch.int32)


def pack_tied_args(randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos, omit_AA_mask, bias_by_res, tied_pos,
                   tied_beta, pssm_coef=None, pssm_bias=None, pssm_multi=None, pssm_log_odds_flag=None, pssm_log_odds_mask=None,
                   pssm_bias_flag=None):
    """Host-side packing of ``tied_sample``'s arguments for ``Engine.sample_tied`` (no device needed): ``pack_sample_args``'s dict
    with decoding_order [B,L] replaced by the regrouping of member 0's order for every member (:1405-1414), plus close [B,L] int32,
    weight [B,L] = tied_beta / len(group) (:1464), pssm_mix [B,L] = pssm_multi * pssm_coef and pssm_bias [B,L,21] (with
    pssm_bias_flag, else None; :1475), pssm_keep [B,L,21] = pssm_log_odds_mask (with pssm_log_odds_flag, else None; :1478)."""
    pk = pack_sample_args(randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos, omit_AA_mask, bias_by_res)
    dev = pk["free"].device
    B, L = pk["free"].shape
    f = lambda x: torch.as_tensor(x).to(dtype=torch.float32, device=dev)
    order, close = tied_decoding_order(pk["decoding_order"][0], tied_pos)
    size = torch.ones(L, dtype=torch.float32)
    for grp in tied_pos:
        for t in grp:
            size[int(t)] = float(len(grp))
    pk["decoding_order"] = order.to(dev)[None].repeat(B, 1)
    pk["close"] = close.to(dev)[None].repeat(B, 1)
    pk["weight"] = (f(tied_beta).reshape(L) / size.to(dev))[None].repeat(B, 1)
    pk.update(pssm_tables(B, L, dev, pssm_coef, pssm_bias, pssm_multi, pssm_log_odds_flag, pssm_log_odds_mask, pssm_bias_flag))
    return pk


def pssm_tables(B, L, dev, pssm_coef, pssm_bias, pssm_multi, pssm_log_odds_flag, pssm_log_odds_mask, pssm_bias_flag):
    """The PSSM terms of both reference samplers as the sampler's tables -> dict(pssm_mix [B,L] = pssm_multi * pssm_coef and pssm_bias
    [B,L,21] (with pssm_bias_flag, else None; :1475), pssm_keep [B,L,21] = pssm_log_odds_mask (with pssm_log_odds_flag, else None; :1478))."""
    f = lambda x: torch.as_tensor(x).to(dtype=torch.float32, device=dev)
    tabs = {"pssm_mix": None, "pssm_bias": None, "pssm_keep": None}
    if pssm_bias_flag:
        tabs["pssm_mix"] = (float(pssm_multi) * f(pssm_coef)).expand(B, L).contiguous()
        tabs["pssm_bias"] = f(pssm_bias).expand(B, L, 21).contiguous()
    if pssm_log_odds_flag:
        tabs["pssm_keep"] = f(pssm_log_odds_mask).expand(B, L, 21).contiguous()
    return tabs


class ProteinMPNNDesign(ProteinMPNN):
    """``ProteinMPNN`` with the reference's ``tied_sample`` and the PSSM flags of ``sample``."""

    def tied_sample(self, X, randn, S_true, chain_mask, chain_encoding_all, residue_idx, mask=None, temperature=1.0,
                    omit_AAs_np=None, bias_AAs_np=None, chain_M_pos=None, omit_AA_mask=None, pssm_coef=None,
                    pssm_bias=None, pssm_multi=None, pssm_log_odds_flag=None, pssm_log_odds_mask=None,
                    pssm_bias_flag=None, tied_pos=None, tied_beta=None, bias_by_res=None, generator=None, uniforms=None):
        """-> {"S" [B,L] int64, "probs" [B,L,21], "decoding_order" [B,L]} (reference :1385-1494): the positions of each group of
        ``tied_pos`` are decoded together, their logits averaged with ``tied_beta`` [L], and one letter drawn for the group; the
        decoding order is member 0's, regrouped, for every member (returned). Per-residue terms (bias_by_res, PSSM, omit_AA_mask,
        chain_M_pos, S_true at a fixed position) are the ones of a group's LAST listed member, and probs is written to every
        member of a group, fixed ones included — both as the reference does. One uniform per (member, closing residue) from
        ``torch.rand(..., generator=generator)`` or ``uniforms`` [B,L] picks the letter by inverse CDF, as ``sample``."""
        pk = self._packed("tied_sample", pack_tied_args, randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos,
                          omit_AA_mask, bias_by_res, [] if tied_pos is None else tied_pos,
                          torch.ones(X.shape[1]) if tied_beta is None else tied_beta, pssm_coef, pssm_bias, pssm_multi, pssm_log_odds_flag,
                          pssm_log_odds_mask, pssm_bias_flag)
        S, probs = self._sample_members("tied_sample", X, S_true, chain_encoding_all, residue_idx, mask, temperature, pk, generator, uniforms)
        return {"S": S, "probs": probs, "decoding_order": pk["decoding_order"]}

    def sample(self, X, randn, S_true, chain_mask, chain_encoding_all, residue_idx, mask=None, temperature=1.0,
               omit_AAs_np=None, bias_AAs_np=None, chain_M_pos=None, omit_AA_mask=None, pssm_coef=None, pssm_bias=None,
               pssm_multi=None, pssm_log_odds_flag=None, pssm_log_odds_mask=None, pssm_bias_flag=None,
               bias_by_res=None, generator=None, uniforms=None):
        """``ProteinMPNN.sample`` with ``pssm_bias_flag`` / ``pssm_log_odds_flag`` supported (:1354-1367): with a flag the members
        run through ``Engine.sample_tied`` with every group a single position, and the probs rows of positions that are not free
        are zeroed afterwards (:1376). Without the flags it is the parent's ``sample``."""
        if not (pssm_bias_flag or pssm_log_odds_flag):
            return super().sample(X, randn, S_true, chain_mask, chain_encoding_all, residue_idx, mask=mask, temperature=temperature,
                                  omit_AAs_np=omit_AAs_np, bias_AAs_np=bias_AAs_np, chain_M_pos=chain_M_pos, omit_AA_mask=omit_AA_mask,
                                  bias_by_res=bias_by_res, generator=generator, uniforms=uniforms)
        pk = self._packed("sample", pack_sample_args, randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos,
                          omit_AA_mask, bias_by_res)
        dev = pk["free"].device
        B, L = pk["free"].shape
        pk["close"], pk["weight"] = torch.ones((B, L), dtype=torch.int32, device=dev), None
        pk.update(pssm_tables(B, L, dev, pssm_coef, pssm_bias, pssm_multi, pssm_log_odds_flag, pssm_log_odds_mask, pssm_bias_flag))
        S, probs = self._sample_members("sample", X, S_true, chain_encoding_all, residue_idx, mask, temperature, pk, generator, uniforms)
        probs = probs * (pk["free"] * mask.to(dev))[:, :, None]
        return {"S": S, "probs": probs, "decoding_order": pk["decoding_order"]}


def tied_featurize(batch, device, chain_dict, fixed_position_dict=None, omit_AA_dict=None, tied_positions_dict=None,
                   pssm_dict=None, bias_by_res_dict=None, ca_only=False):
    """The reference's ``tied_featurize`` (:353-605) with the four design dictionaries (:483-526): ``pdb_io.tied_featurize`` packs
    the batch, and omit_AA_mask, tied_pos_list_of_lists_list, pssm_coef, pssm_bias, pssm_log_odds, bias_by_res_all and tied_beta of
    the 20-tuple are filled from the dictionaries. 1-based positions within a chain; a tied item maps chain letters to positions or
    to ``[positions, betas]``; tied_beta is the LAST batch member's (the reference rebuilds it per member); only designed (masked)
    chains read the per-chain dictionaries."""
    out = list(pdb_io.tied_featurize(batch, device, chain_dict, fixed_position_dict, ca_only=ca_only))
    if omit_AA_dict is None and tied_positions_dict is None and not pssm_dict and not bias_by_res_dict:
        return tuple(out)
    B, L = out[0].shape[0], out[0].shape[1]
    omit = np.zeros((B, L, len(ALPHABET)), np.int32)
    coef, pbias = np.zeros((B, L), np.float32), np.zeros((B, L, 21), np.float32)
    log_odds, by_res = np.zeros((B, L, 21), np.float32), np.zeros((B, L, 21), np.float32)
    tied_ll, tied_beta = [], np.ones(L)
    for b in batch:                                     # the reference keeps the LAST member's chain lists for every member (:382-391)
        masked, visible = chain_dict[b["name"]] if chain_dict is not None else (pdb_io._chain_letters(b), [])
    for i, b in enumerate(batch):
        name, pos, starts = b["name"], 0, {}
        for letter in list(masked) + list(visible):
            for role in [r for r, members in (("visible", visible), ("masked", masked)) if letter in members]:
                n = len(b[f"seq_chain_{letter}"])
                sl = slice(pos, pos + n)
                starts.setdefault(letter, pos)          # :517 takes the letter's first occurrence
                log_odds[i, sl] = 10000.0
                if role == "masked":
                    if omit_AA_dict is not None:
                        for positions, letters in omit_AA_dict[name][letter]:
                            rows = pos + np.asarray(positions, dtype=np.int64).reshape(-1) - 1
                            omit[i, rows[:, None], np.asarray([ALPHABET.index(a) for a in letters], dtype=np.int64)[None, :]] = 1
                    if pssm_dict and pssm_dict[name][letter]:
                        coef[i, sl] = pssm_dict[name][letter]["pssm_coef"]
                        pbias[i, sl] = pssm_dict[name][letter]["pssm_bias"]
                        log_odds[i, sl] = pssm_dict[name][letter]["pssm_log_odds"]
                    if bias_by_res_dict:
                        by_res[i, sl] = bias_by_res_dict[name][letter]
                pos += n
        tied, tied_beta = [], np.ones(L)
        if tied_positions_dict is not None and tied_positions_dict[name]:
            for item in tied_positions_dict[name]:
                one = []
                for letter, v in item.items():
                    if isinstance(v[0], list):          # [positions, betas]
                        for p, beta in zip(v[0], v[1]):
                            one.append(starts[letter] + p - 1)
                            tied_beta[starts[letter] + p - 1] = beta
                    else:
                        one.extend(starts[letter] + p - 1 for p in v)
                tied.append(one)
        tied_ll.append(tied)
    t = lambda a: torch.from_numpy(a).to(dtype=torch.float32, device=device)
    out[11], out[14] = t(omit), tied_ll
    out[15], out[16], out[17], out[18], out[19] = t(coef), t(pbias), t(log_odds), t(by_res), t(tied_beta)
    return tuple(out)
