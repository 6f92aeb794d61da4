"""Drop-in counterpart of /root/reference/transfer_model.py: get_protein_mpnn + TransferModel.

``model(pdb, mutations)`` keeps the reference contract (transfer_model.py:75-121): a list aligned with
``mutations`` holding ``{"ddG": Tensor[1]}`` (on the model's device) or ``None``, and ``None`` as the
second return value. Internally ONE fused forward produces the whole [L, 21] ddG table.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import weights as _weights
from .datasets import ALPHABET
from .pdb_io import tied_featurize
from .protein_mpnn_utils import ProteinMPNN, _EngineOwner, _register_tree

_AA_INDEX = {a: i for i, a in enumerate(ALPHABET)}
HIDDEN_DIM = 128
EMBED_DIM = 128
VOCAB_DIM = 21


def _cfg_get(node, key, default=None):
    try:
        return node[key] if key in node else default
    except TypeError:
        return getattr(node, key, default)


def get_protein_mpnn(cfg, version="v_48_020.pt"):
    """Load vanilla ProteinMPNN weights (transfer_model.py:17-37): ``{thermompnn_dir}/vanilla_model_weights/{version}``
    holding ``num_edges`` and ``model_state_dict``."""
    path = os.path.join(cfg.platform.thermompnn_dir, "vanilla_model_weights", version)
    num_edges, sd = _weights.load_vanilla_checkpoint(path)
    model = ProteinMPNN(ca_only=False, num_letters=21, node_features=HIDDEN_DIM, edge_features=HIDDEN_DIM,
                        hidden_dim=HIDDEN_DIM, num_encoder_layers=3, num_decoder_layers=3, k_neighbors=num_edges,
                        augment_eps=0.0)
    if cfg.model.load_pretrained:
        model.load_state_dict(sd)
    if cfg.model.freeze_weights:
        model.eval()
        for p in model.parameters():
            p.requires_grad = False
    return model


class TransferModel(_EngineOwner):
    # Opt-in gradient path (thermompnn_amd/autograd.py): with differentiable = True, grad mode on and some parameter requiring grad,
    # forward returns ddG values that carry a graph to the parameters, computed on the exact fp32 training kernels whatever
    # `precision` says, with dropout where prot_mpnn / light_attention are in training mode. Otherwise forward is the inference path.
    differentiable = False

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.hidden_dims = list(cfg.model.hidden_dims)
        self.subtract_mut = cfg.model.subtract_mut
        self.num_final_layers = cfg.model.num_final_layers
        self.lightattn = _cfg_get(cfg.model, "lightattn", False)
        if "decoding_order" not in self.cfg:                      # the reference writes this back (:50-51)
            self.cfg.decoding_order = "left-to-right"
        if not 0 <= int(self.num_final_layers) <= 3:
            raise ValueError(f"num_final_layers={self.num_final_layers}: ProteinMPNN has 3 decoder states (transfer_model.py:84-85)")
        # the released configuration (config.yaml:15-21) runs the specialised fused head; any other one the reference
        # constructor accepts (:45-73) runs the generic head kernels (tmpnn_ddg_head_generic) behind the same forward
        self.generic_head = self.hidden_dims != [64, 32] or int(self.num_final_layers) != 2 or not self.lightattn
        self._engine_kwargs = {"with_head": False} if self.generic_head else {}   # generic head: the handle holds the 118 ProteinMPNN tensors
        self.prot_mpnn = get_protein_mpnn(cfg)
        self.k_neighbors = self.prot_mpnn.k_neighbors
        _register_tree(self, _weights.head_param_shapes(self.hidden_dims, int(self.num_final_layers), bool(self.lightattn)))
        with torch.no_grad():                                      # nn.Linear(1, 1)-like non-degenerate default
            self.ddg_out.weight.fill_(1.0)

    def _state_for_engine(self):
        sd = self.state_dict()
        return {k: v for k, v in sd.items() if k.startswith("prot_mpnn.")} if self.generic_head else dict(sd)

    def _generic_tables(self, eng, hidden, S):
        """(ddG table [L,21], z [L,21]) through tmpnn_ddg_head_generic for a non-default head configuration."""
        n = int(self.num_final_layers)
        layers = [getattr(self.both_out, str(2 * i + 1)) for i in range(len(self.hidden_dims) + 1)]
        conv = self.light_attention.feature_convolution if self.lightattn else None
        return eng.ddg_head_generic([hidden[2 - k] for k in range(n)], S, self.prot_mpnn.W_s.weight, [l.weight for l in layers],
                                    [l.bias for l in layers], self.ddg_out.weight, self.ddg_out.bias,
                                    conv_w=None if conv is None else conv.weight, conv_b=None if conv is None else conv.bias,
                                    want_z=True)

    def ssm_table(self, pdb) -> torch.Tensor:
        """The whole site-saturation table of one parsed structure in ONE forward: [L, 21] on the model's device, entry
        [pos, a] = what ``forward(pdb, [Mutation(pos, seq[pos], ALPHABET[a])])`` returns as ddG (the batched form of the
        per-mutation loop of analysis/SSM.py:105-126; ``subtract_mut=False`` models return the un-subtracted head output)."""
        device = next(self.parameters()).device
        feats = tied_featurize([pdb[0] if isinstance(pdb, (list, tuple)) else pdb], device, None, None, None, None, None, None, ca_only=False)
        X, S, mask, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[5], feats[12]
        eng = self.engine()
        L = X.shape[1]
        with torch.cuda.device(eng.device):
            std = self.subtract_mut and not self.generic_head
            res = eng.ssm_forward(X[0], S[0], mask[0], residue_idx[0], chain_enc[0], torch.tensor([0, L], dtype=torch.int32),
                                  max_len=L, want_hidden=not std, want_ddg=not self.generic_head)
            if std:
                return res["ddg"]
            if self.generic_head:
                ddg, z = self._generic_tables(eng, res["hidden"], S[0])
            else:
                ddg, z = res["ddg"], eng.ddg_head(res["hidden"][2], res["hidden"][1], S[0], want_z=True)[1]
            return ddg if self.subtract_mut else z * self.ddg_out.weight.view(()) + self.ddg_out.bias.view(())

    def hit_list(self, pdb, k: int, cutoff=None, include_cys: bool = False, one_per_position: bool = False):
        """The ``k`` most stabilising substitutions of one parsed structure, best first, as ``Mutation(position, wildtype, mutation,
        ddG, pdb)`` (ddG a Python float): ONE fused forward (``ssm_table``) and ONE selection on the device
        (``Engine.select_hits``); only the hits are copied back. Positions without a residue ('-') and 'X' have no candidates;
        ``cutoff`` keeps substitutions with ddG <= cutoff; cysteine only with ``include_cys``; ``one_per_position`` keeps each
        position's best substitution first (retrieve_best_mutants, analysis/SSM.py:32-42)."""
        from .datasets import Mutation
        entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
        seq = entry["seq"]
        table = self.ssm_table(pdb)
        eng = self.engine()
        S = torch.tensor([_AA_INDEX[c] if c in _AA_INDEX and c != "X" else 20 for c in seq], dtype=torch.int32)
        with torch.cuda.device(eng.device):
            res = eng.select_hits(table, S, torch.tensor([0, len(seq)], dtype=torch.int32), k, cutoff=cutoff, include_cys=include_cys,
                                  one_per_position=one_per_position)
            n = int(res["hit_count"][0])
            val, pos, aa = res["hit_ddg"][0, :n].cpu().numpy(), res["hit_pos"][0, :n].cpu().numpy(), res["hit_aa"][0, :n].cpu().numpy()
        name = entry.get("name", "")
        return [Mutation(int(p), seq[int(p)], ALPHABET[int(a)], float(v), name) for v, p, a in zip(val, pos, aa)]

    def variant_tables(self, pdb, variants) -> torch.Tensor:
        """``ssm_table`` of the same backbone under V other sequences, [V, L, 21] on the model's device: the encoder runs once, the
        decoder and the head once per variant (Engine.encode + Engine.decode_variants). A variant is a full one-letter sequence of
        length L, a list of ``Mutation`` applied to the parsed sequence (ValueError on a wrong length, a position out of range, a
        stated wild type that differs from the parsed residue, a substitution at a '-' position), or — all variants at once — an
        integer matrix [V, L] of ALPHABET indices. Entry [v, pos, a] is relative to the variant's own residue at pos;
        ``subtract_mut=False`` models return the un-subtracted head output, as ``ssm_table`` does."""
        from .variant_scan import variant_matrix
        entry = pdb[0] if isinstance(pdb, (list, tuple)) else pdb
        if isinstance(variants, (np.ndarray, torch.Tensor)):
            Sv = torch.as_tensor(variants)
        else:
            Sv = torch.from_numpy(variant_matrix(entry["seq"], list(variants)))
        if Sv.dim() != 2 or Sv.shape[1] != len(entry["seq"]):          # (before the encoder runs; _tables_over checks it against the encoding)
            raise ValueError(f"variants: expected [V, {len(entry['seq'])}] sequences, got {tuple(Sv.shape)}")
        return self._tables_over(self._encode_structure(entry), Sv)

    def double_mutant_hits(self, pdb, k: int, **kw):
        """The ``k`` most stabilising double mutants of one parsed structure, best first, as ``variant_scan.PairHit``: the backbone
        is encoded once, the single-substitution backgrounds are decoded a chunk at a time and every chunk is reduced to ``k`` keys
        on the device (``variant_scan.double_mutant_hits``, which documents the options)."""
        from .variant_scan import double_mutant_hits
        return double_mutant_hits(self, pdb, k, **kw)

    def double_mutant_map(self, pdb, **kw):
        """Every site pair's best double mutant, the extremes of its epistasis and the mean size of it, as ``variant_scan.PairMap``:
        the backbone is encoded once, the single-substitution backgrounds are decoded a chunk at a time and every chunk is reduced
        into the [P, L] state on the device (``variant_scan.double_mutant_map``, which documents the options)."""
        from .variant_scan import double_mutant_map
        return double_mutant_map(self, pdb, **kw)

    def multi_mutant_search(self, pdb, order: int, beam: int, **kw):
        """A beam search for the most stabilising mutants of 1 .. ``order`` substitutions of one parsed structure, one list of
        ``variant_scan.MultiHit`` per level, best first: the backbone is encoded once, every round decodes the beam's sequences in
        their own backgrounds and one step on the device keeps the ``beam`` best distinct children
        (``variant_scan.multi_mutant_search``, which documents the number, the coverage and the options)."""
        from .variant_scan import multi_mutant_search
        return multi_mutant_search(self, pdb, order, beam, **kw)

    def multi_mutant_search_each(self, pdbs, order: int, beam: int, **kw):
        """``multi_mutant_search`` for many parsed structures at once, one list of levels per structure with the same hits, bit for
        bit: the structures are packed, every pack is encoded once, and every round is ONE decode of the pack's beams and ONE step
        on the device for all of its proteins (``variant_scan.multi_mutant_search_each``)."""
        from .variant_scan import multi_mutant_search_each
        return multi_mutant_search_each(self, pdbs, order, beam, **kw)

    def ensemble_table(self, members, cutoff=None, align: bool = False, reference=None, min_identity: float = 0.9,
                       superpose: bool = False, fit_to: int = 0, max_rmsd=None):
        """Per-mutation statistics across the parsed members of ONE conformer ensemble (``pdb_io.parse_pdb_models`` of a multi-MODEL
        file, or one ``alt_parse_PDB`` entry per file), as ``ensemble.EnsembleTable``: mean, spread, lo, hi, lo_member, hi_member,
        count, below, [L, 20] each, on the model's device. One ``tied_featurize``, ONE fused forward over the packed members and ONE
        reduction on the device (``Engine.ensemble_stats``). ``cutoff`` (None: +inf) is what ``below`` counts against. Serves the
        released head configuration with ``subtract_mut``; NotImplementedError otherwise. ``align=True``: members of unequal length are
        aligned on the device to ``reference`` (a sequence string or a one-record FASTA file; default: member 0's sequence) by the
        rule of ``datasets.global_alignment_map`` and the statistics read through that map; the table gains ``aligned`` and
        ``identity``, and a member below ``min_identity`` raises ValueError (``ensemble.scan_ensembles``). ``superpose=True``: before
        the forward every member is laid on member ``fit_to`` by the optimal proper rotation of the C-alpha atoms both have
        (``Engine.superpose``, two small launches); the table gains ``rmsd`` [M], ``n_fit`` [M], ``rmsf`` [L], ``deviation`` [M, L] and
        ``xform`` [M, 12], and a member whose RMSD exceeds ``max_rmsd`` raises ValueError before any forward. The ddG statistics are
        the same bits with and without it."""
        from .ensemble import ensemble_table
        return ensemble_table(self, members, cutoff=cutoff, align=align, reference=reference, min_identity=min_identity, superpose=superpose,
                              fit_to=fit_to, max_rmsd=max_rmsd)

    def ensemble_hits(self, members, k: int, rank: str = "mean", cutoff=None, include_cys: bool = False, one_per_position: bool = False,
                      min_members=None, align: bool = False, reference=None, min_identity: float = 0.9, superpose: bool = False,
                      fit_to: int = 0, max_rmsd=None):
        """The ``k`` most stabilising substitutions of one conformer ensemble, best first, as ``ensemble.EnsembleHit``: the
        statistics of ``ensemble_table`` and ONE selection on the device over the table ``rank`` names — "mean", "worst" (the
        largest ddG over the members: stabilising in every conformer) or "best" (the smallest). ``min_members`` drops entries in
        which fewer members take part; the other options are ``hit_list``'s. Only the hits and their statistics are copied back.
        ``align``, ``reference``, ``min_identity``: as ``ensemble_table``; positions are then the axis'. ``superpose``, ``fit_to``,
        ``max_rmsd``: as ``ensemble_table``; every hit then carries ``rmsf``, the RMSF of its position."""
        from .ensemble import ensemble_hits
        return ensemble_hits(self, members, k, rank=rank, cutoff=cutoff, include_cys=include_cys, one_per_position=one_per_position,
                             min_members=min_members, align=align, reference=reference, min_identity=min_identity, superpose=superpose,
                             fit_to=fit_to, max_rmsd=max_rmsd)

    def _encode_structure(self, entry):
        """One parsed structure -> its EncodedBackbone (Engine.encode: the part of a forward that never reads the sequence)."""
        device = next(self.parameters()).device
        feats = tied_featurize([entry], device, None, None, None, None, None, None, ca_only=False)
        X, mask, chain_enc, residue_idx = feats[0], feats[2], feats[5], feats[12]
        eng = self.engine()
        L = X.shape[1]
        with torch.cuda.device(eng.device):
            return eng.encode(X[0], mask[0], residue_idx[0], chain_enc[0], torch.tensor([0, L], dtype=torch.int32), max_len=L)

    def _encode_structures(self, entries):
        """The packed sibling of ``_encode_structure``: several parsed structures -> ONE EncodedBackbone over their rows laid end to
        end (one Engine.encode; ``enc.offsets`` [P + 1] on the device). Every structure is featurized as ``_encode_structure``
        featurizes it alone, so the forward's batch independence makes its rows those of its own encoding."""
        device = next(self.parameters()).device
        parts = []
        for entry in entries:
            feats = tied_featurize([entry], device, None, None, None, None, None, None, ca_only=False)
            parts.append((feats[0][0], feats[2][0], feats[12][0], feats[5][0]))
        lens = [int(p[0].shape[0]) for p in parts]
        X, mask, residue_idx, chain_enc = (torch.cat([p[i] for p in parts]) for i in range(4))
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
        eng = self.engine()
        with torch.cuda.device(eng.device):
            return eng.encode(X, mask, residue_idx, chain_enc, offsets, max_len=max(lens))

    def _tables_over(self, enc, Sv) -> torch.Tensor:
        """The body of ``variant_tables`` behind the encoder: ``Sv`` [V, L] index matrix -> [V, L, 21] over an EncodedBackbone, which
        a caller that decodes chunk after chunk (``double_mutant_hits``) makes once."""
        Sv = torch.as_tensor(Sv)
        eng = self.engine()
        L = enc.T
        if Sv.dim() != 2 or Sv.shape[1] != L:
            raise ValueError(f"variants: expected [V, {L}] sequences, got {tuple(Sv.shape)}")
        V = Sv.shape[0]
        with torch.cuda.device(eng.device):
            std = self.subtract_mut and not self.generic_head
            res = eng.decode_variants(enc, Sv, want_ddg=not self.generic_head, want_hidden=not std)
            if std:
                return res["ddg"]
            Sf = Sv.reshape(-1).to(device=eng.device, dtype=torch.int32)
            hid = res["hidden"].permute(1, 0, 2, 3).reshape(3, V * L, HIDDEN_DIM).contiguous()      # the head runs over V L rows
            if self.generic_head:
                ddg, z = self._generic_tables(eng, hid, Sf)
            else:
                ddg, z = res["ddg"].view(V * L, VOCAB_DIM), eng.ddg_head(hid[2], hid[1], Sf, want_z=True)[1]
            out = ddg if self.subtract_mut else z * self.ddg_out.weight.view(()) + self.ddg_out.bias.view(())
            return out.view(V, L, VOCAB_DIM)

    def sequence_log_probs(self, pdb, chain_M=None, randn=None, packed=False, X=None) -> torch.Tensor:
        """log p(sequence | structure) of one parsed structure, [L, 21], under the decoding order
        ``decoding_ranks(chain_M * mask, randn)`` (chain_M None: every residue designable; randn None: drawn), with a graph over
        ``prot_mpnn``'s parameters, W_out included (thermompnn_amd/autograd.py). Needs ``differentiable = True``. Together with
        the ddG loss it is two backward passes into the same ``.grad``s. ``packed`` is the switch of
        ``model_utils.ProteinMPNN.packed``; one structure is a batch of one, which takes the per-protein call either way.
        ``X`` [L,4,3], a float tensor on the model's device, replaces the parsed coordinates (sequence, mask, numbering and chains
        still come from ``pdb``); when it requires grad the graph reaches it: ``X.grad`` is dL / dX with the neighbour graph and
        D_max of ``_dist`` held constant (include/tmpnn.h). ``X`` needs unfrozen ProteinMPNN parameters."""
        from . import autograd as _autograd
        return _autograd.transfer_sequence_log_probs(self, pdb, chain_M, randn, X)

    def forward_coords(self, X, pdb, mutations):
        """The differentiable ``forward`` with ``X`` [L,4,3] (a float tensor on the model's device) in place of the parsed coordinates:
        the same return value, and when ``X`` requires grad the ddG values carry a graph to it as well (tmpnn_finetune_backward_x;
        with num_final_layers = 0 the head never reads the structure and ``X.grad`` is zero). Needs ``differentiable = True`` and
        unfrozen ProteinMPNN parameters; always takes the gradient path's exact fp32 kernels."""
        from . import autograd as _autograd
        if not self.differentiable:
            raise RuntimeError(_autograd._NOT_DIFFERENTIABLE.format("forward_coords"))
        return _autograd.transfer_forward(self, pdb, mutations, X)

    def forward(self, pdb, mutations, tied_feat=True):
        if self.differentiable:
            from . import autograd as _autograd
            if _autograd.wants_grad(self):
                return _autograd.transfer_forward(self, pdb, mutations)
        device = next(self.parameters()).device
        feats = tied_featurize([pdb[0]], device, None, None, None, None, None, None, ca_only=False)
        X, S, mask, chain_enc, residue_idx = feats[0], feats[1], feats[2], feats[5], feats[12]
        eng = self.engine()
        L = X.shape[1]
        with torch.cuda.device(eng.device):
            res = eng.ssm_forward(X[0], S[0], mask[0], residue_idx[0], chain_enc[0],
                                  torch.tensor([0, L], dtype=torch.int32), max_len=L, want_hidden=True,
                                  want_ddg=not self.generic_head)
            z_generic = None
            if self.generic_head:
                res["ddg"], z_generic = self._generic_tables(eng, res["hidden"], S[0])
            ddg = res["ddg"]                                        # [L,21]: (w z_a + b) - (w z_wt + b), wt = S
            live = [m for m in mutations if m is not None]
            if not live:
                return [None for _ in mutations], None
            # (host side of a 20 x L scan: three list comprehensions and ONE host-to-device copy, not 3 x 20 L appends and 3 copies)
            code = _AA_INDEX
            sel = torch.tensor([[m.position for m in live],
                                [code[m.mutation] if m.mutation in code else ALPHABET.index(m.mutation) for m in live],
                                [code[m.wildtype] if m.wildtype in code else ALPHABET.index(m.wildtype) for m in live]], device=device)
            pos_t, aa_t, wt_t = sel[0], sel[1], sel[2]
            if self.subtract_mut and bool((S[0][pos_t] == wt_t).all()):
                vals = ddg[pos_t, aa_t]
            else:   # a stated wild type that differs from the structure, or subtract_mut=False: use z directly
                hid = res["hidden"]
                z = z_generic if self.generic_head else eng.ddg_head(hid[2], hid[1], S[0], want_z=True)[1]
                zz = z * self.ddg_out.weight.view(()) + self.ddg_out.bias.view(())
                vals = zz[pos_t, aa_t] - zz[pos_t, wt_t] if self.subtract_mut else zz[pos_t, aa_t]
        pieces = iter(vals.split(1))                               # Tensor[1] views, made in one C++ call (transfer_model.py:117-119)
        return [None if m is None else {"ddG": next(pieces)} for m in mutations], None
