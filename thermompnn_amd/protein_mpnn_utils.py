"""Drop-in counterpart of the hot-path symbols of /root/reference/protein_mpnn_utils.py.

Same names, signatures and return conventions; the arithmetic runs in libtmpnn.so
(hand-written HIP for gfx950) — this module only packs arguments. Out-of-scope symbols of the
reference file (StructureDataset*, loss_*) are not provided.
``ProteinMPNN(ca_only=True)`` is: CA_ProteinFeatures (:911-1081) runs in the engine's C-alpha featurizer (tmpnn_graph_ca.hip); every
method then takes ``X`` [B,L,3] as the reference does.
``ProteinMPNN.conditional_probs`` / ``unconditional_probs`` (:1496-1587) are: the masked decoder runs in tmpnn_decode_ordered.
``ProteinMPNN.sample`` (:1279-1383) is: whole chains are sampled autoregressively inside one launch (tmpnn_sample).
``tied_sample`` (:1385-1494), the PSSM flags of ``sample`` and the design dictionaries of ``tied_featurize`` live in
``thermompnn_amd.design`` (``ProteinMPNNDesign``, a subclass of this module's ``ProteinMPNN``, and ``design.tied_featurize``).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import weights as _weights
from .engine import SAMPLE_TABLES, Engine, cat_neighbors_nodes, gather_edges, gather_nodes  # noqa: F401  (API surface)
from .pdb_io import alt_parse_PDB, featurize, tied_featurize  # noqa: F401  (API surface)


def decoding_order(order_mask, randn) -> torch.Tensor:
    """The reference's ``decoding_order = argsort((order_mask + 0.0001) * abs(randn))`` (protein_mpnn_utils.py:1297, :1533), with
    that expression: decoding_order[..., s] is the residue decoded at step s."""
    return torch.argsort((order_mask + 0.0001) * (torch.abs(randn)))


def decoding_ranks(order_mask, randn) -> torch.Tensor:
    """int32 ranks [..., L] for ``Engine.decode_ordered``: the inverse permutation of ``decoding_order`` —
    rank[..., p] is the step at which residue p is decoded, and a residue sees the neighbours of lower rank."""
    order = decoding_order(order_mask, randn)
    steps = torch.arange(order.shape[-1], device=order.device).expand_as(order)
    return torch.empty_like(order).scatter_(-1, order, steps).to(torch.int32)


def pack_sample_args(randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos, omit_AA_mask, bias_by_res):
    """Host-side packing of ``ProteinMPNN.sample``'s arguments for ``Engine.sample`` (no device needed), with the reference's
    expressions (:1296-1298, :1351-1353, :1372) -> dict(decoding_order [B,L] int64, free [B,L], bias [B,L,21],
    allowed [B,L,21] or None). free = chain_mask * chain_M_pos (the kernel multiplies by the mask); the softmax argument is
    logits / temperature + bias, bias = (bias_AAs_np + bias_by_res) / temperature - 1e8 * omit_AAs_np; allowed = 1 - omit_AA_mask."""
    f = lambda x: torch.as_tensor(x).to(dtype=torch.float32)
    chain_mask, mask = f(chain_mask), f(mask).to(chain_mask.device if isinstance(chain_mask, torch.Tensor) else "cpu")
    free = chain_mask * f(chain_M_pos).to(chain_mask.device)
    order = decoding_order(free * mask, f(randn).to(chain_mask.device))
    B, L = free.shape
    by_res = f(bias_by_res).to(chain_mask.device) if bias_by_res is not None else torch.zeros((B, L, 21), device=chain_mask.device)
    bias = (f(bias_AAs_np).to(chain_mask.device)[None, None, :] + by_res) / float(temperature) \
        - 1e8 * f(omit_AAs_np).to(chain_mask.device)[None, None, :]
    allowed = None if omit_AA_mask is None else 1.0 - f(omit_AA_mask).to(chain_mask.device)
    return {"decoding_order": order, "free": free, "bias": bias.expand(B, L, 21).contiguous(), "allowed": allowed}


def _register_tree(root: nn.Module, shapes) -> None:
    """Register parameters under the reference's dotted state-dict names (containers only; no forward)."""
    for name, shape in shapes.items():
        mod = root
        *path, leaf = name.split(".")
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, nn.Module())
            mod = mod._modules[part]
        p = torch.empty(shape)
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)                 # protein_mpnn_utils.py:1217-1219
        elif leaf == "weight":
            nn.init.ones_(p)
        else:
            nn.init.zeros_(p)
        mod.register_parameter(leaf, nn.Parameter(p))


class _EngineOwner(nn.Module):
    """Builds (and rebuilds after load_state_dict / .to()) the native engine from the module's parameters."""

    _engine = None
    _engine_key = None
    k_neighbors = 48
    precision = None          # matrix-core path of the engine ("f16x2" | "bf16x3" | "fp32"; None = library default). The gradient
                              # path of TransferModel (differentiable = True) always runs the exact fp32 training kernels instead
    retry_precision = "bf16x3"   # Engine reruns an f16x2 forward that left the fp16 range at this precision (None: raise)
    _engine_kwargs: dict = {}    # extra Engine(...) arguments of a subclass (TransferModel with a generic head: with_head=False)

    def _state_for_engine(self):
        return {k: v for k, v in self.state_dict().items()}

    def engine(self) -> Engine:
        params = list(self.parameters())
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("thermompnn_amd runs on MI355X only: move the model to a CUDA (ROCm) device "
                               "with .cuda(); there is no CPU execution path")
        key = (tuple((p.data_ptr(), p._version) for p in params), self.precision, self.retry_precision)
        if self._engine is None or key != self._engine_key:
            self._engine = Engine(self._state_for_engine(), dev, self.k_neighbors, precision=self.precision,
                                  retry_precision=self.retry_precision, **self._engine_kwargs)
            self._engine_key = key
        return self._engine


class ProteinMPNN(_EngineOwner):
    """Constructor/forward signature of the reference class (protein_mpnn_utils.py:1184-1277)."""

    def __init__(self, num_letters, node_features, edge_features, hidden_dim, num_encoder_layers=3,
                 num_decoder_layers=3, vocab=21, k_neighbors=64, augment_eps=0.05, dropout=0.1, ca_only=False):
        super().__init__()
        if (num_letters, node_features, edge_features, hidden_dim, vocab) != (21, 128, 128, 128, 21) or \
                (num_encoder_layers, num_decoder_layers) != (3, 3):
            raise NotImplementedError("the HIP engine is specialised for the ThermoMPNN configuration: "
                                      "21 letters, 128-d features, 3 encoder + 3 decoder layers")
        if not 1 <= int(k_neighbors) <= 48:
            raise NotImplementedError(f"k_neighbors={k_neighbors}: this build supports 1..48 (v_48_* weights)")
        if augment_eps and augment_eps > 0:
            raise NotImplementedError("augment_eps > 0 adds training noise; ThermoMPNN uses 0.0 (transfer_model.py:27)")
        self.node_features, self.edge_features, self.hidden_dim = node_features, edge_features, hidden_dim
        self.k_neighbors = int(k_neighbors)
        self.ca_only = bool(ca_only)
        # ca_only: the reference's parameter tree (CA_ProteinFeatures' own and W_v, :927-930, :1197), so that load_state_dict of a
        # ca_model_weights checkpoint is strict-clean; the engine drops the five its forward never reads
        _register_tree(self, _weights.mpnn_param_shapes(ca_only=self.ca_only))

    def _backbone(self, X):
        """X as the engine takes it, [B,L,4,3]: a ca_only model's [B,L,3] goes into slot 1 (C-alpha) of a zero tensor on the device."""
        if not self.ca_only:
            return X
        if X.dim() != 3 or X.shape[-1] != 3:
            raise ValueError(f"ca_only: X must be [B, L, 3] (C-alpha coordinates), got {tuple(X.shape)}")
        X4 = torch.zeros((X.shape[0], X.shape[1], 4, 3), dtype=torch.float32, device=self.engine().device)
        X4[:, :, 1] = X.to(X4.device, torch.float32)
        return X4

    def forward(self, X, S, mask, chain_M, residue_idx, chain_encoding_all, randn, use_input_decoding_order=False,
                decoding_order=None):
        """-> (list of 3 decoder states [B,L,128] in REVERSED order, h_S [B,L,128], log_probs [B,L,21]).
        ``chain_M``, ``randn`` and the decoding-order arguments do not influence the outputs on this path
        (the reference overwrites its order mask with ones, :1259)."""
        eng = self.engine()
        B, L = X.shape[0], X.shape[1]
        offsets = torch.arange(B + 1, dtype=torch.int32) * L
        with torch.cuda.device(eng.device):
            res = eng.ssm_forward(self._backbone(X).reshape(B * L, 4, 3), S.reshape(-1), mask.reshape(-1), residue_idx.reshape(-1),
                                  chain_encoding_all.reshape(-1), offsets, max_len=L, want_ddg=False,
                                  want_hidden=True, want_log_probs=True)
            h_S = eng.seq_embed(S.reshape(-1)).view(B, L, -1)
        hidden = res["hidden"].view(3, B, L, -1)
        return [hidden[2], hidden[1], hidden[0]], h_S, res["log_probs"].view(B, L, -1)

    def _encode_padded(self, eng, X, mask, residue_idx, chain_encoding_all):
        """The padded batch [B,L,...] as ``forward`` lays it out: B proteins of L rows each on the packed residue axis."""
        B, L = X.shape[0], X.shape[1]
        offsets = torch.arange(B + 1, dtype=torch.int32) * L
        return eng.encode(self._backbone(X).reshape(B * L, 4, 3), mask.reshape(-1), residue_idx.reshape(-1), chain_encoding_all.reshape(-1),
                          offsets, max_len=L)

    def conditional_probs(self, X, S, mask, chain_M, residue_idx, chain_encoding_all, randn, backbone_only=False):
        """-> log p(aa at idx | structure, every other residue) [B,L,21] for every idx with chain_M * mask == 1, rows of the other
        positions exactly 0 (reference :1496-1555): one encode, then one full decode per looped position under the order that
        puts that position last and the others in |randn| order — all of them variants of ONE ``decode_ordered`` call.
        ``backbone_only=True`` puts the position first instead; its logits then only ever read encoder states of its neighbours,
        so every looped row equals the all-invisible decode's (``unconditional_probs``): one decode, rows copied."""
        B, L = X.shape[0], X.shape[1]
        if B != 1:
            raise NotImplementedError("conditional_probs: one structure per call (the reference takes the positions to loop over "
                                      "from batch member 0 for every member)")
        eng = self.engine()
        out = torch.zeros((B, L, 21), dtype=torch.float32, device=eng.device)
        idx = torch.nonzero((chain_M * mask)[0] == 1)[:, 0].to(eng.device)
        if idx.numel() == 0:
            return out
        with torch.cuda.device(eng.device):
            enc = self._encode_padded(eng, X, mask, residue_idx, chain_encoding_all)
            if backbone_only:
                lp = eng.decode_ordered(enc, torch.zeros((1, L), dtype=torch.int32), torch.zeros((1, L), dtype=torch.int32))["log_probs"]
                out[0, idx] = lp[0, idx]
            else:
                order_mask = torch.zeros((idx.numel(), L), device=eng.device)
                order_mask[torch.arange(idx.numel(), device=eng.device), idx] = 1.0
                ranks = decoding_ranks(order_mask, randn.to(eng.device).reshape(1, L))
                lp = eng.decode_ordered(enc, S.reshape(1, L).expand(idx.numel(), L), ranks)["log_probs"]
                out[0, idx] = lp[torch.arange(idx.numel(), device=eng.device), idx]
        return out

    def unconditional_probs(self, X, mask, residue_idx, chain_encoding_all):
        """-> log p(aa | structure alone) [B,L,21] (reference :1557-1587): the decode in which no residue sees another's identity."""
        eng = self.engine()
        B, L = X.shape[0], X.shape[1]
        with torch.cuda.device(eng.device):
            enc = self._encode_padded(eng, X, mask, residue_idx, chain_encoding_all)
            zeros = torch.zeros((1, B * L), dtype=torch.int32)
            return eng.decode_ordered(enc, zeros, zeros)["log_probs"].view(B, L, 21)

    def sample(self, X, randn, S_true, chain_mask, chain_encoding_all, residue_idx, mask=None, temperature=1.0,
               omit_AAs_np=None, bias_AAs_np=None, chain_M_pos=None, omit_AA_mask=None, pssm_coef=None, pssm_bias=None,
               pssm_multi=None, pssm_log_odds_flag=None, pssm_log_odds_mask=None, pssm_bias_flag=None,
               bias_by_res=None, generator=None, uniforms=None):
        """-> {"S" [B,L] int64, "probs" [B,L,21], "decoding_order" [B,L]} (reference :1279-1383): every batch member is one chain
        sampled autoregressively on the device — residue by residue in the reference's decoding order, each letter fed to the
        residues decoded after it — inside one launch (``Engine.sample``). When all members share ``X / mask / residue_idx /
        chain_encoding_all`` and the per-residue tables (the usual batch of copies of one structure) the structure is encoded once
        and the B members run as B chains; otherwise the padded batch is encoded once and member b is sampled as one chain over
        protein b's own steps, all members inside one launch (``Engine.sample_each``) — the bits of B calls with one member each.

        Random stream: one uniform per (member, residue) from ``torch.rand(..., generator=generator)`` on the device picks the
        letter by inverse CDF (the smallest a whose running sum of probs exceeds u * total). The DISTRIBUTION is the
        reference's; the stream is not ``torch.multinomial``'s, so equal seeds do not give the reference's sequences.
        ``uniforms`` [B,L] (indexed by residue) replaces the draw, e.g. to replay recorded ones.
        pssm_bias_flag / pssm_log_odds_flag are not supported here (NotImplementedError) and ``tied_sample`` is not provided:
        ``thermompnn_amd.design.ProteinMPNNDesign`` has both."""
        if pssm_bias_flag or pssm_log_odds_flag:
            raise NotImplementedError("sample: pssm_bias_flag / pssm_log_odds_flag are served by thermompnn_amd.design.ProteinMPNNDesign")
        pk = self._packed("sample", pack_sample_args, randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos,
                          omit_AA_mask, bias_by_res)
        S, probs = self._sample_members("sample", X, S_true, chain_encoding_all, residue_idx, mask, temperature, pk, generator, uniforms)
        return {"S": S, "probs": probs, "decoding_order": pk["decoding_order"]}

    def _packed(self, what, pack, randn, chain_mask, mask, temperature, omit_AAs_np, bias_AAs_np, chain_M_pos, *rest):
        """``pack`` (``pack_sample_args`` or one with its leading arguments) on the engine's device, with the reference's defaults for
        chain_M_pos / omit_AAs_np / bias_AAs_np; ``rest`` goes to ``pack`` as given."""
        if not float(temperature) > 0.0:
            raise ValueError(f"{what}: temperature must be positive, got {temperature!r}")
        dev = self.engine().device
        if mask is None:
            raise ValueError(f"{what}: mask is required")
        if chain_M_pos is None:
            chain_M_pos = torch.ones_like(chain_mask)
        zeros21 = torch.zeros(21)
        return pack(randn.to(dev), chain_mask.to(dev), mask.to(dev), temperature, zeros21 if omit_AAs_np is None else omit_AAs_np,
                    zeros21 if bias_AAs_np is None else bias_AAs_np, chain_M_pos.to(dev), *rest)

    def _sample_members(self, what, X, S_true, chain_encoding_all, residue_idx, mask, temperature, pk, generator, uniforms):
        """The members as chains of the sampler, ``pk`` from ``pack_sample_args`` (``Engine.sample`` / ``sample_each``) or with a
        "close" key from ``design.pack_tied_args`` (``Engine.sample_tied`` / ``sample_tied_each``): one encode and B chains when the
        members share the structure and the per-residue tables of ``pk``; otherwise one padded encode and the per-protein entry,
        member b as one chain over protein b's own steps. -> (S [B,L] int64, probs [B,L,21])."""
        eng = self.engine()
        dev = eng.device
        B, L = X.shape[0], X.shape[1]
        S_true = S_true.to(dev)
        if S_true.numel() and (int(S_true.min()) < 0 or int(S_true.max()) >= 21):
            raise ValueError(f"{what}: S_true must lie in [0, 21)")
        tied, order = "close" in pk, pk["decoding_order"]
        tables = {k: pk[k] for k in SAMPLE_TABLES if k in pk}
        with torch.cuda.device(dev):
            if uniforms is None:
                uniforms = torch.rand((B, L), device=dev, dtype=torch.float32, generator=generator)
            u = torch.as_tensor(uniforms).to(device=dev, dtype=torch.float32).reshape(B, L)
            same = lambda t: t is None or bool((t[1:] == t[:1]).all())
            shared = B > 1 and all(same(t) for t in (X.to(dev), mask.to(dev), residue_idx.to(dev), chain_encoding_all.to(dev), *tables.values()))
            if shared or B == 1:
                enc = self._encode_padded(eng, X[:1], mask[:1], residue_idx[:1], chain_encoding_all[:1])
                kw = dict(temperature=float(temperature), **{k: None if t is None else t[0] for k, t in tables.items()})
                if tied:
                    r = eng.sample_tied(enc, order, pk["close"], S_true, pk["free"], u, weight=pk["weight"], **kw)
                else:
                    r = eng.sample(enc, order, S_true, pk["free"], u, **kw)
                return r["S"].to(torch.int64), r["probs"]
            # ONE padded encode and ONE launch: member b is protein b of the packed axis, sampled as one chain over its own steps
            enc = self._encode_padded(eng, X, mask, residue_idx, chain_encoding_all)
            flat = lambda t: None if t is None else t.reshape(B * L, *t.shape[2:])
            row = lambda t: None if t is None else flat(t)[None]
            shift = (torch.arange(B, device=dev, dtype=order.dtype) * L)[:, None]
            kw = dict(temperature=float(temperature), **{k: flat(t) for k, t in tables.items()})
            if tied:
                r = eng.sample_tied_each(enc, row(order + shift), row(pk["close"]), row(S_true), row(pk["free"]), row(u),
                                         weight=row(pk["weight"]), **kw)
            else:
                r = eng.sample_each(enc, row(order + shift), row(S_true), row(pk["free"]), row(u), **kw)
        return r["S"].view(B, L).to(torch.int64), r["probs"].view(B, L, 21)
