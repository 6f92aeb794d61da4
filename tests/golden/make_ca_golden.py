"""Generate the C-alpha-only (ca_only) fixtures by IMPORTING THE REFERENCE (runs only in the build container, on the CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ca_golden.py            (every file)
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ca_golden.py off_tile   (ca_msk_L17 / L47 / L49 only)

Builds the reference's ProteinMPNN(ca_only=True) with thermompnn_amd.weights.synthetic_state_dict(0, "mpnn_ca") (strict load) and
runs it in float32 and in float64 (default dtype float64 and Tensor.float -> double for the duration of the run: the reference's
`.float()` on the one-hot of PositionalEncodings and its `torch.zeros(Ca.shape)` are the only obstacles). Stores only tensors.

ca_<case>.npz, every array with a leading batch axis B:
    Ca [B,L,3], S, mask, residue_idx, chain_enc [B,L], K, E_idx [B,L,Keff] (the float32 reference's own top-k; the float64 run is
        made on the same graph),
    rows [n] and E64_rows [B,n,Keff,128]: the featurizer's float64 output E on a few rows (first three, last three, the rest spread;
        a full E does not fit a committed file: 12 bytes per value in both precisions) — tests/ca_restatement.py must reproduce
        them to 1e-12 and then stands for the float64 featurizer on every edge;
    ref32_well / ref32_ill: the reference-fp32's largest distance from its float64 self over ALL well- / ill-conditioned edges
        (ca_restatement.well_conditioned on the float64 frames), ill_fraction: the share of ill-conditioned edges;
    hidden32 / hidden64 [3,B,L,128] (decoder layers 1..3), log_probs32 / log_probs64 [B,L,21]  (2OCJ: log_probs only);
    min_window_margin: the smallest distance of a C-alpha step length from 3.6 and 4.0 (asserted >= 1e-3).
Ties: torch.topk is replaced by a stable sort for the whole script (equal distances: lowest index first, the engine's rule).
Cases: syn_L32 (Keff 32 < 48), syn_L40 with k_neighbors = 30, msk_L40, msk_L56_2ch (tests/masked_backbones.py: missing C-alpha -> 0),
msk_L17, msk_L47 and msk_L49 at K = 48 (Keff 17, 47 and 48: off-tile row counts with missing C-alpha atoms; the layouts as they are,
no translation and no other seed was needed for the conditions below),
pad_L32_L40 (syn_L32 and syn_L40 as one padded batch, K = 48), 2OCJ_A and 2OCJ_AB through the reference's alt_parse_PDB(ca_only=True)
and tied_featurize(ca_only=True). Never batch size 3 or padded length 6: the reference's torch.cross calls pass no dim.
ca_params.npz: names and shapes of the reference model's state_dict(). ca_parse_2OCJ.npz: what the reference's parser and packer
return for 2OCJ A+B and the gapped chain A with ca_only=True.
ca_probs_<case>.npz: the reference's conditional_probs (with its randn) and unconditional_probs. ca_sample_<case>.npz /
ca_tied_<case>.npz: its sample / tied_sample on two copies with recorded uniforms (make_tied_sample_golden.run_case)."""
import json
import os
import sys

import numpy as np
import torch

import make_golden as mg          # the same directory: imports the reference
import make_tied_sample_golden as mts

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import ca_restatement as car                               # noqa: E402
from ca_inputs import frame_conditioned                    # noqa: E402
from masked_backbones import layout_arrays                 # noqa: E402
from thermompnn_amd.synthetic import AA20, synthetic_backbone   # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ref = mg.ref_utils


_topk = torch.topk


def stable_topk(D, k, dim=-1, largest=False):
    """torch.topk leaves the order of equal distances open; masked residues all sit at a row's D_max. The fixtures take the lowest
    index first — the engine's documented rule (DESIGN.md "Ties") — so that the reference and the device walk the same graph."""
    assert dim == -1 and not largest
    v, i = torch.sort(D, dim=-1, stable=True)
    return v[..., :k].contiguous(), i[..., :k].contiguous()


def ca_model(K, f64=False):
    m = ref.ProteinMPNN(num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3, num_decoder_layers=3,
                        k_neighbors=K, augment_eps=0.0, dropout=0.0, ca_only=True)
    r = m.load_state_dict(synthetic_state_dict(0, "mpnn_ca"), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return (m.double() if f64 else m).eval()


class Float64:
    """default dtype float64 and Tensor.float -> double while the reference runs"""

    def __enter__(self):
        self.float, self.default = torch.Tensor.float, torch.get_default_dtype()
        torch.Tensor.float = lambda t, *a, **k: t.double()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.Tensor.float = self.float
        torch.set_default_dtype(self.default)


def synthetic(L, seed):
    X, seq = synthetic_backbone(L, seed)
    return dict(Ca=X[:, 1].astype(np.float32), S=np.array([AA20.index(c) for c in seq], np.int64), mask=np.ones(L, np.float32),
                residue_idx=np.arange(L, dtype=np.int64), chain_enc=np.ones(L, np.int64))


def single(name):
    if name == "syn_L32":
        with np.load(os.path.join(HERE, "syn_L32.npz")) as z:
            return dict(Ca=z["X"][:, 1].astype(np.float32), S=z["S"].astype(np.int64), mask=z["mask"].astype(np.float32),
                        residue_idx=z["residue_idx"].astype(np.int64), chain_enc=z["chain_enc"].astype(np.int64))
    if name == "syn_L40":
        return synthetic(40, 1)
    X, S, mask, ridx, cenc = layout_arrays(name)
    Ca = X[:, 1].copy()
    Ca[np.abs(X).reshape(len(S), -1).sum(-1) == 0] = 0           # a numbering gap has no C-alpha; a residue without its N line keeps it
    return dict(Ca=Ca, S=S, mask=mask, residue_idx=ridx.astype(np.int64), chain_enc=cenc.astype(np.int64))


def padded(members):
    L = max(len(m["S"]) for m in members)
    out = {}
    for k in ("Ca", "S", "mask", "residue_idx", "chain_enc"):
        rows = []
        for m in members:
            pad = [(0, L - len(m["S"]))] + [(0, 0)] * (m[k].ndim - 1)
            rows.append(np.pad(m[k], pad, constant_values=-100 if k == "residue_idx" else 0))
        out[k] = np.stack(rows)
    return out


def pdb_case(path, chains):
    d = ref.alt_parse_PDB(path, chains, ca_only=True)[0]
    f = ref.tied_featurize([d], "cpu", None, None, None, None, None, None, ca_only=True)
    return dict(Ca=f[0].numpy(), S=f[1].numpy(), mask=f[2].numpy(), residue_idx=f[12].numpy(), chain_enc=f[5].numpy()), d, f


def window_margin(c):
    """smallest distance of a step length from 3.6 / 4.0 over the members' own rows and the rows behind them inside the padded length"""
    worst = np.inf
    for b in range(c["Ca"].shape[0]):
        n = np.linalg.norm(np.diff(c["Ca"][b].astype(np.float64), axis=0), axis=-1)
        worst = min(worst, float(np.abs(n[:, None] - np.array([3.6, 4.0])).min()))
    return worst


def run(c, K, f64, graph=None):
    """``graph``: the E_idx the run's torch.topk returns instead of its own (the float64 run takes the float32 run's, so that the two
    are compared edge by edge: neighbours at the same 3.8 A on both sides of a residue change places with the rounding)."""
    dt = torch.float64 if f64 else torch.float32
    t = torch.from_numpy
    cap = {}

    def forward():
        m = ca_model(K, f64)
        hooks = [m.features.register_forward_hook(lambda mod, i, o: cap.update(E=o[0], E_idx=o[1]))]
        hooks += [l.register_forward_hook(lambda mod, i, o, li=li: cap.update({f"h{li}": o})) for li, l in enumerate(m.decoder_layers)]
        out = m(t(c["Ca"]).to(dt), t(c["S"]), t(c["mask"]).to(dt), torch.ones(c["mask"].shape, dtype=dt), t(c["residue_idx"]),
                t(c["chain_enc"]), None, use_input_decoding_order=True,         # (its own order is one row: batches need one per member)
                decoding_order=torch.arange(c["S"].shape[1])[None].repeat(c["S"].shape[0], 1))
        for h in hooks:
            h.remove()
        return out[2]                                      # (list of decoder states, h_S, log_probs)

    real_topk = torch.topk
    if graph is not None:
        torch.topk = lambda D, k, dim=-1, largest=False: (torch.gather(D, -1, t(graph)), t(graph))
    try:
        with torch.no_grad():
            if f64:
                with Float64():
                    lp = forward()
            else:
                lp = forward()
    finally:
        torch.topk = real_topk
    assert lp.dtype == dt and cap["E"].dtype == dt
    return dict(E=cap["E"].numpy(), E_idx=cap["E_idx"].numpy(), hidden=np.stack([cap[f"h{l}"].numpy() for l in range(3)]), log_probs=lp.numpy())


def store_case(name, c, K, want_hidden=True, rows=None, new_rules=False):
    """``new_rules`` (the cases added after ca_inputs.frame_conditioned existed): every framed row passes frame_conditioned and the
    ill-conditioned share is at most 10 %, asserted here; the earlier cases keep their files byte for byte."""
    margin = window_margin(c)
    assert margin >= 1e-3, (name, margin)
    if new_rules:
        for b in range(c["Ca"].shape[0]):
            assert bool(frame_conditioned(torch.from_numpy(c["Ca"][b]).double()).all()), (name, b)
    r32 = run(c, K, False)
    r64 = run(c, K, True, graph=r32["E_idx"])
    assert np.array_equal(r32["E_idx"], r64["E_idx"])
    B, L = c["S"].shape
    E_idx = r64["E_idx"]
    rows = rows or sorted(set([0, 1, 2, L - 3, L - 2, L - 1] + list(np.linspace(3, L - 4, 4).astype(int))))
    well = np.stack([car.well_conditioned(car.frames(torch.from_numpy(c["Ca"][b]).double()), torch.from_numpy(E_idx[b])).numpy() for b in range(B)])
    # the restatement must BE the float64 reference before it stands for it
    W = synthetic_state_dict(0, "mpnn_ca")
    for b in range(B):
        t = torch.from_numpy
        Er = car.edge_features(W, t(c["Ca"][b]).double(), t(c["mask"][b]).double(), t(c["residue_idx"][b]), t(c["chain_enc"][b]), t(E_idx[b]))
        err = float((Er - t(r64["E"][b])).abs().max())
        assert err <= 1e-12, (name, b, err)
    d = np.abs(r32["E"].astype(np.float64) - r64["E"]).max(-1)
    assert not new_rules or float((~well).mean()) <= 0.10, (name, float((~well).mean()))
    out = dict(Ca=c["Ca"].astype(np.float32), S=c["S"].astype(np.int16), mask=c["mask"].astype(np.float32), residue_idx=c["residue_idx"].astype(np.int32),
               chain_enc=c["chain_enc"].astype(np.int16), K=np.int32(K), E_idx=E_idx.astype(np.int16), rows=np.array(rows, np.int32),
               E64_rows=r64["E"][:, rows], ref32_well=np.float64(d[well].max()), ref32_ill=np.float64(d[~well].max() if (~well).any() else 0.0),
               ill_fraction=np.float64((~well).mean()), min_window_margin=np.float64(margin),
               log_probs32=r32["log_probs"], log_probs64=r64["log_probs"])
    if want_hidden:
        out.update(hidden32=r32["hidden"], hidden64=r64["hidden"])
    path = os.path.join(HERE, f"ca_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"ca_{name}: B={B}, L={L}, K={K}: reference fp32 vs float64: E {out['ref32_well']:.2e} on well-conditioned edges, {out['ref32_ill']:.2e} on "
          f"the other {100 * out['ill_fraction']:.1f} %; hidden {np.abs(r32['hidden'] - r64['hidden']).max():.2e}, log_probs "
          f"{np.abs(r32['log_probs'] - r64['log_probs']).max():.2e}; window margin {margin:.3f} -> {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < (1 << 20)


def probs_case(name, c, n):
    t = torch.from_numpy
    m = ca_model(48)
    gen = torch.Generator().manual_seed(900 + n)
    L = c["S"].shape[1]
    randn = torch.randn(1, L, generator=gen)
    chain_M = torch.ones(1, L)
    chain_M[0, ::7] = 0
    with torch.no_grad():
        args = (t(c["Ca"]), t(c["S"]), t(c["mask"]), chain_M, t(c["residue_idx"]), t(c["chain_enc"]), randn)
        cond = m.conditional_probs(*args)
        uncond = m.unconditional_probs(t(c["Ca"]), t(c["mask"]), t(c["residue_idx"]), t(c["chain_enc"]))
    np.savez_compressed(os.path.join(HERE, f"ca_probs_{name}.npz"), randn=randn.numpy(), chain_M=chain_M.numpy(), conditional=cond.numpy(),
                        unconditional=uncond.numpy())
    print(f"ca_probs_{name}: {int((cond != 0).any(-1).sum())} conditional rows of {L}")


OFF_TILE = ("msk_L17", "msk_L47", "msk_L49")


def off_tile_cases():
    for name in OFF_TILE:
        m = single(name)
        store_case(name, {k: v[None] for k, v in m.items()}, 48, new_rules=True)


def main():
    torch.manual_seed(0)
    torch.topk = stable_topk                                # for every run of the reference below
    if sys.argv[1:] == ["off_tile"]:                        # only the cases added later: the other files are left as they are
        return off_tile_cases()
    with torch.no_grad():
        sd = ca_model(48).state_dict()
    np.savez_compressed(os.path.join(HERE, "ca_params.npz"), names=np.array(list(sd)), shapes=np.array(json.dumps([list(v.shape) for v in sd.values()])))
    singles = {n: single(n) for n in ("syn_L32", "syn_L40", "msk_L40", "msk_L56_2ch")}
    one = lambda m: {k: v[None] for k, v in m.items()}
    store_case("syn_L32", one(singles["syn_L32"]), 48)
    store_case("syn_L40", one(singles["syn_L40"]), 30)
    store_case("msk_L40", one(singles["msk_L40"]), 48)
    store_case("msk_L56_2ch", one(singles["msk_L56_2ch"]), 48)
    off_tile_cases()
    store_case("pad_L32_L40", padded([singles["syn_L32"], singles["syn_L40"]]), 48, rows=[0, 1, 29, 30, 31, 32, 38, 39])   # (the shorter member's end)
    pdb = os.path.join(HERE, "2OCJ.pdb")
    parse = {}
    for tag, path, chains in (("A", pdb, "A"), ("AB", pdb, ["A", "B"]), ("gapA", os.path.join(HERE, "2OCJ_gap_chainA.pdb"), "A")):
        c, d, f = pdb_case(path, chains)
        if tag != "gapA":
            store_case("2OCJ_" + tag, c, 48, want_hidden=False)
        if tag != "A":
            for ch in chains:
                parse[f"{tag}_CA_chain_{ch}"] = np.asarray(d["coords_chain_" + ch]["CA_chain_" + ch], np.float64)
            parse[tag + "_seq"] = np.array(d["seq"])
            parse.update({f"{tag}_X": f[0].numpy(), f"{tag}_S": f[1].numpy(), f"{tag}_mask": f[2].numpy(), f"{tag}_chain_M": f[4].numpy(),
                          f"{tag}_chain_enc": f[5].numpy(), f"{tag}_chain_M_pos": f[10].numpy(), f"{tag}_residue_idx": f[12].numpy()})
    np.savez_compressed(os.path.join(HERE, "ca_parse_2OCJ.npz"), **parse)
    for n, name in enumerate(("syn_L32", "msk_L56_2ch")):
        probs_case(name, one(singles[name]), n)
    # sample / tied_sample on two copies with recorded uniforms: make_tied_sample_golden.run_case on the CA model and C-alpha inputs
    as_fixture = lambda m: dict(X=m["Ca"], S=m["S"], mask=m["mask"], residue_idx=m["residue_idx"], chain_enc=m["chain_enc"])
    mts.inputs_of = lambda struct: as_fixture(singles[struct])
    mp = ca_model(48)
    cases = {"ca_sample_syn_L32": dict(struct="syn_L32", N=2, temperature=1.0, tied=None),
             "ca_sample_msk_L56_2ch": dict(struct="msk_L56_2ch", N=2, temperature=0.5, tied=None, store_graph=True),
             "ca_tied_syn_L32": dict(struct="syn_L32", N=2, temperature=1.0, tied=mts.PAIRS_SYN, beta={16: 0.5, 27: -0.5}, fixed=(5, 20)),
             "ca_tied_msk_L56_2ch": dict(struct="msk_L56_2ch", N=2, temperature=0.5, tied=[[i, 28 + i] for i in range(28)], store_graph=True)}
    for n, (name, cfg) in enumerate(cases.items()):
        mts.run_case(mp, name, cfg, 20 + n)


if __name__ == "__main__":
    main()
