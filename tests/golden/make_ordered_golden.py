"""Generate the order-masked decoding fixtures by IMPORTING THE REFERENCE (runs only in the build container, on the CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ordered_golden.py

For the structures of the existing fixtures syn_L32, 2OCJ_A and 2OCJ_A_gap (inputs are read from those files) and seed-0 Xavier
weights installed through the reference's own loading path (make_golden.build_reference_model), runs the reference's
ProteinMPNN.conditional_probs (with and without backbone_only) and unconditional_probs and stores ordered_<case>.npz: randn,
cond / cond_backbone_only / uncond [L,21], and the decoding_order the reference drew for three of the looped positions
(order_pos) — recorded from its own torch.argsort calls. Only tensors are stored.

The same for the masked layouts msk_L17, msk_L40 and msk_L56_2ch of tests/masked_backbones.py (inputs: layout_arrays; every
unmasked row lists masked residues there), whose files also hold E_idx, the graph the reference's own features module returned:
torch.topk decides the D_max ties among the masked residues, so the host test replays the reference slot by slot."""
import os
import sys
import tempfile

import numpy as np
import torch

import make_golden as mg          # the same directory: imports the reference

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
from masked_backbones import layout_arrays          # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("syn_L32", "2OCJ_A", "2OCJ_A_gap")
MASKED_CASES = ("msk_L17", "msk_L40", "msk_L56_2ch")


def inputs_of(case):
    if case in MASKED_CASES:
        X, S, mask, ridx, cenc = layout_arrays(case)
        return dict(X=X, S=S, mask=mask, residue_idx=ridx, chain_enc=cenc)
    with np.load(os.path.join(HERE, case + ".npz")) as z:
        return {k: z[k] for k in z.files}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mp = mg.build_reference_model(tmp).prot_mpnn
    for n, case in enumerate(CASES + MASKED_CASES):
        g = inputs_of(case)
        t = torch.from_numpy
        X, mask = t(g["X"])[None], t(g["mask"])[None]
        S = t(g["S"].astype(np.int64))[None]
        ridx, cenc = t(g["residue_idx"].astype(np.int64))[None], t(g["chain_enc"].astype(np.int64))[None]
        chain_M = torch.ones_like(mask)
        L = X.shape[1]
        randn = torch.randn(1, L, generator=torch.Generator().manual_seed(100 + n))
        orders, real_argsort = [], torch.argsort

        def recording_argsort(*a, **k):
            out = real_argsort(*a, **k)
            orders.append(out.clone())
            return out

        graph = {}
        hook = mp.features.register_forward_hook(lambda m, i, o: graph.update(E_idx=o[1][0].numpy().astype(np.int16)))
        with torch.no_grad():
            torch.argsort = recording_argsort
            try:
                cond = mp.conditional_probs(X, S, mask, chain_M, ridx, cenc, randn)[0]
            finally:
                torch.argsort = real_argsort
            bb = mp.conditional_probs(X, S, mask, chain_M, ridx, cenc, randn, backbone_only=True)[0]
            unc = mp.unconditional_probs(X, mask, ridx, cenc)[0]
        hook.remove()
        looped = np.nonzero(g["mask"] == 1)[0]
        assert len(orders) == len(looped)
        pick = [0, len(looped) // 2, len(looped) - 1]
        path = os.path.join(HERE, f"ordered_{case}.npz")
        np.savez_compressed(path, randn=randn.numpy(), cond=cond.numpy(), cond_backbone_only=bb.numpy(), uncond=unc.numpy(),
                            order_pos=looped[pick].astype(np.int32),
                            decoding_order=np.stack([orders[k][0].numpy() for k in pick]).astype(np.int32),
                            **(graph if case in MASKED_CASES else {}))
        print(f"ordered_{case}: L={L}, {len(looped)} looped positions -> {os.path.getsize(path) / 1024:.0f} KiB; "
              f"max |cond - uncond| {float((cond - unc)[looped].abs().max()):.3f}")


if __name__ == "__main__":
    main()
