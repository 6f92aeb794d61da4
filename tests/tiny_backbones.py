"""Many small synthetic backbones for the packed-batch tests (test helper, imported like masked_backbones.py; never imported by the
product): one chain, a random 20-letter sequence, optionally one masked residue, everything from fixed seeds.
"""
import numpy as np

from thermompnn_amd.synthetic import synthetic_backbone


def tiny_member(L, seed, masked=None):
    """-> X [L,4,3] float32, S [L] int64, mask [L] float32, residue_idx [L] int64, chain_enc [L] int64 of synthetic_backbone(L, seed)
    under a random sequence drawn from ``seed``. ``masked``: a residue that lost its N line, as masked_backbones.layout_arrays makes
    one (its N coordinates zeroed, its letter kept, mask 0)."""
    X = synthetic_backbone(L, seed)[0].astype(np.float32)
    S = np.random.default_rng(seed).integers(0, 20, L).astype(np.int64)
    mask = np.ones(L, np.float32)
    if masked is not None:
        assert 0 <= masked < L
        X[masked, 0] = 0.0
        mask[masked] = 0.0
    return X, S, mask, np.arange(L, dtype=np.int64), np.ones(L, np.int64)


def many_short(n=260, seed0=1000):
    """The pack of ``n`` short proteins: lengths 8 + (5 b mod 9) (8..16, odd and even mixed, so most member boundaries sit off every
    tile size), backbone seed ``seed0`` + b, the middle residue of every third member masked. -> list of tiny_member tuples."""
    out = []
    for b in range(n):
        L = 8 + (5 * b) % 9
        out.append(tiny_member(L, seed0 + b, masked=L // 2 if b % 3 == 0 else None))
    return out
