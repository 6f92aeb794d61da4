"""The reference's ``_scores`` on a small hand-made table (runs only where make_golden.py runs: it imports the reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scores_golden.py

Writes scores_small.npz: S int64 [3,7], log_probs float32 [3,7,21] (log-softmax of seeded normals), mask float32 [3,7] (row 0 all
ones, row 1 with masked and fixed positions, row 2 a single designed position) and scores float32 [3], the reference's result.
tests/test_sample_each_host.py compares thermompnn_amd.design_scan.scores with it."""
import os

import numpy as np
import torch

import make_golden as mg          # the same directory: imports the reference

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    rng = np.random.default_rng(0)
    S = rng.integers(0, 21, (3, 7))
    log_probs = torch.log_softmax(torch.from_numpy(rng.normal(size=(3, 7, 21)).astype(np.float32)) * 2.0, dim=-1)
    mask = np.ones((3, 7), np.float32)
    mask[1, [0, 3, 6]] = 0
    mask[2] = 0
    mask[2, 4] = 1
    out = mg.ref_utils._scores(torch.from_numpy(S), log_probs, torch.from_numpy(mask))
    np.savez(os.path.join(HERE, "scores_small.npz"), S=S.astype(np.int64), log_probs=log_probs.numpy(), mask=mask,
             scores=out.numpy().astype(np.float32))
    print("scores", out.tolist())


if __name__ == "__main__":
    main()
