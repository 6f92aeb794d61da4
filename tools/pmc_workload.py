"""Workload for the rocprofv3 --pmc passes (HBM traffic per launch): 3 forwards of the bench batch plus two kernels
with KNOWN byte counts to calibrate FETCH_SIZE / WRITE_SIZE on gfx950 (MI355X_MICROARCH.md §HBM):
  gather_rows: reads 3.1 MB idx + 8.4 MB table (L2-resident), writes 402.7 MB
  torch copy : reads 402.7 MB, writes 402.7 MB
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_batch  # noqa: E402
from thermompnn_amd.engine import Engine  # noqa: E402
from thermompnn_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
eng = Engine(synthetic_state_dict(0), dev, 48)
b = build_batch(64, 256, 0, dev)
if sys.argv[1:] == ["variants"]:      # a pass of its own: its single-protein encode must not enter the bench batch's per-kernel means
    # the variant decoder on the bench protein: 64 sequences over one encoded backbone (its message kernel reads a residue's h_E tile once
    # per chunk of variants; the per-variant figure is the launch's FETCH_SIZE / 64)
    enc = eng.encode(b["X"][:256], b["mask"][:256], b["ridx"][:256], b["cenc"][:256], b["offsets"][:2], max_len=256)
    Sv = b["S"][:256].repeat(64, 1)
    Sv[torch.arange(64), torch.arange(64)] = (Sv[torch.arange(64), torch.arange(64)] + 1) % 20
    for _ in range(3):
        eng.decode_variants(enc, Sv)
    torch.cuda.synchronize()
    print("ok variants")
    raise SystemExit(0)
out = {"ddg": torch.empty((b["T"], 21), device=dev)}
for _ in range(3):
    eng.ssm_forward(b["X"], b["S"], b["mask"], b["ridx"], b["cenc"], b["offsets"], max_len=256, out=out)
g = torch.Generator().manual_seed(0)
nodes = torch.randn(16384, 128, generator=g).to(dev)
idx = ((torch.arange(16384) // 256 * 256).repeat_interleave(48) + torch.randint(0, 256, (16384 * 48,), generator=g)).int().to(dev)
for _ in range(3):
    o = eng.gather_rows(nodes, idx)
dst = torch.empty_like(o)
for _ in range(3):
    dst.copy_(o)
torch.cuda.synchronize()
print("ok", o.numel() * 4)
