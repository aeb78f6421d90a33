#!/usr/bin/env python
"""The workload of the SAC learner's kernel trace: N fused updates at batch size B on fixed data, nothing else on the GPU.
  rocprofv3 --kernel-trace --stats -d OUT -o sac -- python tools/sac_learn_trace.py [--updates 100] [--batch 256]
profiles/sac_learn_kernel_stats.csv is the resulting kernel statistics table; launches per update = calls / updates."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paddlerobotics_amd.sac import DeviceSAC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    B, dev = args.batch, "cuda:0"
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    batch = (r(B, 49), r(B, 12), r(B), r(B, 49), torch.ones(B, device=dev))
    noise = (torch.randn(B, 12, generator=g).to(dev), torch.randn(B, 12, generator=g).to(dev))
    agent = DeviceSAC(49, max_batch=B, device=dev)
    for _ in range(args.updates):
        agent.learn(*batch, noise=noise)
    torch.cuda.synchronize()
    print("%d updates at B = %d done" % (args.updates, B))


if __name__ == "__main__":
    main()
