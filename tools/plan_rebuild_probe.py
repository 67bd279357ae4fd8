"""The rebuild path of the sparse plans: one engine at 256^3 whose mask alternates between two shapes under one pointer, every transition
-- every list of the data stage, the forward steps and the adjoint is cut again each time, the worst case for plan reuse
(csrc/adjoint_plan.hip).  Prints ms per transition with the mask alternating and with it held; run it with IRS_LIB pointing at each of
two builds, or behind `rocprofv3 --kernel-trace --stats --` for the plan kernels' own times.

    python tools/plan_rebuild_probe.py [--size 256] [--steps 40] [--plan 1]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from ir_sgmcmc_amd.data_loader import synthetic_pair
from ir_sgmcmc_amd.engine import TransitionEngine

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--plan', type=int, default=1, help='irs_sparse_plan_set: 1 reuse, 0 rebuild always, 2 / 3 the adjoint from the gradient')
a = ap.parse_args()
N, dev = a.size, torch.device('cuda', 0)
eng = TransitionEngine(bench.engine_config(N, 'gmm', 1234), dev)
eng.set_sparse_plan(a.plan)
f1, m1 = synthetic_pair((N, N, N), seed=0)
fixed, moving = eng.prepare({k: v.unsqueeze(0).to(dev) for k, v in f1.items() if k != 'seg'},
                            {k: v.unsqueeze(0).to(dev) for k, v in m1.items() if k != 'seg'})
eng.gmm_init(fixed, moving)
mask = fixed['mask']
shapes = [mask.clone(), torch.roll(mask, shifts=(6, -4), dims=(-3, -1)).contiguous()]   # the same shape, moved: the same work otherwise
v = bench.initial_velocity('identity', 0.0, N, dev).contiguous()
for name, period in (('alternating', 1), ('held', 10 ** 9)):
    times = []
    for rep in range(3):
        for t in range(6):
            mask.copy_(shapes[(t // period) % 2])
            eng.transition(fixed, moving, v)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for t in range(a.steps):
            mask.copy_(shapes[(t // period) % 2])      # (a 16 MB copy on the stream in both modes: the difference is the plans')
            eng.transition(fixed, moving, v)
        eng.flush()
        torch.cuda.synchronize(dev)
        times.append(1e3 * (time.perf_counter() - t0) / a.steps)
    print(name, 'ms per transition', [round(x, 4) for x in times], 'plan counters', eng.sparse_plan())
