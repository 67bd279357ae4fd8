"""Times the bending-energy prior against the first-order prior on one device, alternating.

1. The `update_ms` stage (and the whole transition) of `irs_transition_timed` on the SSD / RegLoss_L2 workload of
   configs/synthetic_ssd_*_128.json for three engines: the bending prior (energy kernel first, then the bending update), the
   first-order prior as it runs by default (energy as a by-product of its update) and the first-order prior with
   `energy_in_update` = 0 (energy kernel first, as the bending prior has to).  `--reps` timed transitions per engine after
   `--warmup`, in rounds that alternate the engines; medians.  The algorithmic bytes of the two updates are the same (v, g, v_s read
   once, v written: 16 B per voxel and component).
2. The stateless operators: bending.bending_energy against ops.reg_energy, and bending.bending_energy_grad, device events around each call,
   medians, with the streaming floor of one read (energy) or one read and one write (gradient) of the field at the rate of a
   device-to-device copy measured here.

Prints one JSON line per (size, chains).  Run it under `rocprofv3 --kernel-trace --stats` for kernel times alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ir_sgmcmc_amd import bending, ops  # noqa: E402
from ir_sgmcmc_amd.data_loader import synthetic_pair  # noqa: E402
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine  # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps, warmup):
    """median seconds per call"""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e-3


def engines(N, C):
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = {k: v.unsqueeze(0).to(DEV).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).to(DEV).contiguous() for k, v in m1.items() if k != 'seg'}
    out = {}
    for name, kw, opts in (('bending', dict(diff_op='HessianOperator', w_reg=0.1), {}), ('first_order', dict(w_reg=1.4), {}),
                           ('first_order_energy_first', dict(w_reg=1.4), {'energy_in_update': 0})):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), no_chains=C, data_loss='SSD', virtual_decimation=False, **kw), DEV)
        for k, v in opts.items():
            eng.option(k, v)
        fd, md = eng.prepare(fixed, moving)
        out[name] = (eng, fd, md, torch.zeros(C, 3, N, N, N, device=DEV))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=str, nargs='+', default=['128x1', '128x2', '256x1'])
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    src = torch.empty(1 << 28, device=DEV)  # 1 GiB
    dst = torch.empty_like(src)
    copy_gbs = 2 * src.numel() * 4 / timed(lambda: dst.copy_(src), 20, 5) / 1e9
    del src, dst
    for case in args.cases:
        N, C = map(int, case.split('x'))
        engs = engines(N, C)
        for eng, fd, md, v in engs.values():
            for _ in range(args.warmup):
                eng.transition(fd, md, v)
            eng.flush()
        stage = {name: {'update_ms': [], 'total_ms': []} for name in engs}
        for _ in range(args.rounds):  # alternate the engines: other work shares the device
            for name, (eng, fd, md, v) in engs.items():
                for _ in range(args.reps):
                    t = eng.transition(fd, md, v, timed=True)
                    for k in stage[name]:
                        stage[name][k].append(t[k])
        rec = {'size': N, 'chains': C, 'copy_GBs': round(copy_gbs, 1)}
        for name, d in stage.items():
            per_round = [statistics.median(d['update_ms'][i * args.reps:(i + 1) * args.reps]) for i in range(args.rounds)]
            rec[name] = {'update_ms': round(statistics.median(d['update_ms']), 4), 'update_ms_rounds': [round(x, 4) for x in per_round],
                         'total_ms': round(statistics.median(d['total_ms']), 4)}
        field = engs['bending'][3]
        field.copy_(torch.rand(field.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)))
        t = {'bending_energy_ms': [], 'reg_energy_ms': [], 'bending_energy_grad_ms': []}
        for _ in range(args.rounds):
            t['bending_energy_ms'].append(timed(lambda: bending.bending_energy(field), args.reps, 3))
            t['reg_energy_ms'].append(timed(lambda: ops.reg_energy(field), args.reps, 3))
            t['bending_energy_grad_ms'].append(timed(lambda: bending.bending_energy_grad(field), args.reps, 3))
        rec.update({k: round(statistics.median(x) * 1e3, 4) for k, x in t.items()})
        rec['field_read_floor_ms'] = round(field.numel() * 4 / copy_gbs / 1e6, 4)
        print(json.dumps(rec), flush=True)
        del engs, field


if __name__ == '__main__':
    main()
