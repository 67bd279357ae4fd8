"""Measurements of the NGF data term (csrc/ngf_kernels.hip) through the stateless operators and the engine.

    python tools/ngf_bench.py --size 256 --chains 1 --calls 20      # HIP-event time per call of ngf_forward and ngf_backward
    python tools/ngf_bench.py --all                                 # 256^3 x 1 and 128^3 x 2 in one process
    python tools/ngf_bench.py --weight --size 128                   # the rule behind configs/synthetic_ngf_l2_128.json's weight
    python tools/ngf_bench.py --behaviour                           # 32^3, 40 noise-free transitions: NGF, MI and SSD chains

The timed calls run on the synthetic pair with the moving image inverted and biased (`moving_contrast: invert`, `moving_bias: 0.5`),
the fixed mask as the upstream weight.  Run the first form under `rocprofv3 --kernel-trace --stats` for the kernel times alone.
`--weight`: RMS of grad_v at the first transition with w_reg = 1e-20 (the data half), lr 0.4, seed 0, for the SSD config on its own
pair and for NGF at weight 1 on the inverted, biased pair; the config's weight is the ratio.  `--behaviour`: the chain's own data
term first -> last, the hard-bin MI of ops.image_similarity (32 bins) between the fixed and the warped moving image, and the Dice
of the three labels between the fixed segmentation and the moving one warped by the transformation of that transition."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ir_sgmcmc_amd import mi, ngf, ops  # noqa: E402
from ir_sgmcmc_amd.data_loader import synthetic_pair  # noqa: E402
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine  # noqa: E402

DEV = 'cuda:0'


def pair(size, **kw):
    f, m = synthetic_pair((size,) * 3, seed=0, **kw)
    dev = lambda d: {k: v.unsqueeze(0).to(DEV).contiguous() for k, v in d.items() if k != 'seg'}
    return dev(f), dev(m)


def timings(size, chains, calls):
    fixed, moving = pair(size, moving_contrast='invert', moving_bias=0.5)
    eps = ngf.ngf_edge_parameters(fixed['im'], moving['im'], fixed['mask'], moving['mask'])
    m = moving['im'].repeat(chains, 1, 1, 1, 1).contiguous()
    u = fixed['mask'].to(torch.float32)
    out = ngf.ngf_forward(fixed['im'], m, *eps, u)
    ngf.ngf_backward(out['coef'])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(calls):
        out = ngf.ngf_forward(fixed['im'], m, *eps, u)
    ev[1].record()
    for _ in range(calls):
        ngf.ngf_backward(out['coef'])
    ev[2].record()
    torch.cuda.synchronize()
    return {'size': size, 'chains': chains, 'eps': eps, 'sum_ud': float(out['sums'][0]), 'fwd_us': 1e3 * ev[0].elapsed_time(ev[1]) / calls,
            'bwd_us': 1e3 * ev[1].elapsed_time(ev[2]) / calls}


STRUCTURES = {'outer': 10, 'middle': 16, 'inner': 49}   # the label values of synthetic_pair's three nested shells


def dice(seg_fixed, seg_warped):
    out = {}
    for key, label in STRUCTURES.items():
        f, w = seg_fixed == label, seg_warped == label
        out[key] = float(2.0 * (f & w).sum() / (f.sum() + w.sum()))
    return out


def first_gradient(size, fixed, moving, **cfg):
    eng = TransitionEngine(EngineConfig(dims=(size,) * 3, virtual_decimation=False, w_reg=1e-20, lr=0.4, seed=0, **cfg), DEV)
    fd, md = eng.prepare(fixed, moving)
    out = {'grad_v': torch.empty(1, 3, size, size, size, device=DEV)}
    eng.transition(fd, md, torch.zeros(1, 3, size, size, size, device=DEV), None, None, None, out)
    g = out['grad_v'].double()
    return [float(g.pow(2).mean().sqrt()), eng.scalars()['data_term'][0], float(g.abs().max())]


def weight(size):
    res = {'ssd': first_gradient(size, *pair(size), data_loss='SSD')}
    fixed, moving = pair(size, moving_contrast='invert', moving_bias=0.5)
    eps = ngf.ngf_edge_parameters(fixed['im'], moving['im'], fixed['mask'], moving['mask'])
    ngf_cfg = dict(data_loss='NGF', ngf_fixed_eps=eps[0], ngf_moving_eps=eps[1])
    res['eps'] = eps
    res['ngf'] = first_gradient(size, fixed, moving, ngf_weight=1.0, **ngf_cfg)
    res['weight'] = res['ssd'][0] / res['ngf'][0]
    res['ngf_at_weight'] = first_gradient(size, fixed, moving, ngf_weight=round(res['weight'], 4), **ngf_cfg)
    return res


def behaviour(size=32, transitions=40, ngf_weight=1.0):
    fixed, moving = pair(size, moving_contrast='invert', moving_bias=0.5)
    f1, m1 = synthetic_pair((size,) * 3, seed=0, moving_contrast='invert', moving_bias=0.5)
    seg_f, seg_m = f1['seg'].unsqueeze(0).to(DEV).contiguous(), m1['seg'].unsqueeze(0).to(DEV).contiguous()
    eps = ngf.ngf_edge_parameters(fixed['im'], moving['im'], fixed['mask'], moving['mask'])
    f_range, m_range = mi.mi_ranges(fixed['im'], moving['im'], fixed['mask'])
    chains = {'NGF': dict(data_loss='NGF', ngf_weight=ngf_weight, ngf_fixed_eps=eps[0], ngf_moving_eps=eps[1]),
              'MI': dict(data_loss='MI', mi_fixed_range=f_range, mi_moving_range=m_range), 'SSD': dict(data_loss='SSD')}
    rows = {}
    for key, cfg in chains.items():
        eng = TransitionEngine(EngineConfig(dims=(size,) * 3, virtual_decimation=False, uniform_noise=0.0, lr=0.4, seed=0, **cfg), DEV)
        fd, md = eng.prepare(fixed, moving)
        v, zero = torch.zeros(1, 3, size, size, size, device=DEV), torch.zeros(1, 3, size, size, size, device=DEV)
        out = {'im_moving_warped': torch.empty(1, 1, size, size, size, device=DEV),
               'transformation': torch.empty(1, 3, size, size, size, device=DEV)}
        terms, sims, dices = [], [], [dice(seg_f, seg_m)]   # (the Dice before any transition; then of the first and the last)
        for t in range(transitions):
            eng.transition(fd, md, v, None, zero, None, out)
            terms.append(eng.scalars()['data_term'][0])
            if t in (0, transitions - 1):
                stats = ops.image_similarity(fixed['im'], out['im_moving_warped'], fixed['mask'], 32)['stats']
                sims.append(float(stats[0, ops.SIMILARITY_COLUMNS.index('mi')]))
                dices.append(dice(seg_f, ops.warp(seg_m, out['transformation'])))
        rows[key] = {'data_term': [terms[0], terms[-1]], 'hard_bin_mi': sims, 'dice': dices, 'max_abs_v': float(v.abs().max())}
    return {'size': size, 'transitions': transitions, 'eps': eps, **rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=256)
    p.add_argument('--chains', type=int, default=1)
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--all', action='store_true')
    p.add_argument('--weight', action='store_true')
    p.add_argument('--behaviour', action='store_true')
    a = p.parse_args()
    if a.weight:
        print(json.dumps(weight(a.size)))
    elif a.behaviour:
        print(json.dumps(behaviour()))
    elif a.all:
        for size, chains in ((256, 1), (128, 2)):
            print(json.dumps(timings(size, chains, a.calls)), flush=True)
    else:
        print(json.dumps(timings(a.size, a.chains, a.calls)))


if __name__ == '__main__':
    main()
