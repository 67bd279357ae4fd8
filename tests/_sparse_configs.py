"""The cases of tests/test_gpu_sparse_configs.py -- the three sparse stages (data stage, forward squaring steps, adjoint squaring steps)
switched on together, in the configurations the four sparse test files leave at their defaults -- and the geometry each list must
have, formed from the mask alone with `run_lengths` of tests/test_gpu_sparse_data.py.  No GPU here: tests/test_sparse_configs_host.py
proves on the CPU that every list a case calls strictly sparse is strictly sparse at its reach.

Reaches (S: LCC half width, 0 for the SSD term; n: squaring steps; h_i: planned width of forward step i):
  warp hull      tile 64 x 8    3 S
  LCC map        tile 32 x 16   S
  data term      tile 32 x 16   2 S
  forward list k tile 64 x 8    3 S + h_{k+1} + ... + h_{n-1}     (adjoint_plan.h: plan_forward_reach)
  adjoint list k tile 32 x 8    2 S + n - k                        (adjoint_plan.h: plan_adjoint_reach0, one voxel less per list)"""
import torch

from tests.test_gpu_sparse_data import BIG, SMALL, columns, make_mask, planes_of, run_lengths

WARP_TILE, LCC_TILE, ADJ_TILE = (64, 8), (32, 16), (32, 8)
T = 5   # transitions per chain: the first has no published bounds (dense forward steps), four engage

BALL_WALK = ['ball', 'ball', 'corner_voxel', 'ball_shifted', 'ball_shifted']   # ball, then one voxel, then the ball elsewhere


ALL = ('warp', 'map', 'data_term', 'fwd_first', 'fwd_last', 'adj_last')


def case(name, dims, masks='ball', C=1, options=(), per_chain_fixed=False, strict=ALL, **cfg):
    """masks: one entry for all T transitions or a list of T; an entry is a mask kind (shared by the chains) or a tuple of kinds, one
    per chain.  strict: the lists that must march strictly fewer planes than D x tile columns, for every chain in every transition --
    'fwd_first' holds at width 1 per step, which the GPU test asserts alongside."""
    masks = list(masks) if isinstance(masks, list) else [masks] * T
    assert len(masks) == T
    return dict(id=name, dims=dims, masks=masks, C=C, options=tuple(options), per_chain_fixed=per_chain_fixed, strict=tuple(strict), cfg=cfg)


PER_CHAIN = ('warp', 'map', 'fwd_first', 'fwd_last', 'adj_last')    # the per-chain data term keeps its full columns
NO_FWD = ('warp', 'map', 'data_term', 'adj_last')
SSD_FFD = ('warp', 'adj_last')

CASES = [
    # a. lcc_s = 2: the S = 2 reaches and fills, clipped at three faces
    case('a-s2-ball', BIG, 'ball', lcc_s=2),
    case('a-s2-cut_ball', SMALL, 'cut_ball', lcc_s=2),
    case('a-s2-corner_voxel', SMALL, 'corner_voxel', lcc_s=2),
    case('a-s2-ball_walk', BIG, BALL_WALK, lcc_s=2),
    # b. lcc_s = 2, two chains with their own masks: the <2, true> batch list kernel
    case('b-s2-two_masks', SMALL, ('ball', 'cut_ball'), C=2, lcc_s=2),
    # c. per-chain dense data term behind a list-walking map (data_on == 2)
    case('c-C2-s1-data_batch=0', SMALL, ('ball', 'cut_ball'), C=2, options=(('data_batch', 0),), strict=PER_CHAIN),
    case('c-C2-s2-data_batch=0', SMALL, ('ball', 'cut_ball'), C=2, options=(('data_batch', 0),), strict=PER_CHAIN, lcc_s=2),
    case('c-C3-s1-data_batch=0', SMALL, 'ball_shifted', C=3, options=(('data_batch', 0),), strict=PER_CHAIN),
    case('c-C3-s2-data_batch=0', BIG, 'ball', C=3, options=(('data_batch', 0),), strict=PER_CHAIN, lcc_s=2),
    # d. SVFFD: sparse data stage and sparse adjoint, dense forward steps
    case('d-cps2-GMM', BIG, 'ball', strict=NO_FWD, cps=(2, 2, 2), lcc_s=2),
    case('d-cps4-GMM', SMALL, 'ball', strict=NO_FWD, cps=(4, 4, 4)),
    case('d-cps2-SSD', SMALL, 'ball', strict=SSD_FFD, cps=(2, 2, 2), data_loss='SSD', virtual_decimation=False),
    case('d-cps4-SSD', BIG, 'ball_shifted', strict=SSD_FFD, cps=(4, 4, 4), data_loss='SSD', virtual_decimation=False),
    # e. strides and builds of the list kernels
    case('e-K6', SMALL, 'ball', gmm_components=6),
    case('e-no_vd-s2', SMALL, 'cut_ball', virtual_decimation=False, lcc_s=2),
    case('e-fixed_per_chain-s2', SMALL, 'ball_shifted', C=2, per_chain_fixed=True, lcc_s=2),
    case('e-fuse_warp_bwd=0', BIG, 'ball', options=(('fuse_warp_bwd', 0),)),
    # f. five squaring steps at lcc_s = 2: reaches 2 S + n and 3 S + sum h for n != 12
    case('f-n5-s2', BIG, 'ball', no_steps=5, lcc_s=2),
    # g. the update and energy kernels behind a hull-limited forward pass
    case('g-lognormal', BIG, 'ball', reg_loss='RegLoss_LogNormal', reg_learnable=True),
    case('g-hessian-s2', SMALL, 'ball', diff_op='HessianOperator', lcc_s=2),
]


def half_width(c):
    """S of the reaches: the LCC half width, 0 for the pointwise SSD term"""
    return 0 if c['cfg'].get('data_loss', 'GMM') == 'SSD' else c['cfg'].get('lcc_s', 1)


def steps(c):
    return c['cfg'].get('no_steps', 12)


def mask_of(entry, dims):
    """(1 or C,1,D,H,W) bool"""
    kinds = entry if isinstance(entry, tuple) else (entry,)
    return torch.cat([make_mask(k, dims) for k in kinds]).contiguous()


def forward_reach(S, widths, k):
    return 3 * S + sum(widths[k + 1:])


def expected(m3, S, n, widths=None):
    """m3 (D,H,W) bool -> the planes each list must march, from the mask's geometry alone; widths: the planned widths of the forward
    steps (None: 1 each, the narrowest plan there is)"""
    widths = [1] * n if widths is None else list(widths)
    return {'warp': planes_of(run_lengths(m3, WARP_TILE, 3 * S)), 'map': planes_of(run_lengths(m3, LCC_TILE, S)),
            'data_term': planes_of(run_lengths(m3, LCC_TILE, 2 * S)),
            'forward': [planes_of(run_lengths(m3, WARP_TILE, forward_reach(S, widths, k))) for k in range(n)],
            'adjoint': [planes_of(run_lengths(m3, ADJ_TILE, 2 * S + n - k)) for k in range(n)]}


def totals(dims):
    """D x tile columns of the three tiles"""
    return {'warp': dims[0] * columns(dims, WARP_TILE), 'lcc': dims[0] * columns(dims, LCC_TILE), 'adjoint': dims[0] * columns(dims, ADJ_TILE)}


def strict_figures(exp, tot, n):
    """name of `strict` -> (planes, all planes)"""
    return {'warp': (exp['warp'], tot['warp']), 'map': (exp['map'], tot['lcc']), 'data_term': (exp['data_term'], tot['lcc']),
            'fwd_first': (exp['forward'][0], tot['warp']), 'fwd_last': (exp['forward'][n - 1], tot['warp']),
            'adj_last': (exp['adjoint'][n - 1], tot['adjoint'])}
