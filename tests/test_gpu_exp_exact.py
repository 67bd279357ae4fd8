"""The scaling-and-squaring steps and their adjoints (csrc/exp_kernels.hip) held bit for bit to the fp64 reference on the exact
("dyadic") cases of tests/_exact_cases.py ("Numerics note (exact cases)"); tests/test_exact_cases_host.py proves on
the CPU, for every case used here, that fp32 and fp64 agree bit for bit, which classes of position a case holds and which kernel
its chains select: floor(max|d_k|) + 1 per chain is 1 (radius-1 ring / gather), 2 (radius-2) or 3 and more (global-memory taps /
the any-radius fixed-point adjoint).  Every comparison is torch.equal; the launch shapes are the library's own, plus the switch
values tests/test_gpu_ops.py already sets.  The output kernel's vectorised form is held to its two roundings.  GPU only."""
import pytest
import torch

from ir_sgmcmc_amd import ops as G
from ir_sgmcmc_amd._lib import option_set
from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from tests import _exact_cases as X
from tests.test_gpu_ops import dev, smooth_field
from tests.test_gpu_warp_exact import assert_same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

_REF = {}


def _shared(key, make):
    """a case and its fp64 reference, computed once and shared (never modified)"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _chain(dims, name):
    def make():
        case = X.velocity_case(dims, name)
        return (case,) + X.chain_reference(case.v, case.no_steps, torch.float64)[:3]
    return _shared(('chain', tuple(dims), name), make)


def _step(dims):
    def make():
        case = X.step_case(dims)
        out, adj = X.step_reference(case.D, case.G, torch.float64, explicit=True)
        scale = torch.tensor([1.0 / (n - 1) for n in X.axis_sizes(dims)], dtype=torch.float64).view(1, 3, 1, 1, 1)
        v = 2.0 * X.O.to_voxels(case.D)          # fp32, exact: d_0 of a one-step chain of this velocity is D
        gv = X.chain_reference(v, 1, torch.float64, case.G)[3]
        return case, v, gv, adj * scale, out
    return _shared(('step', tuple(dims)), make)


# ---------------------------------------------------------------- a. forward chain
# None: the library's own choice; the others are the (fwd_rows1, fwd_pf) of test_svf_exp_forward_radius1_variants_agree
FWD_SETTINGS = [None, (0, 2), (1, 2), (1, 1)]


@pytest.mark.parametrize('setting', FWD_SETTINGS, ids=['default', 'rows2', 'rows1-pf2', 'rows1-pf1'])
@pytest.mark.parametrize('name', ['one step', 'two steps', 'two steps, far'])
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_forward_chain_is_exact(dims, name, setting):
    """svf_exp_fwd: every d_k, the transformation and the displacement.  The stateless operator has no bound of d_k and runs the
    radius-1 ring for every chain -- the prescaling instantiation at step 0, the plain one behind it -- whose taps leave the ring
    for global memory in the chains that reach 1, 3, 6 and up to 24 voxels."""
    case, t64, u64, steps64 = _chain(dims, name)
    try:
        if setting is not None:
            option_set('fwd_rows1', setting[0])
            option_set('fwd_pf', setting[1])
        t, u, steps = G.svf_exp_fwd(dev(case.v), case.no_steps)
        torch.cuda.synchronize()
    finally:
        option_set('fwd_rows1', -1)
        option_set('fwd_pf', 2)
    assert steps.shape == (case.no_steps, case.C, 3, *dims)
    for k in range(case.no_steps):
        assert_same(f'd_{k + 1}', steps[k], steps64[k + 1])
    assert_same('transformation', t, t64)
    assert_same('displacement', u, u64)


# ---------------------------------------------------------------- b, c, d. adjoint step
@pytest.mark.parametrize('coarse_box', [1, 0])
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_prescaling_adjoint_step_is_exact(dims, coarse_box):
    """svf_exp_bwd of a one-step chain with v = 2 to_voxels(D): d_0 = D, so the five chains select, in ONE call of the prescaling
    instantiation, the radius-1 gather (max|d| = 3/4), the radius-2 gather (exactly 1, and 7/4) and the any-radius kernel (exactly
    2, and up to 3 voxels past every face).  grad_v = adjoint / (n_c - 1): a power of two.  With the coarse source boxes and with
    the plain ones, each against the reference."""
    case, v, gv64, _, d1 = _step(dims)
    steps = G.svf_exp_fwd(dev(v), 1, want_outputs=False)[2]
    assert_same('d_1', steps[0], d1)
    try:
        option_set('coarse_box', coarse_box)
        gv = G.svf_exp_bwd(dev(v), steps, dev(case.G))
        torch.cuda.synchronize()
    finally:
        option_set('coarse_box', 1)
    assert_same('grad_v', gv, gv64)


@pytest.mark.parametrize('coarse_box', [1, 0])
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_plain_adjoint_step_is_exact(dims, coarse_box):
    """The plain instantiation of the three adjoint kernels on one injected field: a two-step call with v = 0 and steps[0] = D (the
    operator reads d_1 from `steps` and measures its bound itself; steps[1] = d_2 is not read).  Step 1 is the adjoint at D; step
    0, at d_0 = 0, doubles it exactly (host: test_the_adjoint_of_a_step_at_zero_doubles_its_input); the prescale of two steps is
    2 / (n_c - 1) / 4: g_v[c] = adjoint(D)[c] / (n_c - 1), against the explicit restatement."""
    case, _, _, want, _ = _step(dims)
    steps = torch.stack([case.D, case.D.flip(0)])
    try:
        option_set('coarse_box', coarse_box)
        gv = G.svf_exp_bwd(dev(torch.zeros_like(case.D)), dev(steps), dev(case.G))
        torch.cuda.synchronize()
    finally:
        option_set('coarse_box', 1)
    assert_same('g_v', gv, want)


# ---------------------------------------------------------------- e. the forward steps inside a transition of the engine
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_engine_forward_steps_are_exact(dims):
    """The radius-2 forward ring and the interleaved layout of d_1 run only inside a context, which selects per chain from the
    bound the step before published: max|d_1| below 1 (radius-1 ring), in [1, 2) (radius-2 ring) and beyond (radius-2 ring with
    global-memory taps).  No smoothing, no jitter, zero noise: the state the steps start from is v itself.  A transition that is
    asked for the fields runs its forward steps dense whatever the switch says: the same bits with the sparse forward steps off."""
    case, t64, u64, _ = _chain(dims, 'engine')
    C = case.C
    g = torch.Generator().manual_seed(11)
    fixed = {'im': dev(torch.rand(1, 1, *dims, generator=g)), 'mask': dev(torch.ones(1, 1, *dims, dtype=torch.bool))}
    moving = {'im': dev(torch.rand(1, 1, *dims, generator=g))}
    for sparse in (True, False):
        cfg = EngineConfig(dims=dims, no_chains=C, no_steps=2, sobolev_s=0, uniform_noise=0.0, data_loss='SSD', virtual_decimation=False,
                           lr=0.05, seed=3)
        eng = TransitionEngine(cfg, DEV)
        eng.set_sparse_forward(sparse)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = dev(case.v).clone()
        out = {n: torch.full((C, 3, *dims), float('nan'), device=DEV) for n in ('curr_state', 'displacement', 'transformation')}
        eng.transition(fd, md, v, None, torch.zeros_like(v), None, out)
        eng.flush()
        assert eng.recovered_transitions == 0
        assert_same('curr_state', out['curr_state'], case.v.double())   # precondition: the steps started from v
        assert_same(f'transformation (sparse forward {sparse})', out['transformation'], t64)
        assert_same(f'displacement (sparse forward {sparse})', out['displacement'], u64)
        del eng


# ---------------------------------------------------------------- f. the output kernel, scalar and four voxels per thread
@pytest.mark.parametrize('dims', [(3, 6, 128), (2, 5, 132), (2, 5, 130)])
def test_outputs_kernel_rounds_once_per_operation(dims):
    """svf_outputs_x4_kernel takes W % 4 == 0 and W >= 128 -- (3, 6, 128) with H % 4 == 2, (2, 5, 132) with H % 4 == 1 and a
    last x-block of 4 lanes -- and svf_outputs_kernel the rest, (2, 5, 130).  From the GPU's own last step d:

    displacement = fl(fl(d (n_c - 1)) 0.5): two correctly rounded products, which the CPU repeats: torch.equal.

    transformation = fl(lin + d), lin the fp32 table of linspace(-1, 1, n).  Against id + d with id in float64: the table entry is
    within 2^-24 of id (one rounding at |id| <= 1 is 2^-25; torch's fp32 linspace, which the table repeats, measures 1.06 * 2^-25 at
    these n -- host: test_the_identity_table_is_one_rounding_from_linspace), and the sum rounds once, by at most 2^-24 |t|:
    |t - (id + d)| <= 2^-24 (1 + |t|) <= 2^-23 max(1, |t|)."""
    v = smooth_field(2, dims, 3.0, 41)
    t, u, steps = G.svf_exp_fwd(dev(v), 2)
    d = steps[-1].cpu()
    assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0
    nm1 = torch.tensor([float(n - 1) for n in X.axis_sizes(dims)]).view(1, 3, 1, 1, 1)
    assert_same('displacement', u, (d * nm1) * 0.5)
    ident = torch.stack([torch.linspace(-1, 1, n, dtype=torch.float64).view(*[-1 if i == a else 1 for i in range(3)]).expand(*dims)
                         for a, n in ((2, dims[2]), (1, dims[1]), (0, dims[0]))]).unsqueeze(0)
    want = ident + d.double()
    err = (t.cpu().double() - want).abs()
    bound = 2.0 ** -23 * want.abs().clamp(min=1.0)
    worst = float((err / bound).max())
    print('transformation: worst error / bound', worst)
    assert worst <= 1.0, (worst, (err > bound).nonzero()[:8].tolist())
