"""Host side of tests/test_gpu_autograd_modules.py, on the CPU: (1) the restatements of tests/_autograd_modules.py are plain float64
autograd of the oracle ops, to 1e-12 relative; (2) the pure-torch backward code of the layer -- _EnergyGrad.backward, SGLD.backward,
the cotangent assembly of _SVFExp.backward up to the _ops.svf_exp_bwd call -- is the same thing when called with a stub ctx on
float64 tensors; (3) every measured tolerance is at least 8x the deviation of the float32 CPU oracle, and the two closed-form ones hold
it; (4) each mistake the layer can make, planted on the REFERENCE side, exceeds the tolerance at least 100x on the chosen inputs;
(5) the inputs meet their conditions: no float32 rounding changes a cell of the warp case, the float32 oracle of the _SVFExp cases
excludes no element, and its 4-step runs have no isolated cell flip that would blow the tolerance up."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ops as O
from tests import _autograd_modules as A

F64, F32 = A.F64, A.F32
REL = 1e-12
SVF_CASES = [(d, n, m) for d in A.SHAPES for n in (4, 12) for m in A.SVF_MODES]
ident = lambda x: 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x)


def close(a, b, rel=REL):
    a, b = a.detach().to(F64), b.detach().to(F64)
    return float((a - b).abs().max()) <= rel * float(b.abs().max())


def excess(wrong, band):
    """by how many tolerances the mistaken reference misses the right one, at its worst element"""
    return float((wrong.detach().to(F64) - band.ref).abs().max()) / band.tol


# ------------------------------------------------------------------------------------------------------------------------------
# 1  the restatements are plain float64 autograd of the oracle ops
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_sgld_restatement_is_the_oracle(dims):
    c = A.sgld_case(dims)
    v = c['v'].to(F64).requires_grad_(True)
    out = O._SGLD.apply(v, c['sigma'].to(F64), A.TAU, c['eps'].to(F64))
    g, = torch.autograd.grad(out, v, c['cot'].to(F64))
    assert close(c['out'], out) and close(c['grad'], g)
    assert bool((c['v'] * c['eps'] > 0).all()) and float(c['sigma'].min()) >= 0.5 and float(c['sigma'].max()) <= 1.5
    assert bool((c['out'].abs() >= c['v'].abs().to(F64)).all())         # nothing cancels: |value| bounds both addends
    assert float((c['sigma'].max() - c['sigma'].min())) > 0.9             # a non-constant sigma field


@pytest.mark.parametrize('dims,no_steps,mode', SVF_CASES, ids=ident)
def test_svf_restatement_is_plain_autograd(dims, no_steps, mode):
    r, p = A.svf_oracle(dims, no_steps, mode), A.svf_oracle(dims, no_steps, mode, plain=True)
    assert close(r['grad_v'], p['grad_v'])
    d = A.svf_case(dims)['v']
    assert abs(float(d.abs().max()) - 1.5) < 1e-6


@pytest.mark.parametrize('transformation', [False, True])
@pytest.mark.parametrize('dims', A.ENERGY_GRAD_SHAPES, ids=ident)
def test_energy_grad_restatement_is_plain_autograd(dims, transformation):
    c, o = A.energy_grad_case(dims), A.energy_grad_oracle(dims, transformation)
    nabla, grad = A.energy_grad_restated(c['v'].to(F64), c['cot'].to(F64), transformation)
    assert close(nabla, o['nabla']) and close(grad, o['grad_v'])


@pytest.mark.parametrize('case', A.REG_CASES)
@pytest.mark.parametrize('dims', A.REG_SHAPES, ids=ident)
def test_regulariser_restatement_is_plain_autograd(dims, case):
    r, p = A.reg_oracle(case, dims), A.reg_oracle(case, dims, plain=True)
    assert set(r) == set(p)
    for k in r:
        assert close(r[k], p[k]), k
    y = r['log_y'].exp()
    assert float(y[1] / y[0]) > 10.0 and float(y[2] / y[1]) > 10.0         # amplitudes 1 : 4 : 16 -> energies 1 : 16 : 256


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('dims', A.LCC_SHAPES, ids=ident)
def test_lcc_reference_is_the_oracle_map(dims, s):
    c = A.lcc_case(dims, s)
    m = c['moving'].to(F64).requires_grad_(True)
    z = O.lcc_map(c['fixed'].to(F64).expand_as(m), m, s)
    g, = torch.autograd.grad(z, m, c['g_z'].to(F64))
    assert close(c['z'], z, 1e-10) and close(c['grad_moving'], g, 1e-10)


@pytest.mark.parametrize('case', list(A.VI_CASES))
def test_vi_restatement_is_the_oracle_step(case):
    r, p = A.vi_oracle(case), A.vi_oracle(case, plain=True)
    assert list(r) == ['grad_' + k for k in A.VI_FIELDS + A.vi_param_names(case)] and list(r) == list(p)
    for k in r:
        assert close(r[k], p[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# 2  the layer's pure-torch backward code, called directly with a stub ctx on float64 tensors
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transformation', [False, True])
@pytest.mark.parametrize('dims', A.ENERGY_GRAD_SHAPES, ids=ident)
def test_energy_grad_backward_is_the_adjoint(dims, transformation):
    from ir_sgmcmc_amd.utils.diff_op import _EnergyGrad
    c, o = A.energy_grad_case(dims), A.energy_grad_oracle(dims, transformation)
    ctx = SimpleNamespace(shape=c['v'].shape, transformation=transformation)
    grad, none = _EnergyGrad.backward(ctx, c['cot'].to(F64))
    assert none is None and close(grad, o['grad_v'])


@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_sgld_backward_scales_by_sigma_squared(dims):
    from ir_sgmcmc_amd.utils.functions import SGLD
    c = A.sgld_case(dims)
    out = SGLD.backward(SimpleNamespace(saved_tensors=(c['sigma'].to(F64),)), c['cot'].to(F64))
    assert out[1:] == (None, None, None) and close(out[0], c['grad'])


@pytest.mark.parametrize('mode', A.SVF_MODES)
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_svf_backward_assembles_the_cotangent(dims, mode, monkeypatch):
    from ir_sgmcmc_amd.utils import transformation as TR
    c = A.svf_case(dims)
    seen = {}
    monkeypatch.setattr(TR._ops, 'svf_exp_bwd', lambda v, steps, g: seen.update(v=v, steps=steps, g=g) or 'g_v')
    v, steps = c['v'].to(F64), torch.zeros(4, *c['v'].shape, dtype=F64)
    g_t = c['g_t'].to(F64) if mode in ('transformation', 'both') else None
    g_disp = c['g_disp'].to(F64) if mode in ('displacement', 'both') else None
    keep = [None if g is None else g.clone() for g in (g_t, g_disp)]
    assert TR._SVFExp.backward(SimpleNamespace(saved_tensors=(v, steps)), g_t, g_disp) == ('g_v', None)
    assert seen['v'] is v and seen['steps'] is steps and seen['g'].is_contiguous()
    assert close(seen['g'], A.svf_cotangent(g_t, g_disp, dims))
    for g, k in zip((g_t, g_disp), keep):                                   # the incoming cotangents are left as they were
        assert g is None or torch.equal(g, k)


# ------------------------------------------------------------------------------------------------------------------------------
# 3  the tolerances against the float32 CPU oracle
# ------------------------------------------------------------------------------------------------------------------------------
def all_bands():
    for d, n, m in SVF_CASES:
        yield f'svf {d} {n} {m}', A.svf_bands(d, n, m)
    for d in A.SHAPES:
        yield f'warp {d}', A.warp_bands(d)
        for s in (1, 3):
            yield f'sobolev {d} {s}', A.measured(A.sobolev_oracle, d, s)
    for d in A.ENERGY_GRAD_SHAPES:
        for tr in (False, True):
            yield f'energy_grad {d} {tr}', A.energy_grad_bands(d, tr)
    for d in A.REG_SHAPES:
        for case in A.REG_CASES:
            yield f'reg {d} {case}', A.reg_bands(case, d)
    for form in ('log_det', 'sample'):
        yield f'entropy {form}', A.entropy_bands(A.SHAPES[0], form)
    for case in A.VI_CASES:
        yield f'vi {case}', A.vi_bands(case)


def test_measured_tolerances_are_eight_times_the_float32_oracle():
    n = 0
    for name, bands in all_bands():
        for k, b in bands.items():
            dev = float((b.f32 - b.ref).abs().max())
            assert dev == b.E and b.tol >= 8.0 * dev and b.tol >= A.FLOOR * float(b.ref.abs().max()), (name, k)
            assert b.tol == max(8.0 * b.E, A.FLOOR * float(b.ref.abs().max())), (name, k)
            assert float(b.ref.abs().max()) > 0.0 and b.tol < 0.02 * float(b.ref.abs().max()), (name, k, b.tol)   # a tolerance, not a blank cheque
            n += 1
    assert n > 100


@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_closed_form_tolerance_of_sgld_holds_the_float32_oracle(dims):
    """4 U |value| is the issue's own bound, not a measured one: the float32 oracle has to be inside it, in either order of
    evaluation (the deviation is about half of it, so there is no factor of 8 to spare here)"""
    c = A.sgld_case(dims)
    amp = (2.0 * A.TAU) ** 0.5
    for out in (O.langevin_perturb(c['v'], c['sigma'], A.TAU, c['eps']), c['v'] + (torch.tensor(amp) * c['sigma']) * c['eps']):
        assert float(A.units(out, c['out'], c['tol_out']).max()) <= 1.0
    assert float(A.units(c['cot'] * c['sigma'] ** 2, c['grad'], c['tol_grad']).max()) <= 1.0


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('dims', A.LCC_SHAPES, ids=ident)
def test_closed_form_tolerance_of_the_lcc_adjoint_is_eight_times_the_float32_oracle(dims, s):
    c = A.lcc_case(dims, s)
    m = c['moving'].clone().requires_grad_(True)
    z = O.lcc_map(c['fixed'].expand_as(m), m, s)
    g, = torch.autograd.grad(z, m, c['g_z'])
    assert float(A.units(g, c['grad_moving'], c['tol_grad']).max()) <= 1.0 / 8.0
    assert float(A.units(z, c['z'], c['tol_z']).max()) <= 1.0
    assert float(c['tol_grad'].min()) > 0.0 and float((c['tol_grad'] / c['grad_moving'].abs().max()).max()) < 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# 4  planted mistakes: each misses the tolerance by 100x or more
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_mistake_sigma_for_sigma_squared(dims):
    c = A.sgld_case(dims)
    wrong = A.sgld_grad(c['sigma'].to(F64), c['cot'].to(F64), 'sigma_for_sigma2')
    assert float(A.units(wrong, c['grad'], c['tol_grad']).max()) >= 100.0


@pytest.mark.parametrize('mistake', ['scale_left_out', 'scale_W_D_swapped'])
@pytest.mark.parametrize('dims,no_steps,mode', [c for c in SVF_CASES if c[2] != 'transformation'], ids=ident)
def test_mistakes_in_the_displacement_scale(dims, no_steps, mode, mistake):
    wrong = A.svf_oracle(dims, no_steps, mode, mistake=mistake)['grad_v']
    assert excess(wrong, A.svf_bands(dims, no_steps, mode)['grad_v']) >= 100.0


@pytest.mark.parametrize('dims', A.ENERGY_GRAD_SHAPES, ids=ident)
def test_mistakes_in_the_adjoint_of_the_differences(dims):
    c = A.energy_grad_case(dims)
    v, cot = c['v'].to(F64), c['cot'].to(F64)
    for tr in (False, True):
        wrong = A.energy_grad_restated(v, cot, tr, 'last_plane_dropped')[1]
        assert excess(wrong, A.energy_grad_bands(dims, tr)['grad_v']) >= 100.0
    wrong = A.energy_grad_restated(v, cot, True, 'spacing_axes_swapped')[1]
    assert excess(wrong, A.energy_grad_bands(dims, True)['grad_v']) >= 100.0


@pytest.mark.parametrize('case', A.REG_CASES)
@pytest.mark.parametrize('dims', A.REG_SHAPES, ids=ident)
def test_mistake_one_chains_g_y_for_all(dims, case):
    wrong = A.reg_oracle(case, dims, mistake='g_y_of_chain_0')['grad_v']
    assert excess(wrong, A.reg_bands(case, dims)['grad_v']) >= 100.0


@pytest.mark.parametrize('mistake', ['one_sample', 'doubled'])
@pytest.mark.parametrize('case', list(A.VI_CASES))
def test_mistakes_in_the_vi_gradient(case, mistake):
    wrong, bands = A.vi_oracle(case, mistake=mistake), A.vi_bands(case)
    for k in A.VI_FIELDS:
        assert excess(wrong['grad_' + k], bands['grad_' + k]) >= 100.0, k
        if mistake == 'doubled':
            assert abs(A.norm_ratio(wrong['grad_' + k], bands['grad_' + k].ref) - 1.0) > 1e3 * A.NORM_RTOL
    # the scalar parameters see the regulariser through log y alone, which the two samples of a pair nearly share: half a pair
    # misses their tolerance too, by less (loc 550x, log_scale 20x)
    for k in A.vi_param_names(case):
        assert excess(wrong['grad_' + k], bands['grad_' + k]) >= (100.0 if mistake == 'doubled' else 10.0), k


@pytest.mark.parametrize('case', list(A.VI_CASES))
def test_float32_oracle_meets_the_norm_bound(case):
    for k in A.VI_FIELDS:
        b = A.vi_bands(case)['grad_' + k]
        assert abs(A.norm_ratio(b.f32, b.ref) - 1.0) <= A.NORM_RTOL / 8.0, k


# ------------------------------------------------------------------------------------------------------------------------------
# 5  the conditions on the inputs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims,no_steps,mode', SVF_CASES, ids=ident)
def test_float32_oracle_excludes_no_element(dims, no_steps, mode):
    b = A.svf_bands(dims, no_steps, mode)['grad_v']
    dev = (b.f32 - b.ref).abs()
    assert int((dev > b.tol).sum()) == 0
    if no_steps == 4:       # no isolated cell flip: the largest deviation is of the size of all the others
        assert b.E <= 4.0 * float(torch.quantile(dev.flatten(), 0.999))


@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_warp_positions_keep_their_cell_in_float32(dims):
    c = A.warp_case(dims)
    n = c['n'].to(F32)
    i32 = ((c['t'] + 1.0) / 2.0) * (n - 1.0)                                   # the sampler's own float32 coordinate pipeline
    assert float((i32.to(F64) - c['p']).abs().max()) < 1e-4
    inside = ~c['outside']
    assert bool((i32.floor().to(F64) == c['p'].floor())[inside].all())
    frac = c['p'] - c['p'].floor()
    assert float(frac.min()) >= 0.25 and float(frac.max()) <= 0.75
    out32 = (i32 <= 0) | (i32 >= n - 1.0)
    assert torch.equal(out32, c['outside'])
    for ch, ax in enumerate((-1, -2, -3)):                                      # every face has voxels pushed out along its own axis
        o = c['outside'][:, ch]
        assert bool(o.narrow(ax, 0, 1).any()) and bool(o.narrow(ax, dims[ax] - 1, 1).any())
        assert bool((~o).narrow(ax, 0, 1).any()) and bool((~o).narrow(ax, dims[ax] - 1, 1).any())
    g = A.warp_bands(dims)['grad_t']
    assert float(g.ref[c['outside']].abs().max()) == 0.0 and float(g.f32[c['outside']].abs().max()) == 0.0
    assert float(g.ref[inside].abs().min()) > 0.0
