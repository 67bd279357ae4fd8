"""The float64 restatement of the LNCC data term (tests/_lncc.py) checked on the CPU: its gradient against float64 autograd of the
definition and against central differences, its tolerance against a float32 evaluation in the kernel's order (which has to stay
under a third of it) and against the mistakes it is there to catch (each has to exceed it somewhere): the padding's fold left out on
one of the six faces, the t term omitted, a ring not primed at a segment seam.  The upstream weight is a mask of ones, which touches
every face: under synthetic_pair's interior mask the fold mistakes change nothing (checked below)."""
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from tests import _data_gradient as G
from tests import _lncc as N

F64 = torch.float64
DIMS = (9, 10, 11)
CASES = [(1, 0.0), (2, 0.0), (1, 0.5), (2, 0.5)]
IDS = [f'r{r}-raised{b}' for r, b in CASES]


def inputs(r, raised, dims=DIMS):
    fixed, moving = N.images(dims, 1, raised)
    return fixed[0, 0], moving[0, 0], torch.ones(dims)


def test_switch_value():
    assert L.IRS_DATA_LNCC == 3 and L.IRS_DATA_GMM_LCC == 0 and L.IRS_DATA_SSD == 1


@pytest.mark.parametrize('r,raised', CASES, ids=IDS)
def test_gradient_equals_autograd(r, raised):
    f, m, u = inputs(r, raised)
    u = torch.randn(DIMS, generator=torch.Generator().manual_seed(2), dtype=F64)   # any upstream weight, negative entries too
    ref = N.reference(f, m, u, r)
    auto = N.autograd_gradient(f, m, u, r)
    assert float((ref['g'] - auto).abs().max()) <= 1e-12 * float(auto.abs().max())


def test_gradient_equals_central_differences():
    r, dims = 1, (5, 6, 7)
    f, m, _ = inputs(r, 0.0, dims)
    u = torch.rand(dims, generator=torch.Generator().manual_seed(3), dtype=F64) + 0.5
    g = N.reference(f, m, u, r)['g']
    loss = lambda mm: float(N.loss_sums(u.unsqueeze(0), N.terms(f, mm, u, r)['d'].unsqueeze(0)))
    h = 1e-5
    for idx in [(0, 0, 0), (4, 5, 6), (2, 3, 3), (0, 3, 6), (4, 0, 2), (1, 5, 0)]:
        mp, mn = m.to(F64).clone(), m.to(F64).clone()
        mp[idx] += h
        mn[idx] -= h
        fd = (loss(mp) - loss(mn)) / (2 * h)
        assert abs(fd - float(g[idx])) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, float(g[idx]))


@pytest.mark.parametrize('r,raised', CASES, ids=IDS)
def test_float32_in_kernel_order_uses_under_a_third(r, raised):
    f, m, u = inputs(r, raised)
    ref, got = N.reference(f, m, u, r), N.float32_in_kernel_order(f, m, u, r)
    for k in ('d', 'p', 'q', 't', 'g'):
        used = float(((got[k].to(F64) - ref[k]).abs() / ref['tol'][k]).max())
        assert used < 1.0 / 3.0, (k, used)


MISTAKES = [(f'fold_axis{a}_end{e}', dict(drop=((a, e),))) for a in (-3, -2, -1) for e in (0, 1)] + [
    ('t_omitted', dict(no_t=True)), ('seam_unprimed', dict(seam=4))]


@pytest.mark.parametrize('r,raised', CASES, ids=IDS)
@pytest.mark.parametrize('name,kw', MISTAKES, ids=[n for n, _ in MISTAKES])
def test_each_mistake_exceeds_the_tolerance(name, kw, r, raised):
    f, m, u = inputs(r, raised)
    ref = N.reference(f, m, u, r)
    wrong = N.gradient(f, m, ref['p'], ref['q'], ref['t'], r, **kw)
    assert float(((wrong - ref['g']).abs() / ref['tol']['g']).max()) > 10.0


def test_interior_mask_hides_the_fold_mistakes():
    """why the cases above use a mask of ones: under synthetic_pair's mask, which stays away from the faces, p, q and t vanish within
    the window's reach of every face and a dropped fold changes nothing"""
    r = 1
    f, m, _ = inputs(r, 0.0, (12, 12, 12))
    _, mask = G.smooth_fixed((12, 12, 12))
    u = mask[0, 0].to(F64)
    assert not bool(u[0].any() or u[-1].any() or u[:, 0].any() or u[:, -1].any() or u[:, :, 0].any() or u[:, :, -1].any())
    ref = N.reference(f, m, u, r)
    for a in (-3, -2, -1):
        for e in (0, 1):
            assert torch.equal(N.gradient(f, m, ref['p'], ref['q'], ref['t'], r, drop=((a, e),)), ref['g'])


def test_flat_window():
    """the definition has no special case: a flat window gives cc = 0, d = 1 and gradient 0"""
    f = torch.full((5, 5, 5), 0.25)
    m = torch.rand(5, 5, 5, generator=torch.Generator().manual_seed(1))
    T = N.terms(f, m, 1.0, 1)
    assert float((T['d'] - 1.0).abs().max()) < 1e-9
    assert float(N.gradient(f, m, T['p'], T['q'], T['t'], 1).abs().max()) < 1e-9


def test_tolerance_refuses_what_first_order_cannot_bound():
    f = torch.full((5, 5, 5), 200.0)
    m = torch.rand(5, 5, 5, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match='too flat'):
        N.tolerance(f, m, 1.0, 1)
