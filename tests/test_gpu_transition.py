"""Full-transition parity of the HIP path (through the C ABI) with the reference fixtures and the CPU oracle."""
import numpy as np
import pytest
import torch

from ir_sgmcmc_amd.engine import EngineConfig, TransitionEngine
from oracle import OracleChain, OracleConfig
from tests._golden import Golden, golden_names
from tests._report import GRAD_RTOL, check, fp64_band

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def engine_config(oc: OracleConfig, seed=0):
    return EngineConfig(dims=oc.dims, no_chains=oc.no_chains, cps=oc.cps if oc.transformation == 'SVFFD_3D' else None,
                        no_steps=oc.no_steps, sobolev_s=oc.sobolev_s or 0, sobolev_lambda=oc.sobolev_lambda, lr=oc.lr,
                        uniform_noise=oc.uniform_noise or 0.0, virtual_decimation=oc.virtual_decimation,
                        data_loss=oc.data_loss, gmm_components=oc.gmm_components, lcc_s=oc.lcc_s, ssd_sigma=oc.ssd_sigma,
                        gmm_lr_log_std=oc.gmm_lr_log_std, gmm_lr_logits=oc.gmm_lr_logits, gmm_lr_decay=oc.gmm_lr_decay,
                        scale_prior=oc.scale_prior, dirichlet_alpha=[oc.dirichlet_alpha], reg_loss=oc.reg_loss,
                        student=O_student(oc), w_reg=oc.w_reg, reg_learnable=oc.reg_learnable, reg_lr=oc.reg_lr, reg_lr_decay=oc.reg_lr_decay,
                        loc_prior_nu=oc.reg_loc_prior_nu, reg_scale_prior=oc.reg_scale_prior, seed=seed)


def O_student(oc):
    from oracle import ops as O
    return O.student_params(*oc.student)


def to_dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def outputs_for(cfg: EngineConfig):
    C, dv, d = cfg.no_chains, cfg.dims_v, cfg.dims
    z = lambda *s: torch.empty(*s, device=DEV, dtype=torch.float32)
    return {'curr_state': z(C, 3, *dv), 'im_moving_warped': z(C, 1, *d), 'residuals': z(C, 1, *d),
            'displacement': z(C, 3, *d), 'transformation': z(C, 3, *d), 'grad_v': z(C, 3, *dv)}


def close(a, b, atol):
    return float((a.double().cpu() - b.double()).abs().max()) <= atol


@pytest.mark.parametrize('name', golden_names())
def test_transition_matches_reference_fixture(name):
    g = Golden(name)
    fixed, moving, v0, sigma = g.inputs()
    cfg = engine_config(g.cfg)
    eng = TransitionEngine(cfg, DEV)
    fixed_d, moving_d = eng.prepare(to_dev(fixed), to_dev(moving))

    # Trainer.__GMM_init on the device vs the reference's parameters after 25 warm-up steps
    eng.gmm_init(fixed_d, moving_d)
    st, gi = eng.state(), g.gmm_init()
    K = cfg.gmm_components
    assert np.allclose(list(st.gmm_log_std)[:K], gi['log_std'].numpy(), atol=2e-4)
    assert np.allclose(list(st.gmm_logits)[:K], gi['logits'].numpy(), atol=2e-4)
    assert st.gmm_adam_step[0] == 25
    # ... then continue from the reference's exact state so that the transition comparison is not polluted
    for k in range(K):
        st.gmm_log_std[k], st.gmm_logits[k] = float(gi['log_std'][k]), float(gi['logits'][k])
        for i in range(2):
            st.gmm_adam_m[i][k], st.gmm_adam_v[i][k] = float(gi['adam'][i][1][k]), float(gi['adam'][i][2][k])
    if 'reg_loc_init' in g.z.files:
        assert abs(st.reg_param[0] - float(g.z['reg_loc_init'])) < 1e-5
        assert abs(st.reg_param[1] - float(g.z['reg_log_scale_init'])) < 1e-5
        st.reg_param[0], st.reg_param[1] = float(g.z['reg_loc_init']), float(g.z['reg_log_scale_init'])
    eng.set_state(st)

    v = v0.to(DEV).contiguous()
    sig = sigma.to(DEV).contiguous()
    out = outputs_for(cfg)
    T = 'fixture/' + name
    for it in range(g.T):
        eps, unif = g.noise(it)
        eng.transition(fixed_d, moving_d, v, sig, eps.to(DEV), unif.to(DEV) if unif is not None else None, out)
        sc, st = eng.scalars(), eng.state()
        ref = lambda k: g.t(it, k)
        check(T, 'alpha', sc['alpha'], ref('alpha'), 2e-5)
        # north-star: loss within 1e-5 relative
        check(T, 'data_term (rel)', torch.tensor(sc['data_term']) / ref('data').abs(), torch.sign(ref('data')), 1e-5)
        check(T, 'reg_term (rel)', torch.tensor(sc['reg_term']) / ref('reg').abs(), torch.sign(ref('reg')), 1e-5)
        check(T, 'reg_energy (rel)', torch.tensor(sc['reg_energy']) / ref('reg_energy').abs(), torch.ones(cfg.no_chains), 1e-5)
        check(T, 'gmm_log_std', list(st.gmm_log_std)[:K], ref('gmm_log_std'), 2e-5)
        check(T, 'gmm_logits', list(st.gmm_logits)[:K], ref('gmm_logits'), 2e-5)
        if g.has(it, 'reg_loc'):
            check(T, 'reg_loc', st.reg_param[0], ref('reg_loc'), 1e-5)
            check(T, 'reg_log_scale', st.reg_param[1], ref('reg_log_scale'), 1e-5)
        elif g.has(it, 'reg_log_w'):
            check(T, 'reg_log_w', st.reg_param[0], ref('reg_log_w'), 1e-5)
        cs = ref('curr_state')
        # (the 64^3 fixture stores sub-sampled outputs -- and the FULL v_new of every transition but the last, on which the chain
        # is re-synchronised below like the dense fixtures: no drift allowance)
        drift = 0.0
        check(T, 'curr_state', g.sub(out['curr_state']), cs, 2e-6 * max(1.0, float(cs.abs().max())) + drift)
        # north-star: displacement field within 1e-4 (voxels)
        check(T, 'displacement [voxels]', g.sub(out['displacement']), ref('displacement'), 1e-4 + drift)
        check(T, 'transformation', g.sub(out['transformation']), ref('transformation'), 1e-5 + drift)
        check(T, 'im_moving_warped', g.sub(out['im_moving_warped']), ref('im_moving_warped'), 1e-5 + drift)
        mask = g.sub(fixed['mask'].float())
        check(T, 'residuals', g.sub(out['residuals']).cpu() * mask, ref('residuals'), 2e-4 + 10 * drift)
        gv = ref('grad_v')
        gmax = float(gv.abs().max())
        check(T, 'grad_v (rel to max)', g.sub(out['grad_v']).cpu() / gmax, gv / gmax, GRAD_RTOL + 10 * drift)
        check(T, 'v_new', g.sub(v), ref('v_new'), cfg.lr * (GRAD_RTOL + 10 * drift) * gmax + 1e-5 + drift)
        # continue from the reference's state so that every transition is compared on equal inputs
        if not g.subsampled:
            v.copy_(ref('v_new').to(DEV))
        elif it + 1 < g.T:
            v.copy_(ref('v_new_full').to(DEV))


@pytest.mark.parametrize('variant', ['ssd_l2', 'ssd_vd_lognormal', 'gmm_nosobolev_c3', 'steps1', 'steps2', 'steps5_c2',
                                     'noncubic_gmm', 'noncubic_ssd_c2', 'tiny_gmm', 'gmm_k2', 'gmm_k6', 'narrow_sobolev', 'narrow_sobolev_svffd'])
def test_transition_matches_oracle_builder_variants(variant):
    """Configurations without a reference counterpart (SSD is builder-defined) or not covered by a fixture; the non-cubic ones
    (D != H != W, none a multiple of a tile edge) put ragged tiles and segments under every kernel of the composition."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    N = 20
    # tiny_gmm: a volume smaller than any tile or marching segment
    # narrow_sobolev*: a velocity grid NARROWER than the 2 s + 1 taps of the Sobolev kernel (replicate padding folds a tap back more
    # than once; irs_create used to refuse these, the reference runs them -- found by tests/test_gpu_fuzz.py)
    dims = {'noncubic_gmm': (18, 26, 34), 'noncubic_ssd_c2': (33, 20, 17), 'tiny_gmm': (8, 9, 10), 'narrow_sobolev': (5, 13, 7),
            'narrow_sobolev_svffd': (12, 14, 9)}.get(variant, (N, N, N))
    kw = dict(ssd_l2=dict(data_loss='SSD', virtual_decimation=False, ssd_sigma=0.05),
              ssd_vd_lognormal=dict(data_loss='SSD', virtual_decimation=True, reg_loss='RegLoss_LogNormal',
                                    reg_learnable=True, no_chains=2),
              gmm_nosobolev_c3=dict(no_chains=3, sobolev_s=None, uniform_noise=None, lcc_s=2, lr=0.02),
              # few squaring steps: the first / last / only step of the chain has its own field layouts in the fused path
              steps1=dict(no_steps=1, lr=0.05), steps2=dict(no_steps=2, lr=0.05), steps5_c2=dict(no_steps=5, no_chains=2, lr=0.05),
              noncubic_gmm=dict(), noncubic_ssd_c2=dict(data_loss='SSD', virtual_decimation=True, no_chains=2),
              tiny_gmm=dict(lr=0.05),
              narrow_sobolev=dict(lr=0.05, sobolev_s=4), narrow_sobolev_svffd=dict(lr=0.05, sobolev_s=4, transformation='SVFFD_3D', cps=(4, 4, 4), data_loss='SSD'),
              # other numbers of mixture components: K <= 4 and K > 4 run different builds of the statistics kernel
              gmm_k2=dict(gmm_components=2), gmm_k6=dict(gmm_components=6, no_chains=2))[variant]
    oc = OracleConfig(dims=dims, **kw)
    C = oc.no_chains
    f1, m1 = synthetic_pair(dims, seed=3)
    fixed = {k: v.unsqueeze(0).expand(C, *v.shape).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).expand(C, *v.shape).contiguous() for k, v in m1.items() if k != 'seg'}
    gen = torch.Generator().manual_seed(11)
    from oracle import ops as O
    amp = 1.5 if variant in ('tiny_gmm', 'narrow_sobolev', 'narrow_sobolev_svffd') else 6.0  # (6 voxels would fold an 8-voxel volume several times over)
    dv = oc.dims_v  # (the control grid of an SVFFD)
    v0 = O.separable_conv3d_replicate(amp * torch.randn(C, 3, *dv, generator=gen), O.sobolev_kernel_1d(2, 0.5)).contiguous()
    orc = OracleChain(oc, v0=v0)
    orc.init_gmm(fixed, moving)

    cfg = engine_config(oc)
    eng = TransitionEngine(cfg, DEV)
    fixed_d, moving_d = eng.prepare(to_dev(fixed), to_dev(moving))
    eng.gmm_init(fixed_d, moving_d)
    st = eng.state()
    if oc.data_loss == 'GMM':
        assert np.allclose(list(st.gmm_log_std)[:oc.gmm_components], orc.log_std.detach().numpy(), atol=2e-4)
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    for it in range(3):
        eps = torch.randn(C, 3, *dv, generator=gen)
        unif = torch.rand(C, 3, *dims, generator=gen) if oc.uniform_noise is not None else None
        o = orc.transition(fixed, moving, eps, unif)
        eng.transition(fixed_d, moving_d, v, None, eps.to(DEV), unif.to(DEV) if unif is not None else None, out)
        sc = eng.scalars()
        T = 'oracle/' + variant
        check(T, 'alpha', sc['alpha'], o['alpha'], 5e-5)
        check(T, 'data_term (rel)', torch.tensor(sc['data_term']) / torch.tensor(o['data']).abs(), torch.sign(torch.tensor(o['data'])), 1e-5)
        check(T, 'reg_term (rel)', torch.tensor(sc['reg_term']) / torch.tensor(o['reg']).abs(), torch.sign(torch.tensor(o['reg'])), 1e-5)
        check(T, 'displacement [voxels]', out['displacement'], o['displacement'], 1e-4)
        gmax = float(o['grad_v'].abs().max())
        check(T, 'grad_v (rel to max)', out['grad_v'].cpu() / gmax, o['grad_v'] / gmax, GRAD_RTOL)
        check(T, 'v_new', v, o['v_new'], oc.lr * GRAD_RTOL * gmax + 1e-5)
        v.copy_(o['v_new'].to(DEV))


@pytest.mark.parametrize('amp', [1.6, 3.5, 9.0])
def test_localised_large_displacement_against_the_oracle(amp):
    """A velocity field whose large displacements sit in ONE region of the volume -- what a converged registration looks like: the
    squaring steps near that region need the radius-2 / any-radius adjoint variants while most of the volume would not (the variant
    is chosen per chain from the global bound; a per-TILE choice was built and measured slower in round 4).
    Against the oracle; the volume is several tiles wide on every axis and ragged, the bump sits off-centre."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    dims = (70, 52, 84)  # D, H, W
    oc = OracleConfig(dims=dims, lr=0.05)
    f1, m1 = synthetic_pair(dims, seed=3)
    fixed = {k: v.unsqueeze(0).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).contiguous() for k, v in m1.items() if k != 'seg'}
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in dims], indexing='ij')
    bump = torch.exp(-(((zz - 40.0) / 11.0) ** 2 + ((yy - 20.0) / 9.0) ** 2 + ((xx - 50.0) / 13.0) ** 2))
    v0 = (amp * torch.stack([bump, -0.8 * bump, 0.6 * bump])).unsqueeze(0).contiguous()
    gen = torch.Generator().manual_seed(5)
    eps = torch.randn(1, 3, *dims, generator=gen)
    unif = torch.rand(1, 3, *dims, generator=gen)
    orc = OracleChain(oc, v0=v0)
    orc.init_gmm(fixed, moving)
    o = orc.transition(fixed, moving, eps, unif)
    cfg = engine_config(oc)
    gmax = float(o['grad_v'].abs().max())
    eng = TransitionEngine(cfg, DEV)
    eng.option('predict_variants', 0)
    fd, md = eng.prepare(to_dev(fixed), to_dev(moving))
    eng.gmm_init(fd, md)
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    eng.transition(fd, md, v, None, eps.to(DEV), unif.to(DEV), out)
    eng.flush()
    T = f'oracle/bump_amp{amp:g}'
    sc = eng.scalars()
    check(T, 'data_term (rel)', torch.tensor(sc['data_term']) / torch.tensor(o['data']).abs(), torch.sign(torch.tensor(o['data'])), 1e-5)
    check(T, 'displacement [voxels]', out['displacement'], o['displacement'], 1e-4)
    # (an analytic bump puts many samples within rounding of a cell face, where the interpolant's derivative jumps and CPU and GPU may
    # take different sides: the bulk is held to the usual tolerance, the stragglers counted -- DESIGN.md "Numerics")
    dev_g = (out['grad_v'].cpu() - o['grad_v']).abs() / gmax
    check(T, 'grad_v (rel to max, 99.9th percentile)', dev_g.flatten().kthvalue(int(0.999 * dev_g.numel())).values, torch.tensor(0.0), GRAD_RTOL)
    check(T, 'grad_v: fraction of voxels beyond tolerance', (dev_g > GRAD_RTOL).float().mean(), torch.tensor(0.0), 1e-3)


@pytest.mark.parametrize('N,loss', [(128, 'gmm'), (128, 'ssd'), (256, 'gmm')])
def test_transition_matches_oracle_at_full_size(N, loss):
    """BASELINE.json configs 2 / 3 at their own size: 128^3, SSD + RegLoss_L2 (config 2; SSD is builder-defined, SURVEY.md
    section 0) and GMM / LCC s = 1 with virtual decimation (config 3), both with Sobolev smoothing and jitter: one transition of
    the HIP path against the CPU oracle on the same injected noise, at the north-star tolerances (loss terms 1e-5 relative,
    displacement 1e-4 voxels).  The oracle needs ~10 s of host time at this size.  (256, 'gmm') is the workload bench.py times,
    compared directly as well (about a minute of host time for the oracle's mixture warm-up and its one transition)."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    oc = OracleConfig(dims=(N, N, N)) if loss == 'gmm' else OracleConfig(dims=(N, N, N), data_loss='SSD', virtual_decimation=False,
                                                                         reg_loss='RegLoss_L2', w_reg=1.4)
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = {k: v.unsqueeze(0).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).contiguous() for k, v in m1.items() if k != 'seg'}
    gen = torch.Generator().manual_seed(21)
    from oracle import ops as O
    # a smooth 3-voxel velocity field (low-resolution noise, upsampled): a rough field that folds the grid amplifies the
    # rounding differences of the twelve compositions beyond any fixed tolerance (see test_svf_exp_forward, amp = 25)
    lo = torch.randn(1, 3, N // 8, N // 8, N // 8, generator=gen)
    v0 = torch.nn.functional.interpolate(lo, size=(N, N, N), mode='trilinear', align_corners=True)
    v0 = (v0 * (3.0 / float(v0.abs().max()))).contiguous()
    orc = OracleChain(oc, v0=v0)
    orc.init_gmm(fixed, moving)
    cfg = engine_config(oc)
    eng = TransitionEngine(cfg, DEV)
    fixed_d, moving_d = eng.prepare(to_dev(fixed), to_dev(moving))
    eng.gmm_init(fixed_d, moving_d)
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    eps = torch.randn(1, 3, N, N, N, generator=gen)
    unif = torch.rand(1, 3, N, N, N, generator=gen) if oc.uniform_noise is not None else None
    o = orc.transition(fixed, moving, eps, unif)
    eng.transition(fixed_d, moving_d, v, None, eps.to(DEV), unif.to(DEV) if unif is not None else None, out)
    sc = eng.scalars()
    T = f'oracle/{N}^3_' + loss
    assert float(o['displacement'].abs().max()) > 1.0   # not a trivial field
    check(T, 'alpha', sc['alpha'], o['alpha'], 5e-5)
    check(T, 'data_term (rel)', torch.tensor(sc['data_term']) / torch.tensor(o['data']).abs(), torch.sign(torch.tensor(o['data'])), 1e-5)
    check(T, 'reg_term (rel)', torch.tensor(sc['reg_term']) / torch.tensor(o['reg']).abs(), torch.sign(torch.tensor(o['reg'])), 1e-5)
    # Displacement: the north star's 1e-4 voxels -- except where the REFERENCE ARITHMETIC ITSELF is not that accurate.  fp32
    # positions live in [-1, 1] (one ulp = 7.6e-6 voxels at 256^3) and twelve compositions accumulate a few of them: the fp32
    # oracle deviates 2.9e-5 voxels (128^3) / 1.17e-4 voxels (256^3) from its own fp64 evaluation on exactly these inputs
    # (tests/golden/fp64_bands.json, written by tests/golden/make_golden_fp64.py).  The HIP path may be no further from the fp32
    # oracle than the fp32 oracle is from fp64; the relative form (1e-4 of the field's maximum) holds at every size.
    band = fp64_band(f'oracle_{N}_gmm_full_size_test_inputs')
    dmax_o = float(o['displacement'].abs().max())
    check(T, 'displacement [voxels]', out['displacement'], o['displacement'], max(1e-4, band['displacement_max_abs_dev_voxels']))
    check(T, 'displacement (rel to max)', out['displacement'].cpu() / dmax_o, o['displacement'] / dmax_o, 1e-4)
    # Gradient: trilinear interpolation's derivative jumps across cell faces, and among millions of voxels x 12 steps a few
    # dozen sampling positions sit within fp32 rounding of a face, where two correct evaluations take different one-sided
    # derivatives.  The yardstick is again the oracle's own fp32-vs-fp64 band on these inputs: the fraction of voxels whose
    # gradient moves by more than 1e-3 of the maximum (2.8e-5 at 128^3, 5.0e-5 at 256^3) bounds the fraction on which the HIP
    # path may differ from the fp32 oracle by that much, and the 99.99th percentile of the deviation stays below 1e-3.
    gmax = float(o['grad_v'].abs().max())
    dev = (out['grad_v'].cpu() - o['grad_v']).abs() / gmax
    frac_bad = float((dev > GRAD_RTOL).double().mean())
    check(T, 'grad_v: fraction of voxels beyond tolerance', torch.tensor(frac_bad), torch.tensor(0.0), band['grad_frac_beyond_1e-3'])
    check(T, 'grad_v (rel to max), 99.99th percentile', torch.tensor(float(dev.flatten().kthvalue(int(0.9999 * dev.numel())).values)), torch.tensor(0.0), GRAD_RTOL)


@pytest.mark.parametrize('case', ['lcc_s2_128', 'svffd_cps4_64'])
def test_larger_sizes_of_the_less_common_configurations(case):
    """The LCC window s = 2 (configs/experiment3-4 of the reference) and SVFFD_3D with control-point spacing 4 (experiment5) are
    pinned by reference fixtures at 16^3 only; here one transition each at a realistic size against the oracle on the same
    injected noise: 128^3 with s = 2 (125-tap box filters: other tile / halo arithmetic than s = 1), 64^3 SVFFD cps 4 (a 19^3
    control grid: B-spline up-sampling and its adjoint around the dense squaring steps)."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    if case == 'lcc_s2_128':
        N = 128
        oc = OracleConfig(dims=(N, N, N), lcc_s=2)
    else:
        N = 64
        oc = OracleConfig(dims=(N, N, N), transformation='SVFFD_3D', cps=(4, 4, 4), lr=0.01)
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = {k: v.unsqueeze(0).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).contiguous() for k, v in m1.items() if k != 'seg'}
    gen = torch.Generator().manual_seed(33)
    dv = oc.dims_v
    lo = torch.randn(1, 3, max(dv[0] // 8, 2), max(dv[1] // 8, 2), max(dv[2] // 8, 2), generator=gen)
    v0 = torch.nn.functional.interpolate(lo, size=dv, mode='trilinear', align_corners=True)
    v0 = (v0 * (2.5 / float(v0.abs().max()))).contiguous()
    orc = OracleChain(oc, v0=v0)
    orc.init_gmm(fixed, moving)
    cfg = engine_config(oc)
    eng = TransitionEngine(cfg, DEV)
    fixed_d, moving_d = eng.prepare(to_dev(fixed), to_dev(moving))
    eng.gmm_init(fixed_d, moving_d)
    v = v0.to(DEV).contiguous()
    out = outputs_for(cfg)
    eps = torch.randn(1, 3, *dv, generator=gen)
    unif = torch.rand(1, 3, N, N, N, generator=gen)
    o = orc.transition(fixed, moving, eps, unif)
    eng.transition(fixed_d, moving_d, v, None, eps.to(DEV), unif.to(DEV), out)
    sc = eng.scalars()
    T = 'oracle/' + case
    assert float(o['displacement'].abs().max()) > 0.5
    check(T, 'alpha', sc['alpha'], o['alpha'], 5e-5)
    check(T, 'data_term (rel)', torch.tensor(sc['data_term']) / torch.tensor(o['data']).abs(), torch.sign(torch.tensor(o['data'])), 1e-5)
    check(T, 'reg_term (rel)', torch.tensor(sc['reg_term']) / torch.tensor(o['reg']).abs(), torch.sign(torch.tensor(o['reg'])), 1e-5)
    check(T, 'displacement [voxels]', out['displacement'], o['displacement'], 1e-4)
    # (the LCC residual divides by the local standard deviation of the warped image: in a nearly flat window the 1e-6 agreement of
    # the warped images is amplified by 1 / sigma_M -- a handful of such voxels among two million; the sums above are unaffected)
    zr = torch.where(fixed['mask'], o['residuals'], torch.zeros(()))
    dz = (out['residuals'].cpu() * fixed['mask'].float() - zr).abs().flatten()
    check(T, 'residuals, 99.99th percentile', torch.tensor(float(dz.kthvalue(max(1, int(0.9999 * dz.numel()))).values)), torch.tensor(0.0), 2e-4)
    check(T, 'residuals, max', torch.tensor(float(dz.max())), torch.tensor(0.0), 1e-3)
    gmax = float(o['grad_v'].abs().max())
    dev = (out['grad_v'].cpu() - o['grad_v']).abs() / gmax
    check(T, 'grad_v: fraction of voxels beyond tolerance', torch.tensor(float((dev > GRAD_RTOL).double().mean())), torch.tensor(0.0), 1e-4)
    check(T, 'v_new (99.99th percentile)', torch.tensor(float((v.cpu() - o['v_new']).abs().flatten().kthvalue(max(1, int(0.9999 * v.numel()))).values)),
          torch.tensor(0.0), oc.lr * GRAD_RTOL * gmax + 1e-5)


def test_sigma_field_runs_the_fused_stage_a():
    """A chain started from the VI posterior (MCMC_init 'VI', utils/functions.py:78-84: 14 of the reference's 16 configs) carries a
    sigma FIELD as the preconditioner of its Langevin noise.  With in-kernel noise that path now takes the one-kernel stage A too
    (its 32 x 16 tile); the chain is bit-identical to the two-kernel form."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    N = 40
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    g = torch.Generator().manual_seed(11)
    sigma = (0.25 + torch.rand(2, 3, N, N, N, generator=g)).to(DEV)
    res = []
    for fuse in (1, 0):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), no_chains=2, seed=3), DEV)
        eng.option('fuse_noise', fuse)
        fd, md = eng.prepare({k: v.expand(2, *v.shape[1:]).contiguous() for k, v in fixed.items()},
                             {k: v.expand(2, *v.shape[1:]).contiguous() for k, v in moving.items()})
        eng.gmm_init(fd, md)
        v = torch.zeros(2, 3, N, N, N, device=DEV)
        for _ in range(3):
            eng.transition(fd, md, v, sigma)
        eng.flush()
        assert bool(torch.isfinite(v).all())
        res.append(v.clone())
    assert torch.equal(res[0], res[1])


def test_in_kernel_noise_path_runs_and_is_reproducible():
    """eps / unif = NULL -> Philox noise keyed by (seed, iteration): same seed -> same chain, other seed -> other chain."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    N = 24
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    res = []
    for i, seed in enumerate((5, 5, 6)):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), seed=seed), DEV)
        if i == 1:
            eng.option('fuse_noise', 0)   # the two-kernel form of perturbation + smoothing draws the same noise: the same chain
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = torch.zeros(1, 3, N, N, N, device=DEV)
        for _ in range(4):
            eng.transition(fd, md, v)
        assert eng.state().iteration == 4
        assert bool(torch.isfinite(v).all())
        res.append(v.clone())
    assert torch.equal(res[0], res[1])   # no float atomics anywhere on the path, fixed summation order: bit-reproducible
    assert float((res[0] - res[2]).abs().max()) > 1e-2 * float(res[0].abs().max())


@pytest.mark.parametrize('amp', [0.3, 1.6, 3.5, 7.0])
def test_variant_prediction_never_changes_the_result(amp):
    """Which squaring-step variants get launched is decided on the host from the (unsynchronised) displacement bounds of an
    earlier transition.  Whatever the decision -- every variant (mode 0), the production heuristic (1), or always 'small'
    (2: forward steps on the radius-1 kernel alone with far taps from global memory; adjoint steps without the any-radius
    kernel, the radius-2 kernel falling back to its generic gather above two voxels) -- the transition is the same."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    N = 24
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    g = torch.Generator().manual_seed(3)
    v0 = perturb_smooth(torch.randn(1, 3, N, N, N, generator=g).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (amp / float(v0.abs().max()))
    eps = torch.randn(1, 3, N, N, N, generator=g).to(DEV)
    res = {}
    for mode in (0, 1, 2):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), seed=1), DEV)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        out = outputs_for(eng.cfg)
        for _ in range(3):   # the heuristic only has bounds to look at from the second transition on
            eng.transition(fd, md, v, eps=eps, outputs=out)
        torch.cuda.synchronize()
        res[mode] = (v.clone(), out['grad_v'].clone(), out['displacement'].clone())
    # Every variant is deterministic and the device selects per step from the same bounds whatever was launched, so the modes run
    # IDENTICAL kernels on every step (a variant that was launched and not selected exits at once): bit-equal, not "close"
    # (tools/debug/variant_bits.py prints the comparison per mode and amplitude).
    for mode in (1, 2):
        for i, what in enumerate(('v', 'grad_v', 'displacement')):
            assert torch.equal(res[mode][i], res[0][i]), (mode, what, float((res[mode][i] - res[0][i]).abs().max()))


@pytest.mark.parametrize('N,C,kw', [(28, 3, {}), (40, 2, {'lcc_s': 2}), (33, 4, {'virtual_decimation': False}), (30, 3, {'per_chain_images': True})])
def test_one_data_term_launch_for_all_chains_is_the_serial_chain(N, C, kw):
    """Several chains in one engine (every reference config runs two; trainer.py:316-330 steps the shared mixture chain after chain
    and evaluates each chain's data term with the mixture ITS step left).  By default the serial loop is statistics -> step only,
    every step leaves a snapshot of the mixture constants, and the data terms of all chains run as ONE launch behind the loop, each
    chain against its snapshot (csrc/api_ctx.hip, `data_batch`).  Same arithmetic on the same values, same partial-sum slots: bit for
    bit the chain of the serial form (`data_batch` 0) -- velocity, mixture and optimiser state, loss terms."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    kw = dict(kw)
    f1, m1 = synthetic_pair((N, N, N), seed=3)
    if kw.pop('per_chain_images', False):
        # every chain its own fixed image and mask (the interface takes one per chain): the single launch strides through them
        fixed = {k: torch.stack([v] * C) for k, v in f1.items() if k != 'seg'}
        moving = {k: torch.stack([v] * C) for k, v in m1.items() if k != 'seg'}
        for c in range(1, C):
            fixed['mask'][c, ..., : 3 * c, :] = 0                         # chain c ignores a band of rows
            fixed['im'][c] = fixed['im'][c].roll(c, dims=-1)              # ... and sees a shifted image
        fixed, moving = to_dev(fixed), to_dev(moving)
    else:
        fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
        moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    g = torch.Generator().manual_seed(12)
    v0 = (2.0 * torch.randn(C, 3, N, N, N, generator=g)).to(DEV)
    res = {}
    for mode in (1, 0):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), no_chains=C, data_loss='GMM', seed=6, **kw), DEV)
        eng.option('data_batch', mode)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        sc = []
        for _ in range(4):
            eng.transition(fd, md, v)
            sc.append(eng.scalars())
        eng.flush()
        torch.cuda.synchronize()
        st = eng.state()
        res[mode] = (v.clone(), (list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v], list(st.reg_param)),
                     [(list(s['alpha']), list(s['data_term']), list(s['reg_term'])) for s in sc])
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert all(len(set(x[1])) == C for x in res[1][2])    # (and the chains are C different chains)


@pytest.mark.parametrize('data_loss', ['GMM', 'SSD'])
def test_chain_overlap_never_changes_the_result(data_loss):
    """Several chains in one engine (every reference config runs two): the data term of chain c runs on a side stream while the
    statistics of chain c + 1 run on the caller's; the mixture step in between waits for both (csrc/api_ctx.hip, `chain_overlap`; measured
    slower than the serial form in round 5 and off by default -- the knob stays, and so does what it must never do).  Same
    kernels, same inputs, same order of every sum: the chain with the overlap is the chain without it, bit for bit -- velocity,
    mixture and optimiser state, loss terms."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    N, C = 28, 3
    f1, m1 = synthetic_pair((N, N, N), seed=2)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    g = torch.Generator().manual_seed(11)
    v0 = (2.0 * torch.randn(C, 3, N, N, N, generator=g)).to(DEV)
    res = {}
    from ir_sgmcmc_amd import _lib as L
    for mode in (0, 1):
        L.check(L.load().irs_option_set(None, b'chain_overlap', mode))   # (read when a context is created: the side stream exists or not)
        try:
            eng = TransitionEngine(EngineConfig(dims=(N, N, N), no_chains=C, data_loss=data_loss, seed=5), DEV)
        finally:
            L.check(L.load().irs_option_set(None, b'chain_overlap', 0))
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        sc = []
        for _ in range(4):
            eng.transition(fd, md, v)
            sc.append(eng.scalars())
        eng.flush()
        torch.cuda.synchronize()
        st = eng.state()
        res[mode] = (v.clone(), (list(st.gmm_log_std), list(st.gmm_logits), [list(r) for r in st.gmm_adam_m], [list(r) for r in st.gmm_adam_v], list(st.reg_param)),
                     [(list(s['alpha']), list(s['data_term']), list(s['reg_term'])) for s in sc])
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]


def test_transition_under_stream_capture_replays_the_plain_chain():
    """A transition captured into a HIP graph (torch.cuda.CUDAGraph on the current stream: the library launches on the stream it is
    handed) carries no host prediction -- every variant is launched, nothing is re-run -- and its replays are the plain chain, bit for
    bit (in-kernel Philox noise: the counter lives on the device and advances per replay).  What a capture cannot carry is refused,
    loudly: per-stage timings (their events are read back right after the call) and irs_set_state (it waits for the stream)."""
    from ir_sgmcmc_amd import _lib as L
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    N = 24
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})

    def fresh():
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), seed=7), DEV)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        return eng, fd, md

    eng, fd, md = fresh()
    v_plain = torch.zeros(1, 3, N, N, N, device=DEV)
    for _ in range(4):
        eng.transition(fd, md, v_plain)
    eng.flush()
    st_plain = eng.state()

    eng, fd, md = fresh()
    v = torch.zeros(1, 3, N, N, N, device=DEV)
    eng.transition(fd, md, v)                     # (one plain transition first: lazily created resources exist before the capture)
    eng.flush()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.transition(fd, md, v)
        with pytest.raises(L.IrsError, match='captured'):
            eng.transition(fd, md, v, timed=True)
        with pytest.raises(L.IrsError, match='captured'):
            eng.set_state(st_plain)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    eng.flush()
    assert torch.equal(v, v_plain)
    st = eng.state()
    assert int(st.iteration) == int(st_plain.iteration) == 4
    assert list(st.gmm_log_std) == list(st_plain.gmm_log_std) and list(st.gmm_logits) == list(st_plain.gmm_logits)


def test_misprediction_is_recovered_not_fatal():
    """A transition launched WITHOUT a kernel variant its displacement then needs (forced: predict_variants = 3 always predicts
    'tiny', so the radius-2 adjoint is never launched, while the field carries several voxels) must not end the chain: the
    device finds the assumption violated, the transition is a no-op (velocity, mixture, Adam moments, Philox counter untouched),
    and a later call re-runs it with every variant.  The chain equals the one that launched every variant all along -- bit for
    bit with in-kernel Philox noise (the failed transition did not consume its counter)."""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from ir_sgmcmc_amd.ops import perturb_smooth, sobolev_kernel_1d
    N, T = 24, 6
    f1, m1 = synthetic_pair((N, N, N), seed=0)
    fixed = to_dev({k: v.unsqueeze(0) for k, v in f1.items() if k != 'seg'})
    moving = to_dev({k: v.unsqueeze(0) for k, v in m1.items() if k != 'seg'})
    g = torch.Generator().manual_seed(3)
    v0 = perturb_smooth(torch.randn(1, 3, N, N, N, generator=g).to(DEV), sobolev_kernel_1d(3, 0.5))
    v0 = v0 * (9.0 / float(v0.abs().max()))   # d_10, d_11 beyond one voxel: the radius-1 adjoint alone is wrong for them
    res = {}
    for mode in (0, 3):
        eng = TransitionEngine(EngineConfig(dims=(N, N, N), seed=11), DEV)
        eng.option('predict_variants', mode)
        fd, md = eng.prepare(fixed, moving)
        eng.gmm_init(fd, md)
        v = v0.clone()
        for _ in range(T):
            eng.transition(fd, md, v)
        eng.flush()                          # the last two transitions are only checked here
        st = eng.state()
        assert st.iteration == T             # every transition happened exactly once
        res[mode] = (v.clone(), list(st.gmm_log_std), list(st.gmm_logits), eng.recovered_transitions)
    assert res[0][3] == 0 and res[3][3] >= 1, (res[0][3], res[3][3])
    assert torch.equal(res[0][0], res[3][0])
    assert res[0][1] == res[3][1] and res[0][2] == res[3][2]
