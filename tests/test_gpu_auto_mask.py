"""`trainer.auto_mask` on the GPU: 32^3, a handful of transitions.  With the option absent a run is the run it always was; with it
the engine, the metrics and the files see the computed masks; a resumed run ends where the uninterrupted one ends; a
Biobank-layout directory with images only runs with `optional` + `auto_mask`."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import masks as M
from ir_sgmcmc_amd.parse_config import ConfigParser
from ir_sgmcmc_amd.trainer import Trainer
from ir_sgmcmc_amd.utils.imageio import read_nifti, write_nifti
from tests import _masks as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 32
RUN = dict(no_iters_burn_in=2, no_samples_MCMC=4, log_period_MCMC=2)
IMAGE = {'source': 'image', 'closing': 2, 'dilation': 1}


def make_trainer(tmp_path, data_loader=None, **trainer_over):
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    if data_loader is not None:
        cfg['data_loader'] = data_loader
    cfg['trainer'].update(RUN)
    cfg['trainer'].update(trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, config.init_metrics(), device=DEV), dl


def run(t):
    """the chains start from a draw of torch's global generator (sample_q_v): the same draw for every run that is compared"""
    torch.manual_seed(0)
    t.run()


def files(t):
    root = t.config.save_dirs['samples'].parent
    return sorted(str(p.relative_to(root)) for p in root.rglob('*') if p.is_file() and 'log' not in p.parts and p.suffix != '.log')


def digest(t):
    """what tests/test_gpu_trainer.py compares of two runs: the last velocity, the posterior moments, the engine's state"""
    s = t.engine.state()
    return (t.v_curr_state.cpu(), t.displacement_mean.cpu(), t.displacement_std.cpu(), s.iteration, list(s.gmm_log_std), list(s.reg_param))


def same(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(digest(a), digest(b)))


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    t, dl = make_trainer(tmp_path_factory.mktemp('plain'))
    run(t)
    return t, dl


@pytest.fixture(scope='module')
def from_image(tmp_path_factory):
    t, dl = make_trainer(tmp_path_factory.mktemp('image'), auto_mask=IMAGE)
    run(t)
    return t, dl


def test_absent_option_changes_nothing(plain, tmp_path):
    t, dl = plain
    assert t.auto_mask_options is None and t.auto_mask_summary is None
    assert not any('auto_mask' in f for f in files(t)) and not any(k.startswith('auto_mask') for k in t.metrics.result())
    fixed, _, _ = next(iter(dl))
    assert torch.equal(t._fixed['mask'].bool().cpu().reshape(fixed['mask'].shape), fixed['mask'])
    # the hook itself leaves the chain alone: a margin of nothing around the file masks is the same run, plus its own files
    idle, _ = make_trainer(tmp_path, auto_mask={'source': 'file', 'fill_holes': False, 'closing': 0, 'dilation': 0})
    run(idle)
    assert same(t, idle)
    assert [f for f in files(idle) if 'auto_mask' not in f] == files(t)
    assert idle.metrics.result()['auto_mask/fixed/dice_vs_file'] == 1.0


def test_masks_from_the_image(plain, from_image):
    t, dl = from_image
    fixed, moving, _ = next(iter(dl))
    res = t.metrics.result()
    for side, triple in (('fixed', fixed), ('moving', moving)):
        s = t.auto_mask_summary[side]
        im = triple['im'][0, 0].numpy()
        ref, voxels = S.foreground_mask(im, s['threshold'], 26, 1, True, 2, 1)
        value_range = (float(im.min()), float(im.max()))
        assert s['threshold'] == S.otsu_threshold(S.intensity_histogram(im, 256, value_range), value_range)
        assert s['voxels'] == voxels and s['voxels_final'] == int(ref.sum())
        for key in ('threshold', 'voxels', 'fraction', 'components', 'dice_vs_file'):
            assert f'auto_mask/{side}/{key}' in res, key
        assert res[f'auto_mask/{side}/voxels'] == ref.sum() and res[f'auto_mask/{side}/fraction'] == ref.sum() / N ** 3
        file_mask = triple['mask'][0, 0].numpy()
        dice = 2.0 * (ref & file_mask).sum() / (ref.sum() + file_mask.sum())
        assert res[f'auto_mask/{side}/dice_vs_file'] == pytest.approx(dice, abs=1e-12) and dice > 0
        print(f'dice_vs_file {side}: {dice:.4f}, voxels {int(ref.sum())} against {int(file_mask.sum())} of the file mask')
        saved, _ = read_nifti(str(t.config.save_dirs['samples'] / f'auto_mask_{side}.nii.gz'), np.uint8)
        assert np.array_equal(saved.astype(bool), ref)
        if side == 'fixed':  # the engine's mask is the computed one
            assert np.array_equal(t._fixed['mask'].bool().cpu().numpy().reshape(ref.shape), ref)
    assert not same(t, plain[0])  # another mask, another chain


def test_margin_around_the_file_masks(tmp_path):
    t, dl = make_trainer(tmp_path, auto_mask={'source': 'file', 'which': 'fixed', 'fill_holes': False, 'closing': 0, 'dilation': 2})
    run(t)
    fixed, _, _ = next(iter(dl))
    file_mask = fixed['mask'][0, 0].numpy()
    got = t._fixed['mask'].bool().cpu().numpy().reshape(file_mask.shape)
    assert np.array_equal(got, S.dilate(file_mask, 2)) and got[file_mask].all() and got.sum() > file_mask.sum()
    assert sorted(t.auto_mask_summary) == ['fixed'] and t.auto_mask_summary['fixed']['voxels'] == {'file': int(file_mask.sum()),
                                                                                                  'dilation': int(got.sum())}
    assert t.metrics.result()['auto_mask/fixed/voxels'] == got.sum()
    assert not (t.config.save_dirs['samples'] / 'auto_mask_moving.nii.gz').exists()


def test_resumed_run_ends_bit_identical(tmp_path):
    kw = dict(no_iters_burn_in=2, no_samples_MCMC=6, log_period_MCMC=2, checkpoint_period=4, auto_mask=IMAGE)
    a, _ = make_trainer(tmp_path / 'a', **kw)
    run(a)
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000004.pt'
    assert ck.is_file()
    b, _ = make_trainer(tmp_path / 'b', resume=str(ck), **kw)
    run(b)
    assert same(a, b) and torch.equal(a._fixed['mask'], b._fixed['mask'])
    assert a.auto_mask_summary['fixed']['voxels'] == b.auto_mask_summary['fixed']['voxels']


def image_only_dir(root):
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    root.mkdir()
    fixed, moving = synthetic_pair((N, N, N), seed=0)
    for name, triple in (('a_fixed', fixed), ('b_moving', moving)):
        # the reader hands the array over in (x, y, z) order as the file has it; the content only has to be a blob
        write_nifti(triple['im'][0].numpy(), str(root / f'{name}.nii.gz'))
    return str(root)


def test_images_only_run_with_optional_and_auto_mask(tmp_path):
    d = image_only_dir(tmp_path / 'data')
    loader = lambda **extra: {'type': 'BiobankDataLoader', 'args': {'data_dir': d, 'dims': [N, N, N], 'sigma_v_init': 0.5,
                                                                    'u_v_init': 0.1, **extra}}
    with pytest.raises(FileNotFoundError, match='need at least two image / mask / seg triples'):
        make_trainer(tmp_path / 'strict', data_loader=loader(), auto_mask=IMAGE)
    t, dl = make_trainer(tmp_path / 'run', data_loader=loader(optional=['masks', 'segs']), auto_mask=IMAGE)
    assert (dl.has_masks, dl.has_segs) == (False, False)
    run(t)
    res = t.metrics.result()
    assert 'auto_mask/fixed/voxels' in res and 'auto_mask/fixed/dice_vs_file' not in res
    assert 0 < res['auto_mask/fixed/fraction'] < 0.5 and bool(torch.isfinite(t.displacement_mean).all())
    assert int(t._fixed['mask'].sum()) == res['auto_mask/fixed/voxels']
    # without the option the all-true masks are what the engine gets
    u, _ = make_trainer(tmp_path / 'all_true', data_loader=loader(optional=['masks', 'segs']))
    run(u)
    assert int(u._fixed['mask'].sum()) == N ** 3


def test_refusals_at_construction(tmp_path):
    d = image_only_dir(tmp_path / 'data')
    loader = {'type': 'BiobankDataLoader', 'args': {'data_dir': d, 'dims': [N, N, N], 'sigma_v_init': 0.5, 'u_v_init': 0.1,
                                                    'optional': ['masks', 'segs']}}
    with pytest.raises(ValueError, match='cannot be combined with trainer.native_resolution'):
        make_trainer(tmp_path / 'native', data_loader=loader, auto_mask=IMAGE, native_resolution=True)
    with pytest.raises(ValueError, match='"source": "file" needs mask files'):
        make_trainer(tmp_path / 'file', data_loader=loader, auto_mask={'source': 'file'})
    for option in ('label_posterior', 'surface_posterior'):
        with pytest.raises(ValueError, match=f'trainer.{option} needs the fixed and the moving segmentation'):
            make_trainer(tmp_path / option, data_loader=loader, auto_mask=IMAGE, **{option: True})
    with pytest.raises(ValueError, match=r'trainer\.auto_mask\.connectivity'):
        make_trainer(tmp_path / 'bad', auto_mask={'connectivity': 4})
    assert M.auto_mask_options({'auto_mask': IMAGE})['keep'] == 1
