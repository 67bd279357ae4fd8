"""What ir_sgmcmc_amd/ops.py does between torch tensors and the C ABI, pinned without a library and without a GPU.

A recording stand-in replaces the loaded library, `_lib.dev_ptr` loses its `is_cuda` test and hands out tokens, and every case
of CASES runs one public function of ops.py on small CPU tensors.  A case records the C functions called, in order, with every
argument (ints and floats by value, ctypes arrays by their contents, pointer tokens by the input argument they came from -- or
'allocated' --, shape and dtype), then the container type, shapes and dtypes of what the function returns, or the type and the
full message of what it raises.  The stand-in also holds every call to `_lib.SIGNATURES`: the number of arguments and, through
each ctypes type's own from_param, what kind of value stands where.

The expectations are data: tests/golden/ops_calls.json, recorded from the ops.py of the commit before its helpers were folded
(ffd_up/plain, ffd_adjoint/plain and ffd_adjoint/strided again since: their scratch is sized by irs_ffd_scratch_floats).
`IRS_RECORD_OPS_CALLS=1 python -m pytest tests/test_ops_calls_host.py` writes the file anew; a change of ops.py that is meant
to leave its behaviour alone does not need to.
"""
import ctypes as C
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.native import NativeGrid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ops_calls.json')
RECORD = os.environ.get('IRS_RECORD_OPS_CALLS') == '1'
WS_BYTES = 4096  # what every irs_*_workspace of the stand-in answers

# C = 2 chains and three different extents: a transposed dimension shows in a recorded shape
Cn, D, H, W = 2, 4, 5, 6
VOL = (D, H, W)
f32, f64, i16, i32, u8, u16, b8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.uint8, torch.uint16, torch.bool


def t(dtype, *shape):
    """a tensor of the shape with small repeating values (-1 .. 2 in halves for floats, 0 .. 6 for integers)"""
    x = (torch.arange(math.prod(shape)) % 7).reshape(shape)
    if dtype == b8:
        return x % 2 == 0
    return (x * 0.5 - 1.0).to(dtype) if dtype.is_floating_point else x.to(dtype)


# ------------------------------------------------------------------------------------------------ the stand-ins
class Token:
    """what the stand-in dev_ptr returns: the tensor itself, kept alive so that no later allocation takes its address"""

    def __init__(self, tensor):
        self.tensor = tensor


class Recorder:
    def __init__(self, inputs):
        self.calls = []
        self.names = {}     # address of an input's storage -> the argument it came in as
        self.tokens = {}    # address of a tensor that crossed as a pointer -> that tensor
        for name, v in inputs.items():
            for key, x in (v.items() if isinstance(v, dict) else enumerate(v) if isinstance(v, list) else [(None, v)]):
                if isinstance(x, torch.Tensor) and x.numel():
                    self.names[x.untyped_storage().data_ptr()] = name if key is None else f'{name}[{key!r}]'

    # -- _lib.load / dev_ptr / stream_ptr
    def load(self, path=None):
        return self

    @staticmethod
    def dev_ptr(tensor, dtype=None, allow_none=False):
        """_lib.dev_ptr without its is_cuda test"""
        if tensor is None:
            if allow_none:
                return None
            raise L.IrsError('required tensor is None')
        if dtype is not None and tensor.dtype != dtype:
            raise L.IrsError(f'expected {dtype}, got {tensor.dtype}')
        if not tensor.is_contiguous():
            raise L.IrsError('tensor must be contiguous')
        return Token(tensor)

    @staticmethod
    def stream_ptr():
        return 'stream'

    # -- the library
    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)

        def fn(*args):
            argtypes = L.SIGNATURES[name]
            assert len(args) == len(argtypes), f'{name}: {len(args)} arguments for {len(argtypes)} parameters'
            for i, (a, ty) in enumerate(zip(args, argtypes)):
                if isinstance(a, Token) or a == 'stream':
                    assert ty is C.c_void_p, f'{name}: argument {i} is a device pointer, the header has {ty.__name__}'
                else:
                    ty.from_param(a)  # TypeError / ArgumentError where ctypes would refuse the value
            self.calls.append({'fn': name, 'args': [self.argument(name, i, args) for i in range(len(args))]})
            if name.endswith('_workspace'):
                args[-1]._obj.value = WS_BYTES
            if name == 'irs_ffd_scratch_floats':  # a size by value: the scratch the next call takes shows it
                return WS_BYTES // 4
            if name == 'irs_label_boxes':  # the boxes a later call reads back through its host pointer
                args[5].tensor.copy_(torch.arange(args[5].tensor.numel()).reshape(args[5].tensor.shape))
            return 0
        return fn

    def tensor(self, x):
        name = self.names.get(x.untyped_storage().data_ptr(), 'allocated') if x.numel() else 'allocated'
        return {'ptr': name, 'shape': list(x.shape), 'dtype': str(x.dtype)}

    def argument(self, fn, i, args):
        a = args[i]
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, Token):
            self.tokens[a.tensor.data_ptr()] = a.tensor
            return self.tensor(a.tensor)
        if isinstance(a, C.Array):
            return {'array': a._type_.__name__, 'values': list(a)}
        if isinstance(a, C._Pointer):  # into the host copy of a tensor an earlier call wrote: what it is and what it holds
            x = self.tokens[C.cast(a, C.c_void_p).value]
            return {'host': self.tensor(x), 'pointer': a._type_.__name__, 'values': [a[j] for j in range(x.numel())]}
        if isinstance(a, C.c_void_p) and fn == 'irs_perturb_smooth' and i == 4:  # the 2 s + 1 taps, s the next argument
            return {'array': 'c_float', 'values': list(C.cast(a, C.POINTER(C.c_float * (2 * args[5] + 1))).contents)}
        if type(a).__name__ == 'CArgObject':
            return {'byref': type(a._obj).__name__}
        raise AssertionError(f'{fn}: argument {i} is a {type(a).__name__}')


def describe(v):
    """container types, shapes and dtypes of a return value; plain numbers by value"""
    if isinstance(v, torch.Tensor):
        return {'tensor': list(v.shape), 'dtype': str(v.dtype)}
    if isinstance(v, np.ndarray):
        return {'ndarray': list(v.shape), 'dtype': str(v.dtype)}
    if isinstance(v, dict):
        return {'dict': {k: describe(x) for k, x in v.items()}}
    if isinstance(v, (tuple, list)):
        return {type(v).__name__: [describe(x) for x in v]}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def run(monkeypatch, fn, kwargs):
    rec = Recorder(kwargs)
    monkeypatch.setattr(L, 'load', rec.load)
    monkeypatch.setattr(L, 'dev_ptr', rec.dev_ptr)
    monkeypatch.setattr(L, 'stream_ptr', rec.stream_ptr)
    kwargs = dict(kwargs)
    star = kwargs.pop('*', [])
    out = {}
    try:
        out['returns'] = describe(getattr(ops, fn)(*star, **kwargs))
    except (L.IrsError, NotImplementedError) as e:
        out['raises'] = {'type': type(e).__name__, 'message': str(e)}
    out['calls'] = rec.calls
    return out


# ------------------------------------------------------------------------------------------------ the table
def field(*lead):
    return t(f32, *(lead or (Cn,)), 3, D, H, W)


def vol(dtype=f32, chains=Cn):
    return t(dtype, chains, 1, D, H, W)


CPS = (1, 2, 5)  # a (6,5,4) control grid
GRID = NativeGrid.from_shape((3, 5, 4), VOL)  # padded by one voxel per side along the first axis
NAT = tuple(GRID.shape)
LABELS = [1, 2, 3]
SPACING = (1.0, 1.5, 2.0)
BINS = 6


def surface_state(**over):
    return {'mean': t(f32, *VOL), 'm2': t(f32, *VOL), 'count': t(i32, *VOL), **over}


def seg_pair(chains=1, **over):
    return {'seg_fixed': vol(i16, chains), 'seg_moving': vol(i16), 'labels': LABELS, 'spacing': SPACING, **over}


def moments(**over):
    return {'mean': field(2, Cn), 'm2': field(2, Cn), **over}


def jacobian_state(**over):
    return {'folds': t(i32, *VOL), 'mean': t(f32, *VOL), 'm2': t(f32, *VOL), **over}


def covariance_state(**over):
    return {'mean': t(f32, 3, *VOL), 'comoment': t(f32, 6, *VOL), **over}


def quantile_state(**over):
    return {'centre': t(f32, 3, *VOL), 'hist': t(u16, 3, BINS, *VOL), **over}


def quantile_final(**over):
    return quantile_state(**{'n': 5, 'width': (0.5, 0.25, 0.125), 'scale': (1.0, 2.0, 3.0), 'probs': (0.025, 0.5, 0.975), **over})


def ice_state(**over):
    return {'mean': t(f32, *VOL), 'peak': t(f32, *VOL), **over}


def local_state(**over):
    return {'mean': t(f32, *VOL), 'low': t(f32, *VOL), 'count': t(i32, *VOL), **over}


def ice(**over):
    return {'t_a': field(), 'd_a': field(), 'd_b': field(), **over}


def pair(chains=1, **over):
    return {'fixed': vol(f32, chains), 'moving': vol(), **over}


def native(**over):
    return {'displacement': field(), 'grid': GRID, **over}


def nat(dtype, chains=Cn):
    return t(dtype, chains, 1, *NAT)


K = 3


def landmarks(**over):
    state = ops.landmark_state(K, 'cpu')
    state.update(over.pop('state', {}))
    return {'state': state, 'target': t(f32, K, 3), **over}


MASKS = {'bool': lambda: t(b8, *VOL), 'uint8': lambda: t(u8, *VOL)}
MASKS5 = {'bool': lambda: t(b8, 1, 1, *VOL), 'uint8': lambda: t(u8, 1, 1, *VOL)}
R = {'fixed_range': (-1.0, 2.0), 'moving_range': (-2.0, 3.0)}
inf, nan = math.inf, math.nan

# (id, function, keyword arguments; '*' holds positional ones).  Ids: function/what.  A '!' starts the id of a malformed call,
# '!!' that of a call with two violations, one on each side of the function's first dev_ptr: the first one must be reported.
CASES = [
    ('sobolev_kernel_1d/s2', 'sobolev_kernel_1d', lambda: dict(s=2, lam=0.5)),
    ('control_grid_size/456', 'control_grid_size', lambda: dict(dims=VOL, cps=CPS)),

    ('perturb_smooth/all', 'perturb_smooth', lambda: dict(v=field(), kernel=[0.25, 0.5, 0.25], sigma=field(), eps=field(), tau=0.125,
                                                         seed=3, iteration=7)),
    ('perturb_smooth/smooth_only', 'perturb_smooth', lambda: dict(v=field(), kernel=np.float32([0.1, 0.2, 0.4, 0.2, 0.1]))),
    ('perturb_smooth/perturb_only', 'perturb_smooth', lambda: dict(v=field(), kernel=None, sigma=field(), tau=1)),
    ('perturb_smooth/!channels', 'perturb_smooth', lambda: dict(v=vol(), kernel=None)),
    ('perturb_smooth/!dim', 'perturb_smooth', lambda: dict(v=t(f32, 3, D, H, W), kernel=None)),

    ('svf_exp_fwd/outputs', 'svf_exp_fwd', lambda: dict(v=field(), no_steps=3)),
    ('svf_exp_fwd/steps_only', 'svf_exp_fwd', lambda: dict(v=field(), no_steps=2, want_outputs=False)),
    ('svf_exp_fwd/!channels', 'svf_exp_fwd', lambda: dict(v=vol())),
    ('svf_exp_bwd/plain', 'svf_exp_bwd', lambda: dict(v=field(), steps=field(3, Cn), g_last=field())),
    ('svf_exp_bwd/strided_g_last', 'svf_exp_bwd', lambda: dict(v=field(), steps=field(3, Cn),
                                                               g_last=t(f32, Cn, 3, D, W, H).transpose(3, 4))),
    ('svf_exp_bwd/!channels', 'svf_exp_bwd', lambda: dict(v=vol(), steps=field(3, Cn), g_last=field())),
    ('svf_exp_inverse/plain', 'svf_exp_inverse', lambda: dict(v=field(), no_steps=4)),
    ('svf_exp_inverse/!channels', 'svf_exp_inverse', lambda: dict(v=vol())),

    ('ffd_up/plain', 'ffd_up', lambda: dict(v_cp=t(f32, Cn, 3, *ops.control_grid_size(VOL, CPS)), dims=VOL, cps=CPS)),
    ('ffd_up/!grid', 'ffd_up', lambda: dict(v_cp=t(f32, Cn, 3, 5, 5, 5), dims=VOL, cps=CPS)),
    ('ffd_adjoint/plain', 'ffd_adjoint', lambda: dict(g_dense=field(), cps=CPS)),
    ('ffd_adjoint/strided', 'ffd_adjoint', lambda: dict(g_dense=t(f32, Cn, 3, D, W, H).transpose(3, 4), cps=CPS)),
    ('ffd_adjoint/!channels', 'ffd_adjoint', lambda: dict(g_dense=vol(), cps=CPS)),

    ('warp_displacement/shared', 'warp_displacement', lambda: dict(im=vol(f32, 1), d_last=field())),
    ('warp_displacement/per_chain_jitter', 'warp_displacement', lambda: dict(im=vol(), d_last=field(), unif=field(), alpha=0.5, seed=1,
                                                                             iteration=2)),
    ('warp_displacement/!d_last', 'warp_displacement', lambda: dict(im=vol(), d_last=vol())),
    ('warp_displacement/!image', 'warp_displacement', lambda: dict(im=t(f32, Cn, 1, D, W, H), d_last=field())),
    ('warp_displacement/!image_chains', 'warp_displacement', lambda: dict(im=vol(f32, 3), d_last=field())),
    ('warp_displacement/!unif', 'warp_displacement', lambda: dict(im=vol(), d_last=field(), unif=field(1))),
    ('warp_displacement_bwd/shared', 'warp_displacement_bwd', lambda: dict(im=vol(f32, 1), d_last=field(), g_warped=vol())),
    ('warp_displacement_bwd/per_chain_jitter', 'warp_displacement_bwd', lambda: dict(
        im=vol(), d_last=field(), g_warped=t(f32, Cn, 1, D, W, H).transpose(3, 4), unif=field(), alpha=0.25, seed=5, iteration=6)),
    ('warp_displacement_bwd/!d_last', 'warp_displacement_bwd', lambda: dict(im=vol(), d_last=vol(), g_warped=vol())),
    ('warp_displacement_bwd/!image', 'warp_displacement_bwd', lambda: dict(im=t(f32, Cn, D, H, W), d_last=field(), g_warped=vol())),
    ('warp_displacement_bwd/!g_warped_shared', 'warp_displacement_bwd', lambda: dict(im=vol(), d_last=field(), g_warped=vol(f32, 1))),
    ('warp_displacement_bwd/!unif', 'warp_displacement_bwd', lambda: dict(im=vol(), d_last=field(), g_warped=vol(), unif=vol())),

    ('warp/float32_shared', 'warp', lambda: dict(im=vol(f32, 1), transformation=field())),
    ('warp/float32_per_chain', 'warp', lambda: dict(im=vol(), transformation=field())),
    ('warp/bool', 'warp', lambda: dict(im=vol(b8), transformation=field())),
    ('warp/int16_shared', 'warp', lambda: dict(im=vol(i16, 1), transformation=field())),
    ('warp/!transformation', 'warp', lambda: dict(im=vol(), transformation=vol())),
    ('warp/!image', 'warp', lambda: dict(im=t(f32, Cn, 1, H, D, W), transformation=field())),
    ('warp/!image_chains', 'warp', lambda: dict(im=vol(f32, 3), transformation=field())),
    ('warp/!dtype', 'warp', lambda: dict(im=vol(f64), transformation=field())),
    ('warp/!dtype_uint8', 'warp', lambda: dict(im=vol(u8), transformation=field())),
    ('warp/!!image_then_pointer', 'warp', lambda: dict(im=vol(f32, 3), transformation=field().double())),
    ('warp/!!pointer_then_dtype', 'warp', lambda: dict(im=vol(f64), transformation=field().double())),

    ('lcc_normalise/plain', 'lcc_normalise', lambda: dict(im=vol(), s=2)),
    ('lcc_normalise/sigma', 'lcc_normalise', lambda: dict(im=vol(), s=1, want_sigma=True)),
    ('lcc_normalise/!channels', 'lcc_normalise', lambda: dict(im=field(), s=1)),
    ('lcc_map_fwd/shared', 'lcc_map_fwd', lambda: dict(fhat=vol(f32, 1), warped=vol(), s=2)),
    ('lcc_map_fwd/per_chain', 'lcc_map_fwd', lambda: dict(fhat=vol(), warped=vol(), s=1)),
    ('lcc_map_fwd/!warped', 'lcc_map_fwd', lambda: dict(fhat=vol(), warped=field(), s=1)),
    ('lcc_map_fwd/!fhat', 'lcc_map_fwd', lambda: dict(fhat=t(f32, Cn, 1, D, H, W + 1), warped=vol(), s=1)),
    ('lcc_map_bwd/shared', 'lcc_map_bwd', lambda: dict(fhat=vol(f32, 1), z=vol(), sigma_m=vol(), g_z=vol(), s=2)),
    ('lcc_map_bwd/per_chain_strided', 'lcc_map_bwd', lambda: dict(fhat=vol(), z=vol(), sigma_m=vol(),
                                                                  g_z=t(f32, Cn, 1, H, D, W).transpose(2, 3), s=1)),
    ('lcc_map_bwd/!z', 'lcc_map_bwd', lambda: dict(fhat=vol(), z=field(), sigma_m=vol(), g_z=vol(), s=1)),
    ('lcc_map_bwd/!fhat', 'lcc_map_bwd', lambda: dict(fhat=vol(f32, 3), z=vol(), sigma_m=vol(), g_z=vol(), s=1)),
    ('lcc_map_bwd/!sigma_m', 'lcc_map_bwd', lambda: dict(fhat=vol(), z=vol(), sigma_m=vol(f32, 1), g_z=vol(), s=1)),
    ('lcc_map_bwd/!g_z', 'lcc_map_bwd', lambda: dict(fhat=vol(), z=vol(), sigma_m=vol(), g_z=t(f32, Cn, 1, D, W, H), s=1)),

    ('reg_energy/plain', 'reg_energy', lambda: dict(v=field())),
    ('reg_energy/!channels', 'reg_energy', lambda: dict(v=vol())),
    ('gradient_operator/velocity', 'gradient_operator', lambda: dict(v=field())),
    ('gradient_operator/transformation', 'gradient_operator', lambda: dict(v=field(), transformation=True)),
    ('gradient_operator/!channels', 'gradient_operator', lambda: dict(v=vol())),
    ('log_det_jacobian/plain', 'log_det_jacobian', lambda: dict(transformation=field())),
    ('log_det_jacobian/!channels', 'log_det_jacobian', lambda: dict(transformation=vol())),

    ('label_surface_distance/shared', 'label_surface_distance', lambda: seg_pair()),
    ('label_surface_distance/per_chain_tensor_spacing', 'label_surface_distance', lambda: seg_pair(Cn, spacing=torch.tensor(SPACING))),
    ('label_surface_distance/numpy_spacing_one_label', 'label_surface_distance', lambda: seg_pair(labels=np.array([5]),
                                                                                                 spacing=np.array(SPACING))),
    ('label_surface_distance/no_labels', 'label_surface_distance', lambda: seg_pair(labels=[])),
    ('label_surface_distance/!moving', 'label_surface_distance', lambda: seg_pair(seg_moving=t(i16, Cn, 3, D, H, W))),
    ('label_surface_distance/!fixed', 'label_surface_distance', lambda: seg_pair(seg_fixed=t(i16, 1, 1, D, W, H))),
    ('label_surface_distance/!fixed_chains', 'label_surface_distance', lambda: seg_pair(3)),
    ('label_surface_distance/!fixed_dim', 'label_surface_distance', lambda: seg_pair(seg_fixed=t(i16, D, H, W))),
    ('label_surface_distance/!spacing', 'label_surface_distance', lambda: seg_pair(spacing=(1.0, 2.0))),
    ('label_surface_distance/!!fixed_then_pointer', 'label_surface_distance', lambda: seg_pair(3, seg_moving=vol(i32))),
    ('label_surface_distance/!!pointer_then_spacing', 'label_surface_distance', lambda: seg_pair(seg_moving=vol(i32), spacing=(1.0,))),

    ('label_hausdorff_distance/shared_default', 'label_hausdorff_distance', lambda: seg_pair()),
    ('label_hausdorff_distance/per_chain_two_percentiles', 'label_hausdorff_distance', lambda: seg_pair(Cn, percentiles=(50, 95.5),
                                                                                                       spacing=torch.tensor(SPACING))),
    ('label_hausdorff_distance/no_percentiles', 'label_hausdorff_distance', lambda: seg_pair(percentiles=())),
    ('label_hausdorff_distance/no_labels', 'label_hausdorff_distance', lambda: seg_pair(labels=[])),
    ('label_hausdorff_distance/!moving', 'label_hausdorff_distance', lambda: seg_pair(seg_moving=t(i16, Cn, D, H, W))),
    ('label_hausdorff_distance/!fixed', 'label_hausdorff_distance', lambda: seg_pair(seg_fixed=t(i16, 1, 1, H, D, W))),
    ('label_hausdorff_distance/!fixed_chains', 'label_hausdorff_distance', lambda: seg_pair(3)),
    ('label_hausdorff_distance/!spacing', 'label_hausdorff_distance', lambda: seg_pair(spacing=(1.0, 2.0, 3.0, 4.0))),
    ('label_hausdorff_distance/!!fixed_then_pointer', 'label_hausdorff_distance', lambda: seg_pair(3, seg_moving=vol(i32))),
    ('label_hausdorff_distance/!!pointer_then_spacing', 'label_hausdorff_distance', lambda: seg_pair(seg_fixed=vol(f32, 1), spacing=())),

    ('surface_posterior_update/plain', 'surface_posterior_update', lambda: seg_pair(**surface_state())),
    ('surface_posterior_update/tensor_spacing', 'surface_posterior_update', lambda: seg_pair(**surface_state(), labels=(7,),
                                                                                             spacing=torch.tensor(SPACING))),
    ('surface_posterior_update/!moving', 'surface_posterior_update', lambda: seg_pair(**surface_state(), seg_moving=field().to(i16))),
    ('surface_posterior_update/!fixed_per_chain', 'surface_posterior_update', lambda: seg_pair(Cn, **surface_state())),
    ('surface_posterior_update/!fixed_volume', 'surface_posterior_update', lambda: seg_pair(**surface_state(), seg_fixed=t(i16, *VOL))),
    ('surface_posterior_update/!mean_shape', 'surface_posterior_update', lambda: seg_pair(**surface_state(mean=t(f32, D, W, H)))),
    ('surface_posterior_update/!m2_dtype', 'surface_posterior_update', lambda: seg_pair(**surface_state(m2=t(f64, *VOL)))),
    ('surface_posterior_update/!count_dtype', 'surface_posterior_update', lambda: seg_pair(**surface_state(count=t(torch.int64, *VOL)))),
    ('surface_posterior_update/!spacing', 'surface_posterior_update', lambda: seg_pair(**surface_state(), spacing=(1.0, 1.0))),
    ('surface_posterior_update/!!state_then_pointer', 'surface_posterior_update', lambda: seg_pair(
        **surface_state(count=t(f32, *VOL)), seg_moving=vol(i32))),
    ('surface_posterior_update/!!pointer_then_spacing', 'surface_posterior_update', lambda: seg_pair(
        **surface_state(), seg_moving=vol(i32), spacing=(1.0, 1.0))),

    ('surface_posterior_finalize/levels', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16, 1), labels=LABELS, **surface_state(),
                                                                                     levels=(0.5, 0.9))),
    ('surface_posterior_finalize/no_levels_bool_mask', 'surface_posterior_finalize', lambda: dict(
        seg_fixed=vol(i16, 1), labels=LABELS, **surface_state(), levels=(), mask=MASKS['bool']())),
    ('surface_posterior_finalize/four_levels_uint8_mask', 'surface_posterior_finalize', lambda: dict(
        seg_fixed=vol(i16, 1), labels=[4], **surface_state(), levels=(0.25, 0.5, 0.75, 0.95), mask=MASKS['uint8']())),
    ('surface_posterior_finalize/!fixed_chains', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16), labels=LABELS,
                                                                                            **surface_state(), levels=())),
    ('surface_posterior_finalize/!fixed_dim', 'surface_posterior_finalize', lambda: dict(seg_fixed=t(i16, *VOL), labels=LABELS,
                                                                                         **surface_state(), levels=())),
    ('surface_posterior_finalize/!m2_shape', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16, 1), labels=LABELS,
                                                                                        **surface_state(m2=t(f32, 1, *VOL)), levels=())),
    ('surface_posterior_finalize/!mask', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16, 1), labels=LABELS, **surface_state(),
                                                                                    levels=(), mask=t(f32, *VOL))),
    ('surface_posterior_finalize/!levels_many', 'surface_posterior_finalize', lambda: dict(
        seg_fixed=vol(i16, 1), labels=LABELS, **surface_state(), levels=(0.1, 0.2, 0.3, 0.4, 0.5))),
    ('surface_posterior_finalize/!levels_range', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16, 1), labels=LABELS,
                                                                                            **surface_state(), levels=(0.5, 1.0))),
    ('surface_posterior_finalize/!levels_order', 'surface_posterior_finalize', lambda: dict(seg_fixed=vol(i16, 1), labels=LABELS,
                                                                                            **surface_state(), levels=(0.9, 0.5))),

    ('chain_moments_update/plain', 'chain_moments_update', lambda: dict(x=field(), **moments(), half=1, k=4)),
    ('chain_moments_update/!x', 'chain_moments_update', lambda: dict(x=vol(), **moments(), half=0, k=1)),
    ('chain_moments_update/!mean', 'chain_moments_update', lambda: dict(x=field(), **moments(mean=field(1, Cn)), half=0, k=1)),
    ('chain_moments_update/!m2', 'chain_moments_update', lambda: dict(x=field(), **moments(m2=field(2, Cn + 1)), half=0, k=1)),
    ('split_rhat/plain', 'split_rhat', lambda: dict(**moments(), n=8)),
    ('split_rhat/bool_mask_thresholds', 'split_rhat', lambda: dict(**moments(), n=8, mask=MASKS['bool'](), thresholds=(1.05, 1.2))),
    ('split_rhat/uint8_mask_5d', 'split_rhat', lambda: dict(**moments(), n=8, mask=MASKS5['uint8']())),
    ('split_rhat/!mean', 'split_rhat', lambda: dict(**moments(mean=field(Cn), m2=field(Cn)), n=8)),
    ('split_rhat/!halves', 'split_rhat', lambda: dict(**moments(mean=field(3, Cn), m2=field(3, Cn)), n=8)),
    ('split_rhat/!m2', 'split_rhat', lambda: dict(**moments(m2=field(2, 3)), n=8)),
    ('split_rhat/!mask_dtype', 'split_rhat', lambda: dict(**moments(), n=8, mask=t(i32, *VOL))),
    ('split_rhat/!mask_count', 'split_rhat', lambda: dict(**moments(), n=8, mask=t(b8, Cn, *VOL))),
    ('split_rhat/!thresholds', 'split_rhat', lambda: dict(**moments(), n=8, thresholds=(1.01,))),
    ('chain_variogram_update/plain', 'chain_variogram_update', lambda: dict(x=field(), ring=field(3, Cn), vsum=field(3), k=2)),
    ('chain_variogram_update/!x', 'chain_variogram_update', lambda: dict(x=vol(), ring=field(3, Cn), vsum=field(3), k=2)),
    ('chain_variogram_update/!ring', 'chain_variogram_update', lambda: dict(x=field(), ring=field(3, 1), vsum=field(3), k=2)),
    ('chain_variogram_update/!ring_dim', 'chain_variogram_update', lambda: dict(x=field(), ring=field(), vsum=field(3), k=2)),
    ('chain_variogram_update/!vsum', 'chain_variogram_update', lambda: dict(x=field(), ring=field(3, Cn), vsum=field(4), k=2)),
    ('split_ess/plain', 'split_ess', lambda: dict(**moments(), vsum=field(3), n=8)),
    ('split_ess/bool_mask_threshold', 'split_ess', lambda: dict(**moments(), vsum=field(5), n=8, mask=MASKS['bool'](), threshold=100)),
    ('split_ess/uint8_mask', 'split_ess', lambda: dict(**moments(), vsum=field(3), n=8, mask=MASKS['uint8']())),
    ('split_ess/!mean', 'split_ess', lambda: dict(**moments(mean=t(f32, 2, Cn, 1, D, H, W)), vsum=field(3), n=8)),
    ('split_ess/!m2', 'split_ess', lambda: dict(**moments(m2=field(2, 1)), vsum=field(3), n=8)),
    ('split_ess/!vsum', 'split_ess', lambda: dict(**moments(), vsum=t(f32, 3, 3, D, W, H), n=8)),
    ('split_ess/!vsum_dim', 'split_ess', lambda: dict(**moments(), vsum=field(3, Cn), n=8)),
    ('split_ess/!mask', 'split_ess', lambda: dict(**moments(), vsum=field(3), n=8, mask=t(f32, *VOL))),

    ('label_posterior_update/plain', 'label_posterior_update', lambda: dict(seg_warped=vol(i16), labels=LABELS, counts=t(i32, 3, *VOL),
                                                                            volume=t(f64, 3, 2), records_before=4)),
    ('label_posterior_update/!seg_warped', 'label_posterior_update', lambda: dict(seg_warped=field().to(i16), labels=LABELS,
                                                                                  counts=t(i32, 3, *VOL), volume=t(f64, 3, 2), records_before=0)),
    ('label_posterior_update/!counts_planes', 'label_posterior_update', lambda: dict(seg_warped=vol(i16), labels=LABELS, counts=t(i32, 2, *VOL),
                                                                                     volume=t(f64, 3, 2), records_before=0)),
    ('label_posterior_update/!counts_dtype', 'label_posterior_update', lambda: dict(seg_warped=vol(i16), labels=LABELS, counts=t(f32, 3, *VOL),
                                                                                    volume=t(f64, 3, 2), records_before=0)),
    ('label_posterior_update/!volume_shape', 'label_posterior_update', lambda: dict(seg_warped=vol(i16), labels=LABELS, counts=t(i32, 3, *VOL),
                                                                                    volume=t(f64, 2, 3), records_before=0)),
    ('label_posterior_update/!volume_dtype', 'label_posterior_update', lambda: dict(seg_warped=vol(i16), labels=LABELS, counts=t(i32, 3, *VOL),
                                                                                    volume=t(f32, 3, 2), records_before=0)),
    ('label_posterior_finalize/volume', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=LABELS,
                                                                                 seg_fixed=t(i16, *VOL))),
    ('label_posterior_finalize/5d_bool_mask', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=LABELS,
                                                                                       seg_fixed=vol(i16, 1), mask=MASKS['bool']())),
    ('label_posterior_finalize/uint8_mask', 'label_posterior_finalize', lambda: dict(counts=t(i32, 1, *VOL), n=6, labels=[9],
                                                                                     seg_fixed=t(i16, *VOL), mask=MASKS['uint8']())),
    ('label_posterior_finalize/!counts', 'label_posterior_finalize', lambda: dict(counts=t(i32, *VOL), n=6, labels=LABELS,
                                                                                  seg_fixed=t(i16, *VOL))),
    ('label_posterior_finalize/!labels', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=[1, 2],
                                                                                  seg_fixed=t(i16, *VOL))),
    ('label_posterior_finalize/!seg_fixed', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=LABELS,
                                                                                     seg_fixed=t(i16, D, W, H))),
    ('label_posterior_finalize/!seg_fixed_chains', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=LABELS,
                                                                                            seg_fixed=vol(i16))),
    ('label_posterior_finalize/!mask', 'label_posterior_finalize', lambda: dict(counts=t(i32, 3, *VOL), n=6, labels=LABELS,
                                                                                seg_fixed=t(i16, *VOL), mask=t(i16, *VOL))),

    ('jacobian_posterior_update/plain', 'jacobian_posterior_update', lambda: dict(transformation=field(), **jacobian_state(),
                                                                                  records_before=2)),
    ('jacobian_posterior_update/!transformation', 'jacobian_posterior_update', lambda: dict(transformation=vol(), **jacobian_state(),
                                                                                            records_before=2)),
    ('jacobian_posterior_update/!folds_dtype', 'jacobian_posterior_update', lambda: dict(
        transformation=field(), **jacobian_state(folds=t(f32, *VOL)), records_before=2)),
    ('jacobian_posterior_update/!mean_shape', 'jacobian_posterior_update', lambda: dict(
        transformation=field(), **jacobian_state(mean=t(f32, H, D, W)), records_before=2)),
    ('jacobian_posterior_update/!m2_dtype', 'jacobian_posterior_update', lambda: dict(
        transformation=field(), **jacobian_state(m2=t(f64, *VOL)), records_before=2)),
    ('jacobian_posterior_finalize/plain', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(), n=6)),
    ('jacobian_posterior_finalize/bool_mask', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(), n=6, mask=MASKS['bool']())),
    ('jacobian_posterior_finalize/uint8_mask', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(), n=6, mask=MASKS5['uint8']())),
    ('jacobian_posterior_finalize/!folds_dim', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(folds=t(i32, 1, *VOL)), n=6)),
    ('jacobian_posterior_finalize/!folds_dtype', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(folds=t(i16, *VOL)), n=6)),
    ('jacobian_posterior_finalize/!m2_shape', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(m2=t(f32, D, H, W + 1)), n=6)),
    ('jacobian_posterior_finalize/!mask', 'jacobian_posterior_finalize', lambda: dict(**jacobian_state(), n=6, mask=t(u8, D, H))),

    ('displacement_covariance_update/plain', 'displacement_covariance_update', lambda: dict(displacement=field(), **covariance_state(),
                                                                                            records_before=0)),
    ('displacement_covariance_update/!displacement', 'displacement_covariance_update', lambda: dict(
        displacement=vol(), **covariance_state(), records_before=0)),
    ('displacement_covariance_update/!mean', 'displacement_covariance_update', lambda: dict(
        displacement=field(), **covariance_state(mean=t(f32, 6, *VOL)), records_before=0)),
    ('displacement_covariance_update/!comoment_dtype', 'displacement_covariance_update', lambda: dict(
        displacement=field(), **covariance_state(comoment=t(f64, 6, *VOL)), records_before=0)),
    ('displacement_covariance_finalize/plain', 'displacement_covariance_finalize', lambda: dict(**covariance_state(), n=4,
                                                                                                scale=(1.0, 2.0, 3.5))),
    ('displacement_covariance_finalize/bool_mask', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(), n=4, scale=torch.tensor([1.0, 2.0, 3.5]), mask=MASKS['bool']())),
    ('displacement_covariance_finalize/uint8_mask', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(), n=4, scale=[1, 2, 3], mask=MASKS['uint8']())),
    ('displacement_covariance_finalize/!mean_dim', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(mean=t(f32, 1, 3, *VOL)), n=4, scale=(1.0, 1.0, 1.0))),
    ('displacement_covariance_finalize/!mean_channels', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(mean=t(f32, 2, *VOL)), n=4, scale=(1.0, 1.0, 1.0))),
    ('displacement_covariance_finalize/!comoment', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(comoment=t(f32, 3, *VOL)), n=4, scale=(1.0, 1.0, 1.0))),
    ('displacement_covariance_finalize/!mask', 'displacement_covariance_finalize', lambda: dict(
        **covariance_state(), n=4, scale=(1.0, 1.0, 1.0), mask=t(f64, *VOL))),
    ('displacement_covariance_finalize/!scale', 'displacement_covariance_finalize', lambda: dict(**covariance_state(), n=4, scale=(1.0, 1.0))),

    ('displacement_quantiles_update/plain', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(), inv_width=(2.0, 4.0, 8.0), records_before=10)),
    ('displacement_quantiles_update/!displacement', 'displacement_quantiles_update', lambda: dict(
        displacement=vol(), **quantile_state(), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!hist_dim', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(hist=t(u16, BINS, *VOL)), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!bins_odd', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(hist=t(u16, 3, 5, *VOL)), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!centre', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(centre=t(f32, *VOL)), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!hist_dtype', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(hist=t(i16, 3, BINS, *VOL)), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!hist_shape', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(hist=t(u16, 3, BINS, D, W, H)), inv_width=(2.0, 4.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!records_negative', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(), inv_width=(2.0, 4.0, 8.0), records_before=-1)),
    ('displacement_quantiles_update/!records_full', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(), inv_width=(2.0, 4.0, 8.0), records_before=65534)),
    ('displacement_quantiles_update/!inv_width', 'displacement_quantiles_update', lambda: dict(
        displacement=field(), **quantile_state(), inv_width=(2.0, 0.0, 8.0), records_before=0)),
    ('displacement_quantiles_update/!!records_then_pointer', 'displacement_quantiles_update', lambda: dict(
        displacement=field().double(), **quantile_state(), inv_width=(2.0, 4.0), records_before=-1)),
    ('displacement_quantiles_update/!!pointer_then_inv_width', 'displacement_quantiles_update', lambda: dict(
        displacement=field().double(), **quantile_state(), inv_width=(2.0, 4.0), records_before=0)),
    ('displacement_quantiles_finalize/plain', 'displacement_quantiles_finalize', lambda: quantile_final()),
    ('displacement_quantiles_finalize/bool_mask_two_probs', 'displacement_quantiles_finalize', lambda: quantile_final(
        probs=[0.05, 0.95], mask=MASKS['bool']())),
    ('displacement_quantiles_finalize/uint8_mask', 'displacement_quantiles_finalize', lambda: quantile_final(mask=MASKS['uint8']())),
    ('displacement_quantiles_finalize/!centre_dim', 'displacement_quantiles_finalize', lambda: quantile_final(centre=t(f32, *VOL))),
    ('displacement_quantiles_finalize/!bins', 'displacement_quantiles_finalize', lambda: quantile_final(hist=t(u16, 3, 2, *VOL))),
    ('displacement_quantiles_finalize/!centre', 'displacement_quantiles_finalize', lambda: quantile_final(centre=t(f64, 3, *VOL))),
    ('displacement_quantiles_finalize/!hist', 'displacement_quantiles_finalize', lambda: quantile_final(hist=t(u16, 2, BINS, *VOL))),
    ('displacement_quantiles_finalize/!mask', 'displacement_quantiles_finalize', lambda: quantile_final(mask=t(b8, D, H, W + 1))),
    ('displacement_quantiles_finalize/!probs_one', 'displacement_quantiles_finalize', lambda: quantile_final(probs=(0.5,))),
    ('displacement_quantiles_finalize/!probs_many', 'displacement_quantiles_finalize', lambda: quantile_final(
        probs=[0.1 * i for i in range(1, 10)])),
    ('displacement_quantiles_finalize/!probs_order', 'displacement_quantiles_finalize', lambda: quantile_final(probs=(0.5, 0.25))),
    ('displacement_quantiles_finalize/!probs_range', 'displacement_quantiles_finalize', lambda: quantile_final(probs=(0.0, 0.5))),
    ('displacement_quantiles_finalize/!n_zero', 'displacement_quantiles_finalize', lambda: quantile_final(n=0)),
    ('displacement_quantiles_finalize/!n_large', 'displacement_quantiles_finalize', lambda: quantile_final(n=65536)),
    ('displacement_quantiles_finalize/!width', 'displacement_quantiles_finalize', lambda: quantile_final(width=(0.5, inf, 0.5))),
    ('displacement_quantiles_finalize/!scale', 'displacement_quantiles_finalize', lambda: quantile_final(scale=(1.0, 2.0))),

    ('inverse_consistency/plain', 'inverse_consistency', lambda: ice()),
    ('inverse_consistency/scale_residual_volume_mask', 'inverse_consistency', lambda: ice(scale=(1.0, 2.0, 4.0), mask=MASKS['bool'](),
                                                                                          want_residual=True)),
    ('inverse_consistency/shared_uint8_mask', 'inverse_consistency', lambda: ice(mask=MASKS5['uint8']())),
    ('inverse_consistency/per_chain_bool_mask', 'inverse_consistency', lambda: ice(mask=vol(b8))),
    ('inverse_consistency/!t_a', 'inverse_consistency', lambda: ice(t_a=vol())),
    ('inverse_consistency/!d_a', 'inverse_consistency', lambda: ice(d_a=field(1))),
    ('inverse_consistency/!d_b', 'inverse_consistency', lambda: ice(d_b=t(f32, Cn, 3, D, W, H))),
    ('inverse_consistency/!mask_dtype', 'inverse_consistency', lambda: ice(mask=vol(f32, 1))),
    ('inverse_consistency/!mask_count', 'inverse_consistency', lambda: ice(mask=vol(b8, 3))),
    ('inverse_consistency/!mask_shape', 'inverse_consistency', lambda: ice(mask=t(b8, D, W, H))),
    ('inverse_consistency/!scale', 'inverse_consistency', lambda: ice(scale=(1.0, -1.0, 1.0))),
    ('inverse_consistency/!!mask_then_pointer', 'inverse_consistency', lambda: ice(t_a=field().double(), d_a=field().double(),
                                                                                   d_b=field().double(), mask=vol(f32, 1))),
    ('inverse_consistency/!!pointer_then_scale', 'inverse_consistency', lambda: ice(d_b=field().half(), scale=(1.0, nan, 1.0))),
    ('inverse_consistency_update/plain', 'inverse_consistency_update', lambda: dict(norm=vol(), **ice_state(), records_before=3)),
    ('inverse_consistency_update/!norm', 'inverse_consistency_update', lambda: dict(norm=field(), **ice_state(), records_before=3)),
    ('inverse_consistency_update/!mean', 'inverse_consistency_update', lambda: dict(norm=vol(), **ice_state(mean=t(f32, 1, *VOL)),
                                                                                    records_before=3)),
    ('inverse_consistency_update/!peak', 'inverse_consistency_update', lambda: dict(norm=vol(), **ice_state(peak=t(f64, *VOL)),
                                                                                    records_before=3)),
    ('inverse_consistency_finalize/plain', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=0.5)),
    ('inverse_consistency_finalize/bool_mask', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=2, mask=MASKS['bool']())),
    ('inverse_consistency_finalize/uint8_mask', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=0.5,
                                                                                             mask=MASKS['uint8']())),
    ('inverse_consistency_finalize/!mean_dim', 'inverse_consistency_finalize', lambda: dict(**ice_state(mean=t(f32, 1, *VOL)), threshold=0.5)),
    ('inverse_consistency_finalize/!mean_dtype', 'inverse_consistency_finalize', lambda: dict(**ice_state(mean=t(f64, *VOL)), threshold=0.5)),
    ('inverse_consistency_finalize/!peak', 'inverse_consistency_finalize', lambda: dict(**ice_state(peak=t(f32, D, W, H)), threshold=0.5)),
    ('inverse_consistency_finalize/!mask', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=0.5, mask=t(i16, *VOL))),
    ('inverse_consistency_finalize/!threshold_zero', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=0.0)),
    ('inverse_consistency_finalize/!threshold_inf', 'inverse_consistency_finalize', lambda: dict(**ice_state(), threshold=inf)),

    ('native_warp/image_default_fill', 'native_warp', lambda: native(im=nat(f32))),
    ('native_warp/everything_shared', 'native_warp', lambda: native(im=nat(f32, 1), seg=nat(i16, 1), mask=nat(b8, 1), fill=-1,
                                                                    want_displacement=GRID.voxel_scale())),
    ('native_warp/seg_and_uint8_mask_per_chain', 'native_warp', lambda: native(seg=nat(i16), mask=nat(u8))),
    ('native_warp/displacement_only', 'native_warp', lambda: native(want_displacement=(1.0, 2.0, 3.0), fill=5.0)),
    ('native_warp/!displacement', 'native_warp', lambda: native(displacement=vol(), im=nat(f32))),
    ('native_warp/!grid', 'native_warp', lambda: native(displacement=t(f32, Cn, 3, D, W, H), im=nat(f32))),
    ('native_warp/!nothing', 'native_warp', lambda: native()),
    ('native_warp/!im_shape', 'native_warp', lambda: native(im=vol())),
    ('native_warp/!seg_chains', 'native_warp', lambda: native(seg=nat(i16, 3))),
    ('native_warp/!im_dtype', 'native_warp', lambda: native(im=nat(f64))),
    ('native_warp/!seg_dtype', 'native_warp', lambda: native(seg=nat(i32))),
    ('native_warp/!mask_dtype', 'native_warp', lambda: native(mask=nat(i16))),
    ('native_warp/!leading', 'native_warp', lambda: native(im=nat(f32, 1), seg=nat(i16))),
    ('native_warp/!fill', 'native_warp', lambda: native(im=nat(f32), fill=inf)),
    ('native_warp/!fill_from_image', 'native_warp', lambda: native(im=nat(f32) * nan)),
    ('native_warp/!want_displacement_count', 'native_warp', lambda: native(want_displacement=(1.0, 2.0))),
    ('native_warp/!want_displacement_nan', 'native_warp', lambda: native(seg=nat(i16), want_displacement=(1.0, nan, 2.0))),

    ('intensity_ranges/two', 'intensity_ranges', lambda: {'*': [vol(), torch.tensor([3.0, inf, -2.5, nan, -inf])]}),
    ('intensity_ranges/one', 'intensity_ranges', lambda: {'*': [t(f32, 7)]}),
    ('image_similarity/ranges_given', 'image_similarity', lambda: pair(**R)),
    ('image_similarity/ranges_found_per_chain_hist', 'image_similarity', lambda: pair(Cn, bins=8, want_hist=True)),
    ('image_similarity/fixed_range_bool_mask', 'image_similarity', lambda: pair(fixed_range=(0, 1), mask=MASKS5['bool']())),
    ('image_similarity/moving_range_uint8_mask', 'image_similarity', lambda: pair(moving_range=(-5.0, 5.0), mask=MASKS5['uint8']())),
    ('image_similarity/!moving', 'image_similarity', lambda: pair(moving=field())),
    ('image_similarity/!fixed', 'image_similarity', lambda: pair(fixed=t(f32, 1, 1, D, W, H))),
    ('image_similarity/!mask_volume', 'image_similarity', lambda: pair(**R, mask=MASKS['bool']())),
    ('image_similarity/!mask_per_chain', 'image_similarity', lambda: pair(**R, mask=vol(u8))),
    ('image_similarity/!mask_dtype', 'image_similarity', lambda: pair(**R, mask=vol(f32, 1))),
    ('image_similarity/!bins_float', 'image_similarity', lambda: pair(**R, bins=16.0)),
    ('image_similarity/!bins_bool', 'image_similarity', lambda: pair(**R, bins=True)),

    ('local_similarity_constants/plain', 'local_similarity_constants', lambda: dict(**R)),
    ('local_similarity_constants/!fixed', 'local_similarity_constants', lambda: dict(fixed_range=(1.0, 1.0), moving_range=(0.0, 1.0))),
    ('local_similarity_constants/!moving', 'local_similarity_constants', lambda: dict(fixed_range=(0.0, 1.0), moving_range=(0.0, inf))),
    ('local_similarity/ranges_given', 'local_similarity', lambda: pair(**R)),
    ('local_similarity/ranges_found_per_chain_lncc', 'local_similarity', lambda: pair(Cn, radius=1, want=['lncc'])),
    ('local_similarity/fixed_range_bool_mask_ssim', 'local_similarity', lambda: pair(fixed_range=(0, 1), mask=MASKS5['bool'](),
                                                                                     want=('ssim',))),
    ('local_similarity/moving_range_uint8_mask_stats', 'local_similarity', lambda: pair(moving_range=(-5.0, 5.0), mask=MASKS5['uint8'](),
                                                                                        want=())),
    ('local_similarity/!moving', 'local_similarity', lambda: pair(moving=field())),
    ('local_similarity/!fixed', 'local_similarity', lambda: pair(fixed=vol(f32, 3))),
    ('local_similarity/!mask_volume', 'local_similarity', lambda: pair(**R, mask=MASKS['uint8']())),
    ('local_similarity/!mask_dtype', 'local_similarity', lambda: pair(**R, mask=vol(i16, 1))),
    ('local_similarity/!radius_float', 'local_similarity', lambda: pair(**R, radius=2.0)),
    ('local_similarity/!radius_bool', 'local_similarity', lambda: pair(**R, radius=False)),
    ('local_similarity/!want', 'local_similarity', lambda: pair(**R, want=('lncc', 'ncc'))),
    ('local_similarity/!range', 'local_similarity', lambda: pair(fixed_range=(2.0, 1.0))),
    ('local_similarity/!range_found', 'local_similarity', lambda: pair(fixed=torch.zeros(1, 1, *VOL))),
    ('local_similarity/!!want_then_pointer', 'local_similarity', lambda: pair(moving=vol(f64), want=('x',), moving_range=(1.0, 0.0))),
    ('local_similarity/!!pointer_then_range', 'local_similarity', lambda: pair(moving=vol(f64), moving_range=(1.0, 0.0))),
    ('local_similarity_update/plain', 'local_similarity_update', lambda: dict(lncc=vol(), **local_state(), records_before=2)),
    ('local_similarity_update/!lncc', 'local_similarity_update', lambda: dict(lncc=field(), **local_state(), records_before=2)),
    ('local_similarity_update/!mean', 'local_similarity_update', lambda: dict(lncc=vol(), **local_state(mean=t(f64, *VOL)),
                                                                              records_before=2)),
    ('local_similarity_update/!low', 'local_similarity_update', lambda: dict(lncc=vol(), **local_state(low=t(f32, D, H)), records_before=2)),
    ('local_similarity_update/!count', 'local_similarity_update', lambda: dict(lncc=vol(), **local_state(count=t(f32, *VOL)),
                                                                               records_before=2)),
    ('local_similarity_finalize/plain', 'local_similarity_finalize', lambda: local_state()),
    ('local_similarity_finalize/bool_mask', 'local_similarity_finalize', lambda: local_state(mask=MASKS['bool']())),
    ('local_similarity_finalize/uint8_mask', 'local_similarity_finalize', lambda: local_state(mask=MASKS5['uint8']())),
    ('local_similarity_finalize/!mean_dim', 'local_similarity_finalize', lambda: local_state(mean=vol(f32, 1))),
    ('local_similarity_finalize/!low', 'local_similarity_finalize', lambda: local_state(low=t(f32, H, D, W))),
    ('local_similarity_finalize/!count', 'local_similarity_finalize', lambda: local_state(count=t(i16, *VOL))),
    ('local_similarity_finalize/!mask', 'local_similarity_finalize', lambda: local_state(mask=t(f32, *VOL))),

    ('transform_points/plain', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field())),
    ('transform_points/offset_scale_sampled', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field(), scale=(2, 3.0, 4.5),
                                                                               offset=t(f32, K, 3), want_sampled=True)),
    ('transform_points/!displacement', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=vol())),
    ('transform_points/!points_shape', 'transform_points', lambda: dict(points=t(f32, 3, K + 1), displacement=field())),
    ('transform_points/!points_dtype', 'transform_points', lambda: dict(points=t(f64, K, 3), displacement=field())),
    ('transform_points/!points_none', 'transform_points', lambda: dict(points=t(f32, 0, 3), displacement=field())),
    ('transform_points/!offset', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field(), offset=t(f32, K + 1, 3))),
    ('transform_points/!scale', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field(), scale=(1.0, 1.0, 0.0))),
    ('transform_points/!!offset_then_pointer', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field().double(),
                                                                                offset=t(f64, K, 3), scale=(1.0,))),
    ('transform_points/!!pointer_then_scale', 'transform_points', lambda: dict(points=t(f32, K, 3), displacement=field().double(),
                                                                               scale=(1.0,))),
    ('landmark_state/plain', 'landmark_state', lambda: dict(K=K, device='cpu')),
    ('landmark_update/plain', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K, 3), records_before=4)),
    ('landmark_update/!mapped_shape', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, 3, K + 1), records_before=0)),
    ('landmark_update/!mapped_dtype', 'landmark_update', lambda: landmarks(mapped=t(f64, Cn, K, 3), records_before=0)),
    ('landmark_update/!target', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K + 1, 3), records_before=0)),
    ('landmark_update/!state_shape', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K, 3), records_before=0,
                                                                          state={'comoment': t(f64, K, 3)})),
    ('landmark_update/!state_dtype', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K, 3), records_before=0,
                                                                          state={'count': t(torch.int64, K)})),
    ('landmark_update/!!target_then_pointer', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K, 3).transpose(0, 1).contiguous()
                                                                                   .transpose(0, 1), records_before=0, target=t(f32, K, 2))),
    ('landmark_update/!!pointer_then_state', 'landmark_update', lambda: landmarks(mapped=t(f32, Cn, K, 3).transpose(0, 1).contiguous()
                                                                                  .transpose(0, 1), records_before=0,
                                                                                  state={'tre_max': t(f32, K)})),
    ('landmark_finalize/plain', 'landmark_finalize', lambda: landmarks()),
    ('landmark_finalize/!target', 'landmark_finalize', lambda: landmarks(target=t(f32, K, 3).double())),
    ('landmark_finalize/!state_shape', 'landmark_finalize', lambda: landmarks(state={'mean': t(f64, K + 1, 3)})),
    ('landmark_finalize/!state_dtype', 'landmark_finalize', lambda: landmarks(state={'tre_m2': t(f32, K)})),
]
IDS = [c[0] for c in CASES]
RECORDED = {}


def expected():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('case_id,fn,kwargs', CASES, ids=IDS)
def test_calls_and_results(monkeypatch, case_id, fn, kwargs):
    got = run(monkeypatch, fn, kwargs())
    assert ('raises' in got) == ('!' in case_id), got
    RECORDED[case_id] = got
    if not RECORD:
        want = expected()[case_id]
        assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)


def test_the_table_is_the_fixture():
    """last in the file: with IRS_RECORD_OPS_CALLS=1 it writes what the cases above recorded, one case per line"""
    assert len(set(IDS)) == len(IDS)
    if RECORD:
        assert list(RECORDED) == IDS, 'record with the whole module selected'
        with open(GOLDEN, 'w') as f:
            f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(RECORDED[k], sort_keys=True)}' for k in IDS) + '\n}\n')
    assert sorted(expected()) == sorted(IDS)


def test_every_public_function_has_a_well_formed_case():
    public = [n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith('_')]
    assert len(public) == 47
    assert sorted(public) == sorted({fn for case_id, fn, _ in CASES if '!' not in case_id})
