"""The kernels that cap their grid, the shapes that take each of them past its cap, and the inputs and float64 references of
tests/test_grid_caps_host.py and tests/test_gpu_grid_caps.py.

Almost every reduction and streaming kernel outside the transition launches min(ceil(units / 256), cap) blocks of 256 threads;
past the cap every thread walks the rest of the array in a grid-stride loop ("trips") and a second stage folds the rows of
per-block partials.  RECORDS holds one record per such launch: the family, the kernel, the unit a thread takes per trip (1, 4
or 8 elements, a row of voxels, a work item), the cap, where the cap is defined (file, name of the constant and the regular
expression that reads it), the launcher's rule restated in Python, and the shape chosen for it: the smallest convenient ragged
shape that crosses the cap, whose last trip is ragged, that takes the scalar or the vector form as meant and that is no larger
than 1.5 x the threshold (`shape_problems`).  `trip_of` says which trip and which block an element falls in; the input builders
use it to give the later trips another mean, spread, mask density and label mix, and to put the extremes and the non-finite or
masked-out elements into the last, ragged trip.

A case (`case(name)`) bundles the inputs of one family with `reference(weight)`: the family's own float64 restatement evaluated
with every element counted `weight` times.  weight = 1 is the value the device must reproduce; 0 after the first trip, 2 on
the last trip and 0 beyond the first 256 rows of partials are the three mistakes a capped kernel can make without any
result below the cap changing.  tests/test_grid_caps_host.py proves on the CPU that every summary column tells them apart by at
least 1000 times the tolerance the GPU test holds it to.
"""
import functools
import math
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('ir_sgmcmc_amd', 'csrc')
HEADER = os.path.join('include', 'irsgmcmc.h')
BLOCK = 256
f32 = np.float32

# rule: 'stream' min(ceil(units / per_block), cap) blocks; 'local' the work items of local_similarity_geometry; 'scan' the
# chunks of cc_blocks, `per` consecutive ones per thread of one block of `cap` threads
# form: 'scalar' / 'vector' where the launcher has both and the shape must pick this one; 'only' where it has one
# count: how the launcher counts elements from the shape and the chains: V, 3V, C3V, rows (D H), work, chunks, components
Record = namedtuple('Record', 'family kernel form unit per_block cap count rule source constant pattern shape chains note')


def _r(family, kernel, form, unit, cap, count, source, constant, pattern, shape, chains=1, per_block=BLOCK, rule='stream', note=''):
    return Record(family, kernel, form, unit, per_block, cap, count, rule, source, constant, pattern, tuple(shape), chains, note)


def _hip(name):
    return os.path.join(CSRC, name)


_STREAM = r'int {}\(int64_t n\) \{{[^}}]*?, (\d+)\); \}}'
_WS = r'#define {} \((?:IRS_MAX_CHAINS \* )?(\d+) \*'
S41, S45, S57, S65, S71 = (41, 41, 41), (45, 45, 45), (57, 57, 57), (65, 65, 65), (71, 71, 71)
DIAG = (89, 88, 90)       # 704 880 voxels, a multiple of 4: the vector form of the variogram update, and both finalizes
MOM = (71, 71, 72)        # 362 952 voxels, two chains: 2 177 712 elements per half, 544 428 units of four
BIG = (101, 102, 103)     # 1 061 106 voxels: the 4096-block streams, the component scan with two chunks per thread
BIG4 = (101, 102, 104)    # 1 071 408 voxels, a multiple of 4: the vector histograms
LOCAL = (1361, 17, 33)    # 6 tiles x 171 segments of 8 planes = 1026 work items (local_similarity_geometry, radius 1)
LABEL8 = (130, 127, 128)  # 2 113 280 voxels, a multiple of 8
SURF = (47, 45, 9)        # 2115 rows

RECORDS = (
    _r('modes', 'modes_gram_partial_kernel', 'only', 1, 256, 'V', _hip('modes_kernels.hip'), 'kGramMaxChunks',
       r'constexpr int kGramMaxChunks = (\d+);', S41),
    _r('preconditioner', 'precond_mean_kernel<0>', 'only', 1, 1024, '3V', _hip('precond_kernels.hip'), 'kPartialRows',
       r'constexpr int kPartialRows = (\d+);', S45),
    _r('preconditioner', 'precond_mean_kernel<1>', 'only', 1, 1024, '3V', _hip('precond_kernels.hip'), 'kPartialRows',
       r'constexpr int kPartialRows = (\d+);', S45),
    _r('preconditioner', 'precond_field_kernel', 'only', 1, 1024, '3V', _hip('precond_kernels.hip'), 'kPartialRows',
       r'constexpr int kPartialRows = (\d+);', S45),
    _r('preconditioner', 'precond_mean_finish_kernel', 'only', 1, 1024, '3V', _hip('precond_kernels.hip'), 'kPartialRows',
       r'constexpr int kPartialRows = (\d+);', S45, note='second stage of the two mean kernels'),
    _r('preconditioner', 'precond_summary_kernel', 'only', 1, 1024, '3V', _hip('precond_kernels.hip'), 'kPartialRows',
       r'constexpr int kPartialRows = (\d+);', S45, note='second stage of the field kernel'),
    _r('diagnostics', 'chain_moments_kernel<VEC>', 'vector', 4, 2048, 'C3V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', MOM, chains=2, note='both halves 16-byte aligned: C 3 V a multiple of 4'),
    _r('diagnostics', 'chain_moments_kernel<scalar>', 'scalar', 1, 2048, 'C3V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', S57, note='C 3 V odd: the slice of half 1 starts 12 bytes past a 16-byte boundary, so '
                                                          'its updates take the scalar form (half 0 the vector form and its tail)'),
    _r('diagnostics', 'split_rhat_kernel', 'only', 1, 2048, 'V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', DIAG, chains=2),
    _r('diagnostics', 'chain_variogram_kernel<VEC>', 'vector', 4, 2048, '3V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', DIAG, chains=2, note='E = 3 V elements, the chains inside the loop'),
    _r('diagnostics', 'chain_variogram_kernel<scalar>', 'scalar', 1, 2048, '3V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', S57),
    _r('diagnostics', 'split_ess_kernel', 'only', 1, 2048, 'V', _hip('diag_kernels.hip'), 'kDiagMaxBlocks',
       r'constexpr int kDiagMaxBlocks = (\d+);', DIAG, chains=2),
    _r('inverse_consistency', 'inverse_consistency_kernel', 'only', 1, 1024, 'V', HEADER, 'IRS_ICE_WS_BYTES',
       _WS.format('IRS_ICE_WS_BYTES'), S65, chains=2, note='1024 rows per chain'),
    _r('inverse_consistency', 'inverse_consistency_update_kernel', 'only', 1, 4096, 'V', _hip('inverse_kernels.hip'), 'stream_blocks',
       _STREAM.format('stream_blocks'), BIG, chains=2),
    _r('inverse_consistency', 'negate_kernel', 'only', 1, 4096, 'C3V', _hip('inverse_kernels.hip'), 'stream_blocks',
       _STREAM.format('stream_blocks'), S71),
    _r('inverse_consistency', 'inverse_consistency_finalize_kernel', 'only', 1, 1024, 'V', HEADER, 'IRS_ICE_MAP_WS_BYTES',
       _WS.format('IRS_ICE_MAP_WS_BYTES'), S65),
    _r('local_similarity', 'local_similarity_kernel<1>', 'only', 1, 1024, 'work', HEADER, 'IRS_LOCAL_MAX_BLOCKS',
       r'#define IRS_LOCAL_MAX_BLOCKS (\d+)', LOCAL, chains=2, per_block=1, rule='local', note='radius 1'),
    _r('local_similarity', 'local_similarity_update_kernel', 'only', 1, 4096, 'V', _hip('local_similarity_kernels.hip'),
       'local_stream_blocks', _STREAM.format('local_stream_blocks'), BIG, chains=2),
    _r('local_similarity', 'local_similarity_finalize_kernel', 'only', 1, 1024, 'V', HEADER, 'IRS_LOCAL_MAP_WS_BYTES',
       _WS.format('IRS_LOCAL_MAP_WS_BYTES'), S65),
    _r('residual_check', 'residual_histogram_kernel<scalar>', 'scalar', 1, 1024, 'V', HEADER, 'IRS_RESIDUAL_MAX_BLOCKS',
       r'#define IRS_RESIDUAL_MAX_BLOCKS (\d+)', S65, chains=2, note='1024 rows per chain'),
    _r('residual_check', 'residual_histogram_kernel<VEC>', 'vector', 4, 1024, 'V', HEADER, 'IRS_RESIDUAL_MAX_BLOCKS',
       r'#define IRS_RESIDUAL_MAX_BLOCKS (\d+)', BIG4, chains=2, note='1024 rows per chain'),
    _r('residual_check', 'residual_nll_update_kernel', 'only', 1, 4096, 'V', _hip('residual_kernels.hip'), 'residual_stream_blocks',
       _STREAM.format('residual_stream_blocks'), BIG, chains=2),
    _r('residual_check', 'residual_nll_finalize_kernel', 'only', 1, 1024, 'V', HEADER, 'IRS_RESIDUAL_MAP_WS_BYTES',
       _WS.format('IRS_RESIDUAL_MAP_WS_BYTES'), S65),
    _r('image_similarity', 'similarity_accumulate_kernel<scalar> C=8', 'scalar', 1, 1024 // 8, 'V', HEADER,
       'IRS_SIMILARITY_MAX_BLOCKS', r'#define IRS_SIMILARITY_MAX_BLOCKS (\d+)', (33, 33, 33), chains=8, note='cap / C per chain'),
    _r('image_similarity', 'similarity_accumulate_kernel<VEC> C=8', 'vector', 4, 1024 // 8, 'V', HEADER,
       'IRS_SIMILARITY_MAX_BLOCKS', r'#define IRS_SIMILARITY_MAX_BLOCKS (\d+)', (52, 51, 52), chains=8, note='cap / C per chain'),
    _r('image_similarity', 'similarity_accumulate_kernel<scalar> C=1', 'scalar', 1, 1024, 'V', HEADER,
       'IRS_SIMILARITY_MAX_BLOCKS', r'#define IRS_SIMILARITY_MAX_BLOCKS (\d+)', S65),
    _r('image_similarity', 'similarity_accumulate_kernel<VEC> C=1', 'vector', 4, 1024, 'V', HEADER,
       'IRS_SIMILARITY_MAX_BLOCKS', r'#define IRS_SIMILARITY_MAX_BLOCKS (\d+)', BIG4),
    _r('label_posterior', 'label_update_kernel<scalar>', 'scalar', 1, 1024, 'V', _hip('label_kernels.hip'), 'kLabelMaxBlocks',
       r'constexpr int kLabelMaxBlocks = (\d+);', S65, chains=2),
    _r('label_posterior', 'label_update_kernel<VEC>', 'vector', 8, 1024, 'V', _hip('label_kernels.hip'), 'kLabelMaxBlocks',
       r'constexpr int kLabelMaxBlocks = (\d+);', LABEL8, chains=2, note='units of 8 voxels: the cap is only passed above 2 097 152 voxels'),
    _r('label_posterior', 'label_finalize_kernel', 'only', 1, 1024, 'V', _hip('label_kernels.hip'), 'kLabelMaxBlocks',
       r'constexpr int kLabelMaxBlocks = (\d+);', S65),
    _r('surface_posterior', 'surface_finalize_kernel', 'only', 1, 512, 'rows', HEADER, 'IRS_SURFACE_MAX_BLOCKS',
       r'#define IRS_SURFACE_MAX_BLOCKS (\d+)', SURF, per_block=4, note='a wavefront per row, 4 rows per block'),
    _r('masks', 'intensity_histogram_kernel', 'only', 1, 1024, 'V', _hip('mask_kernels.hip'), 'launch_intensity_histogram (literal)',
       r'const int blocks = \(int\)std::min<int64_t>\(\(V \+ kBlock - 1\) / kBlock, (\d+)\);', S65, chains=2),
    _r('masks', 'cc_scan_kernel', 'only', 1024, 1024, 'chunks', _hip('mask_kernels.hip'), 'kScanBlock',
       r'constexpr int kScanBlock = (\d+);', BIG, chains=2, per_block=1, rule='scan', note='per >= 2 once V / 1024 > 1024'),
    _r('masks', 'select_largest_kernel', 'only', 1, 1, 'components', _hip('mask_kernels.hip'), 'kScanBlock',
       r'constexpr int kScanBlock = (\d+);', BIG, chains=2, per_block=1024, note='one block of 1024 threads sweeps the components'),
)


def key(rec):
    return f'{rec.family}/{rec.kernel}'


RECORD = {key(r): r for r in RECORDS}
assert len(RECORD) == len(RECORDS)
FAMILIES = tuple(dict.fromkeys(r.family for r in RECORDS))


def records_of(family):
    return [key(r) for r in RECORDS if r.family == family]


# ---------------------------------------------------------------- the launchers' rules, restated
def stream_blocks(units, cap, per_block=BLOCK):
    """min(ceil(units / per_block), cap), at least 1: every capped launcher's grid"""
    return int(max(1, min(-(-int(units) // per_block), cap)))


def local_similarity_geometry(D, H, W, radius, max_blocks=1024):
    """local_similarity_kernels.hip: tiles of 32 x 8 in x-y times z-segments no shorter than 8 radius -> dict"""
    tiles_x = (W + 31) // 32
    tiles = tiles_x * ((H + 7) // 8)
    want = (max_blocks + tiles - 1) // tiles
    nseg = max(1, min(want, (D + 8 * radius - 1) // (8 * radius)))
    seg_len = (D + nseg - 1) // nseg
    nwork = tiles * ((D + seg_len - 1) // seg_len)
    return {'tiles_x': tiles_x, 'tiles': tiles, 'seg_len': seg_len, 'nwork': nwork, 'blocks': min(nwork, max_blocks)}


def cc_blocks(V, chunk=1024):
    """mask_kernels.hip: the chunks of 1024 consecutive voxels whose roots cc_scan_kernel scans"""
    return (int(V) + chunk - 1) // chunk


def trip_of(index, unit, blocks, per_block=BLOCK):
    """(trip, block) of element `index` (an int or an array) of a grid-stride loop: `blocks` blocks, each taking `per_block`
    units of `unit` elements per trip"""
    u = np.asarray(index) // unit
    stride = blocks * per_block
    return u // stride, (u % stride) // per_block


Geometry = namedtuple('Geometry', 'elements units blocks per_block trips threshold')


def volume(shape):
    return int(np.prod(shape))


def elements_of(rec, components=None):
    V = volume(rec.shape)
    if rec.count == 'components':
        return int(components if components is not None else case('masks/components')['sizes'][0].size)
    return {'V': V, '3V': 3 * V, 'C3V': rec.chains * 3 * V, 'rows': rec.shape[0] * rec.shape[1],
            'work': local_similarity_geometry(*rec.shape, 1)['nwork'], 'chunks': V}[rec.count]


def geometry(rec, cap=None, components=None):
    """the launch of `rec` at its shape by the restated rule.  threshold: the most units one trip takes"""
    cap = rec.cap if cap is None else cap
    n = elements_of(rec, components)
    if rec.rule == 'local':
        g = local_similarity_geometry(*rec.shape, 1, cap)
        return Geometry(n, g['nwork'], g['blocks'], 1, -(-g['nwork'] // g['blocks']), cap)
    if rec.rule == 'scan':  # thread t of the one block owns chunks t per .. t per + per - 1
        chunks = cc_blocks(n)
        return Geometry(n, chunks, 1, cap, -(-chunks // cap), cap)
    units = -(-n // rec.unit) if rec.kernel.startswith('chain_moments') else n // rec.unit
    blocks = stream_blocks(units, cap, rec.per_block)
    return Geometry(n, units, blocks, rec.per_block, -(-units // (blocks * rec.per_block)), cap * rec.per_block)


def shape_problems(rec, cap=None, components=None):
    """what keeps rec.shape from being a shape past the cap, as a list of sentences (empty: nothing)"""
    g = geometry(rec, cap, components)
    out = []
    if g.trips < 2:
        out.append(f'{g.units} units stay within one trip of {g.threshold}')
    if rec.rule == 'local':
        if g.units % g.blocks == 0:
            out.append('the last trip is full')
        return out  # (exempt from the 1.5 x rule: the threshold comes from the segment rule)
    if rec.rule == 'scan':
        if g.units % g.trips == 0:
            out.append('the last thread owns a full share of chunks')
    elif g.units % g.per_block == 0 or g.units % g.threshold == 0:
        out.append(f'{g.units} units: the last trip is not ragged')
    if rec.form == 'scalar' and g.elements % 4 == 0:
        out.append(f'{g.elements} elements are a multiple of 4: the launcher takes the vector form')
    if rec.form == 'vector' and g.elements % rec.unit != 0:
        out.append(f'{g.elements} elements are no multiple of {rec.unit}: the launcher takes the scalar form')
    if rec.count != 'components' and 2 * g.units > 3 * g.threshold:
        out.append(f'{g.units} units are more than 1.5 x the threshold {g.threshold}')
    return out


def source_cap(rec, root=ROOT):
    """the cap as the source defines it: rec.pattern's one group in rec.source"""
    with open(os.path.join(root, rec.source)) as f:
        found = re.findall(rec.pattern, f.read(), flags=re.S)
    assert len(found) == 1, (key(rec), rec.constant, found)
    return int(found[0])


def restated_cap(rec):
    """the value source_cap must give: similarity's per-chain cap is the constant divided by the chains"""
    if rec.family == 'image_similarity':
        return rec.cap * rec.chains
    if rec.count == 'components':
        return rec.per_block
    return rec.cap


def trips_of(rec, components=None):
    """(trip, block) arrays over the elements of rec, and its geometry"""
    g = geometry(rec, components=components)
    idx = np.arange(g.elements)
    if rec.rule == 'local':
        raise ValueError('work items: see local_work')
    if rec.rule == 'scan':  # over the chunks: the position in the owning thread's share
        chunk = np.arange(g.units)
        return chunk % g.trips, np.zeros_like(chunk), g
    trip, block = trip_of(idx, rec.unit, g.blocks, g.per_block)
    return trip, block, g


def local_work(shape, radius=1):
    """per voxel of `shape` the work item that writes it -> (trip, block) volumes"""
    D, H, W = shape
    g = local_similarity_geometry(D, H, W, radius)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    work = (z // g['seg_len']) * g['tiles'] + (y // 8) * g['tiles_x'] + x // 32
    return trip_of(work, 1, g['blocks'], 1)


MUTANTS = ('as is', 'tail dropped', 'last trip twice', 'one round of the second stage')


def weights(trip, block):
    """the four evaluations of the host test as integer weights over the elements"""
    last = trip == trip.max()
    return {'as is': np.ones(trip.shape, np.int64), 'tail dropped': (trip == 0).astype(np.int64),
            'last trip twice': 1 + last.astype(np.int64), 'one round of the second stage': (block < BLOCK).astype(np.int64)}


def gather(weight):
    """the element indices with every element repeated `weight` times"""
    return np.repeat(np.arange(weight.size), weight.reshape(-1))


def density_mask(rng, trip, first=0.7, later=0.4):
    return rng.random(trip.shape) < np.where(trip == 0, first, later)


# ---------------------------------------------------------------- the cases
_CASES = {}


def _case(name):
    def register(fn):
        _CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return register


def case(name):
    """the inputs and the reference of one case, built once and left unchanged"""
    return _CASES[name]()


def case_names():
    return tuple(_CASES)


def _last(trip, k):
    """the k-th element of the last trip"""
    return int(np.flatnonzero(trip.reshape(-1) == trip.max())[k])


def _beyond(trip, block, k):
    """the k-th element of the first trip that lies in a row of partials past the first 256 (the last trip ends before them)"""
    return int(np.flatnonzero((trip.reshape(-1) == 0) & (block.reshape(-1) >= BLOCK))[k])


# ---- modes: the Gram matrix
@_case('modes/gram')
def _modes():
    from tests import _displacement_modes as R
    rec = RECORD['modes/modes_gram_partial_kernel']
    trip, block, g = trips_of(rec)
    V, n = g.elements, 5
    rng = np.random.default_rng(101)
    x = (rng.uniform(-1, 1, (1, 3, V)) + 0.3 * rng.standard_normal((n, 3, V))) * 0.05
    x = (x * (1 + 2 * trip) + 0.02 * trip).astype(f32)                   # the later trips: another mean and spread
    hi, lo, out = _last(trip, 5), _last(trip, 9), _last(trip, 3)
    x[0, 0, hi], x[1, 1, lo] = 0.75, -0.75                               # the extremes, in the last trip
    mask = density_mask(rng, trip)
    mask[hi] = mask[lo] = True
    mask[out] = False
    spoiled = x.copy()
    spoiled[2, 2, out] = np.nan                                          # what the mask leaves out may hold anything
    flat = x.reshape(n, 3, -1)

    def reference(weight, masked=True):
        idx = gather(weight * mask if masked else weight)
        return {'gram': R.gram_np(flat[:, :, idx])}

    ref, bound = R.gram_reference(x, mask)
    ref0, bound0 = R.gram_reference(x, None)
    return {'record': rec, 'trip': trip, 'block': block, 'records': x.reshape(n, 3, *rec.shape), 'spoiled': spoiled.reshape(n, 3, *rec.shape),
            'mask': mask.reshape(rec.shape), 'appends': (2, 3), 'reference': reference, 'tol': {'gram': bound},
            'gram': {True: (ref, bound), False: (ref0, bound0)}, 'any': (),
            'exempt': {('gram', MUTANTS[3]): 'the cap is 256 chunks and the finish kernel adds them in one serial loop: there is '
                                             'no row beyond a first round'}}


# ---- preconditioner: the two means, the field and its summary
PRECOND = dict(beta=0.9, count=5, damping=0.1, sigma_min=0.875, sigma_max=1.125)


def _precond(smooth):
    from tests import _preconditioner as S
    rec = RECORD['preconditioner/precond_field_kernel']
    trip, block, g = trips_of(rec)
    N = g.elements
    rng = np.random.default_rng(202)
    V = (np.exp(rng.uniform(-4.0, 4.0, N)) * (1 + 3 * trip)).astype(f32).reshape(1, 3, *rec.shape)
    V[0, 2, 40:45, 0:5, 0:5], V[0, 2, 40:45, 10:15, 0:5] = 1e6, 1e-8     # both clamps inside the last trip, box mean or not
    bias = S.bias_correction(PRECOND['beta'], PRECOND['count'])
    with np.errstate(all='ignore'):
        s = np.sqrt(S.corrected(V, bias, smooth))
        sbar = float(s.astype(np.float64).sum() / N)
        G = S._G(s, sbar, PRECOND['damping'])
        gbar = float(G.astype(np.float64).sum() / N)
        raw = np.sqrt(G / f32(gbar))
        sg = np.minimum(np.maximum(raw, f32(PRECOND['sigma_min'])), f32(PRECOND['sigma_max']))
    cols = {k: a.reshape(-1).astype(np.float64) for k, a in (('s', s), ('G', G), ('sg', sg))}
    low, high = (raw < f32(PRECOND['sigma_min'])).reshape(-1), (raw > f32(PRECOND['sigma_max'])).reshape(-1)

    def reference(weight):
        w = weight.astype(np.float64)
        on = weight > 0
        return {'s_mean': float((cols['s'] * w).sum() / N), 'G_mean': float((cols['G'] * w).sum() / N),
                'sigma2_mean': float((cols['sg'] ** 2 * w).sum() / N), 'clamped_low': int((low * weight).sum()),
                'clamped_high': int((high * weight).sum()), 'sigma_min': float(cols['sg'][on].min()),
                'sigma_max': float(cols['sg'][on].max())}

    rel = N * 2.0 ** -52  # the bound of tests/test_gpu_preconditioner.py:101-108
    tol = {'s_mean': rel * sbar, 'G_mean': rel * gbar, 'sigma2_mean': rel * float((cols['sg'] ** 2).sum() / N), 'clamped_low': 0,
           'clamped_high': 0, 'sigma_min': 0, 'sigma_max': 0}
    why = 'the clamp is reached in every trip, so the extremes of sigma are the two clamp values whatever is left out'
    exempt = {(c, m): why for c in ('sigma_min', 'sigma_max') for m in MUTANTS[1:]}
    return {'record': rec, 'trip': trip, 'block': block, 'V': V, 'smooth': smooth, 'reference': reference, 'tol': tol, 'exempt': exempt,
            'any': (), 'low': low, 'high': high}


_case('preconditioner/smooth0')(lambda: _precond(0))
_case('preconditioner/smooth1')(lambda: _precond(1))


# ---- chain diagnostics
DIAG_N, DIAG_LAG, DIAG_ESS_THRESHOLD, DIAG_RHAT_THRESHOLDS = 8, 3, 4.0, (1.01, 1.1)


def diag_samples(shape, seed, chains=1, rec=None):
    """(C, 8, 3, V) float32 AR(1) chains, every chain around its own level, whose later voxels have another level, spread and
    memory -- later by the trips of the R-hat kernel over the voxels or, with `rec` one of the two chain updates, by the trips of
    its loop over the flat (C, 3, V) sample, read at the last chain and channel; in the last trip a voxel whose halves sit 40
    apart (the largest R-hat), one that ramps within each half (the smallest ESS) and, outside the mask, one with an infinite
    sample -> (x, mask (V,), trip, block, the three voxels)"""
    V, Cn = volume(shape), chains
    if rec is None:
        trip, block = trip_of(np.arange(V), 1, stream_blocks(V, 2048))
    else:
        g = geometry(rec)
        trip, block = trip_of(g.elements - V + np.arange(V), rec.unit, g.blocks)
        assert trip.max() == g.trips - 1 and trip.min() == 0
    rng = np.random.default_rng(seed)
    phi = np.clip(rng.uniform(-0.5, 0.9, (3, V)) - 0.3 * trip, -0.6, 0.9)
    x = np.empty((Cn, DIAG_N, 3, V))
    x[:, 0] = rng.standard_normal((Cn, 3, V)) / np.sqrt(1 - phi ** 2)
    for i in range(1, DIAG_N):
        x[:, i] = phi * x[:, i - 1] + rng.standard_normal((Cn, 3, V))
    x = x * (1 + 2 * trip) + 0.5 * trip + 0.2 * np.arange(Cn).reshape(Cn, 1, 1, 1)
    a, b, c = _last(trip, 7), _last(trip, 11), _last(trip, 13)
    x[0, DIAG_N // 2:, :, a] += 40.0 * (1 + 2 * trip.max())
    x[0, :, :, b] = (np.tile(np.arange(DIAG_N // 2), 2)[:, None] + 0.01 * rng.standard_normal((DIAG_N, 3)))
    x = x.astype(f32)
    x[0, 2, 1, c] = np.inf
    mask = density_mask(rng, trip)
    mask[a] = mask[b] = True
    mask[c] = False
    return x, mask, trip, block, (a, b, c)


@_case('diagnostics/finalize')
def _diag():
    from tests._split_ess import split_ess_map_np
    from tests._split_rhat import split_rhat_map_np
    rec = RECORD['diagnostics/split_rhat_kernel']
    x, mask, trip, block, planted = diag_samples(rec.shape, 303, rec.chains)
    with np.errstate(all='ignore'):
        rhat = split_rhat_map_np(x)
        ess, mcse, truncated, margin = split_ess_map_np(x, DIAG_LAG)
    # a truncation decision within 1e-3 of flipping (tests/test_gpu_ess.py:116-118) is left out of the mask: the count of
    # truncated voxels in the summary is then an integer like the others, and the GPU test asks for equality
    mask = mask & (margin >= 1e-3)
    assert mask[planted[0]] and mask[planted[1]]
    r32, e32 = rhat.astype(f32), ess.astype(f32)

    def reference(weight):
        w = weight * mask
        on = w > 0
        return {'rhat/voxels': int(w.sum()), 'rhat/above_1.01': int((w * (r32 > f32(1.01))).sum()),
                'rhat/above_1.1': int((w * (r32 > f32(1.1))).sum()), 'rhat/max': float(rhat[on].max()),
                'rhat/sum': float((rhat[on] * w[on]).sum()), 'ess/voxels': int(w.sum()),
                'ess/below': int((w * (e32 < f32(DIAG_ESS_THRESHOLD))).sum()), 'ess/truncated': int((w * truncated).sum()),
                'ess/min': float(ess[on].min()), 'ess/sum': float((ess[on] * w[on]).sum())}

    full = reference(np.ones(x.shape[-1], np.int64))
    tol = {k: 0 for k in full}
    tol['rhat/sum'], tol['ess/sum'] = 1e-12 * full['rhat/sum'], 1e-12 * full['ess/sum']  # test_gpu_chain_diagnostics.py:126, test_gpu_ess.py:159
    twice = 'an extremum does not change when elements are counted twice'
    rows = 'the last trip ends in block %d: its extremum is inside the first 256 rows' % int(block[trip == trip.max()].max())
    exempt = {('rhat/max', MUTANTS[2]): twice, ('ess/min', MUTANTS[2]): twice, ('rhat/max', MUTANTS[3]): rows, ('ess/min', MUTANTS[3]): rows}
    return {'record': rec, 'trip': trip, 'block': block, 'x': x, 'mask': mask.reshape(rec.shape), 'planted': planted, 'rhat': rhat,
            'ess': ess, 'mcse': mcse, 'truncated': truncated, 'margin': margin, 'reference': reference, 'tol': tol, 'exempt': exempt,
            'any': ()}


# ---- inverse consistency
ICE_THRESHOLD = 1.5


@_case('inverse_consistency/main')
def _ice_main():
    import torch
    from tests import _exact_cases as X
    from tests import _inverse_consistency as R
    rec = RECORD['inverse_consistency/inverse_consistency_kernel']
    trip, block, g = trips_of(rec)
    C, dims, V = rec.chains, rec.shape, g.elements
    rng = np.random.default_rng(404)
    level = torch.from_numpy((1.0 + 2.0 * trip).reshape(1, 1, *dims)).float()
    v = R.smooth_field(C, dims, 6.0, 41)
    d_a = (v * level).contiguous()
    d_b = (-v * level + 0.25 * R.smooth_field(C, dims, 3.0, 42)).contiguous()   # not quite the inverse: a residual to measure
    hi, bad, out = _last(trip, 17), _last(trip, 23), _last(trip, 29)
    d_a.view(C, 3, V)[0, :, hi] += 30.0                                          # chain 0's largest norm, in the last trip
    d_a.view(C, 3, V)[1, :, _last(trip, 19)] -= 25.0                             # and chain 1's
    scale = torch.tensor([2.0 / (n - 1) for n in X.axis_sizes(dims)]).view(1, 3, 1, 1, 1)
    t_a = (X.identity(dims) + d_a * scale).contiguous()
    bad2 = _beyond(trip, block, 5)
    d_a.view(C, 3, V)[1, 0, [bad, bad2]] = float('nan')                          # inside the masks: counted as non-finite
    d_a.view(C, 3, V)[0, 2, out] = float('inf')                                  # outside them
    mask = np.stack([density_mask(rng, trip) for _ in range(C)])
    mask[:, [hi, bad, bad2, _last(trip, 19)]] = True
    mask[:, out] = False
    mask_t = torch.from_numpy(mask.reshape(C, 1, *dims))
    r64, n64 = R.compose(t_a, d_a, d_b, torch.float64)
    norm = n64.reshape(C, V)

    def reference(weight):
        idx = torch.from_numpy(gather(weight))
        out_ = {}
        for c in range(C):
            ints, floats = R.chain_summary(norm[c][idx], mask_t[c].reshape(-1)[idx])
            out_.update({f'{c}/voxels': ints[0], f'{c}/nonfinite': ints[1], f'{c}/sum': floats[0], f'{c}/sum2': floats[1],
                         f'{c}/max': floats[2]})
        return out_

    full = reference(np.ones(V, np.int64))
    tol = {k: 0 for k in full}
    for c in range(C):  # test_gpu_inverse_consistency.py:79-80
        tol[f'{c}/sum'], tol[f'{c}/sum2'] = V * 2.0 ** -53 * full[f'{c}/sum'], V * 2.0 ** -53 * full[f'{c}/sum2']
    exempt = {}
    for c in range(C):
        exempt[(f'{c}/max', MUTANTS[2])] = 'a maximum does not change when elements are counted twice'
        exempt[(f'{c}/max', MUTANTS[3])] = 'the last trip ends before block 256: its maximum is inside the first 256 rows'
        if c == 0:
            exempt.update({(f'{c}/nonfinite', m): 'chain 0 has no non-finite norm inside its mask' for m in MUTANTS[1:]})
    return {'record': rec, 'trip': trip, 'block': block, 't_a': t_a, 'd_a': d_a, 'd_b': d_b, 'mask': mask_t, 'r64': r64, 'n64': n64,
            'reference': reference, 'tol': tol, 'exempt': exempt, 'any': ()}


def _map_state(rec, seed, sign=1.0):
    """a synthetic per-voxel posterior state for a finalize kernel: mean, second map (peak / low), count, mask, and the planted
    voxels of the last trip: (extreme of the mean, extreme of the second map, empty inside the mask, outside the mask)"""
    trip, block, g = trips_of(rec)
    V = g.elements
    rng = np.random.default_rng(seed)
    mean = (rng.random(V) * (1 + trip) + 0.25 * trip).astype(f32)
    second = (mean + sign * rng.random(V).astype(f32) * (1 + trip)).astype(f32)
    count = rng.integers(1, 6, V).astype(np.int32)
    a, b, e, o = _last(trip, 31), _last(trip, 37), _last(trip, 41), _last(trip, 43)
    mean[a] = sign * 50.0
    second[b] = sign * 90.0
    e2 = _beyond(trip, block, 7)
    count[e] = count[e2] = count[_last(trip, 47)] = 0
    mask = density_mask(rng, trip)
    mask[[a, b, e, e2, _last(trip, 47)]] = True
    mask[o] = False
    return trip, block, V, mean, second, count, mask, (a, b, e, o, e2)


@_case('inverse_consistency/finalize')
def _ice_finalize():
    import torch
    from tests import _inverse_consistency as R
    rec = RECORD['inverse_consistency/inverse_consistency_finalize_kernel']
    trip, block, V, mean, peak, _, mask, (a, b, e, o, e2) = _map_state(rec, 505)
    mean[e] = mean[e2] = peak[_last(trip, 47)] = np.nan  # non-finite means and a peak that never saw a finite value
    mean[o] = np.inf
    mt, pt, kt = torch.from_numpy(mean), torch.from_numpy(peak), torch.from_numpy(mask)

    def reference(weight):
        idx = torch.from_numpy(gather(weight))
        ints, floats = R.map_summary(mt[idx], pt[idx], ICE_THRESHOLD, kt[idx])
        return {'voxels': ints[0], 'nonfinite': ints[1], 'above': ints[2], 'sum_mean': floats[0], 'max_mean': floats[1], 'max_peak': floats[2]}

    full = reference(np.ones(V, np.int64))
    tol = {k: 0 for k in full}
    tol['sum_mean'] = full['voxels'] * 2.0 ** -53 * full['sum_mean']  # test_gpu_inverse_consistency.py:199
    exempt = _extreme_exemptions(('max_mean', 'max_peak'))
    return {'record': rec, 'trip': trip, 'block': block, 'mean': mean.reshape(rec.shape), 'peak': peak.reshape(rec.shape),
            'mask': mask.reshape(rec.shape), 'reference': reference, 'tol': tol, 'exempt': exempt, 'any': ()}


def _extreme_exemptions(columns):
    out = {}
    for c in columns:
        out[(c, MUTANTS[2])] = 'an extremum does not change when elements are counted twice'
        out[(c, MUTANTS[3])] = 'the last trip ends before block 256: its extremum is inside the first 256 rows'
    return out


# ---- local similarity
@_case('local_similarity/main')
def _local_main():
    from ir_sgmcmc_amd.ops import local_similarity_constants
    from tests import _local_similarity as S
    rec = RECORD['local_similarity/local_similarity_kernel<1>']
    shape, C = rec.shape, rec.chains
    D, H, W = shape
    trip, block = local_work(shape, 1)
    assert int((trip == 1).sum()) == 33 and trip.max() == 1  # plane 1360, row 16: the two work items past the cap
    fixed, moving = S.noise_pair(shape, C, seed=606)
    rng = np.random.default_rng(607)
    # in the last two planes and rows the moving images are the fixed ones upside down: only the clamped windows of the last row
    # of the last plane -- the last trip -- lie wholly inside, and hold the smallest LNCC and SSIM of the volume
    moving[:, 0, D - 2:, H - 2:, 13:] = (1.0 - fixed[:, 0, D - 2:, H - 2:, 13:]).astype(f32)
    moving[1, 0, D - 1, H - 1, 3] = np.nan                         # spoils the windows of x = 2 .. 4 of the last trip
    mask = S.random_mask(shape, 608)
    mask[D - 1, H - 1, :] = True
    mask[D - 1, H - 1, 9] = False
    consts = local_similarity_constants(S.UNIT, S.UNIT)
    maps = [S.reference_maps(fixed[c, 0], moving[c, 0], 1, consts) for c in range(C)]
    flat = [{k: (v.reshape(-1) if isinstance(v, np.ndarray) else v) for k, v in m.items()} for m in maps]
    mflat = mask.reshape(-1)

    def reference(weight):
        idx = gather(weight)
        out = {}
        for c in range(C):
            sub = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in flat[c].items()}
            st = S.reference_stats(sub, mflat[idx])
            out.update({f'{c}/{k}': st[k] for k in S.COLUMNS})
        return out

    full = reference(np.ones(mflat.size, np.int64))
    tol = {k: (0 if k.split('/')[1] in ('n', 'n_flat', 'n_nonfinite') else 1e-9) for k in full}  # test_gpu_local_similarity.py:83-93
    exempt = {}
    for c in range(C):
        exempt.update(_extreme_exemptions((f'{c}/lncc_min', f'{c}/ssim_min')))
        exempt.update({(f'{c}/n_flat', m): 'no window of these inputs is flat' for m in MUTANTS[1:]})
        if c == 0:
            exempt.update({(f'{c}/n_nonfinite', m): 'chain 0 holds no non-finite value' for m in MUTANTS[1:]})
    return {'record': rec, 'trip': trip.reshape(-1), 'block': block.reshape(-1), 'fixed': fixed, 'moving': moving, 'mask': mask, 'maps': maps,
            'consts': consts, 'reference': reference, 'tol': tol, 'exempt': exempt, 'any': ()}


@_case('local_similarity/finalize')
def _local_finalize():
    rec = RECORD['local_similarity/local_similarity_finalize_kernel']
    trip, block, V, mean, low, count, mask, _ = _map_state(rec, 707, sign=-1.0)
    m64, l64 = mean.astype(np.float64), low.astype(np.float64)

    def reference(weight):
        w = weight * mask
        some = (w > 0) & (count > 0)
        return {'voxels': int(w.sum()), 'empty': int((w * (count == 0)).sum()), 'sum_mean': float((m64 * w)[some].sum()),
                'min_mean': float(m64[some].min()), 'min_low': float(l64[some].min())}

    full = reference(np.ones(V, np.int64))
    tol = {k: 0 for k in full}
    tol['sum_mean'] = 1e-12 * float(np.abs(m64[mask & (count > 0)]).sum())  # test_gpu_local_similarity.py:270
    return {'record': rec, 'trip': trip, 'block': block, 'mean': mean.reshape(rec.shape), 'low': low.reshape(rec.shape),
            'count': count.reshape(rec.shape), 'mask': mask.reshape(rec.shape), 'reference': reference, 'tol': tol,
            'exempt': _extreme_exemptions(('min_mean', 'min_low')), 'any': ()}


# ---- residual check
RES_STD, RES_PI, RES_HALF, RES_BINS, RES_MARGIN = (0.05, 0.2), (0.7, 0.3), 0.5, 128, 4.0


def residual_draw(rec, seed):
    """two recorded steps of residuals (C,1,V) and the shared mask (V,): the later trips wider and shifted; in the last trip of
    the first step the largest |z| (clipped), a NaN inside the mask and an inf outside it"""
    from tests import _residual_check as S
    trip, block, g = trips_of(rec)
    V, C = g.elements, rec.chains
    rng = np.random.default_rng(seed)
    steps = []
    for s in range(2):
        z = S.draw_mixture((V,), C, RES_STD, RES_PI, seed + s).reshape(C, V)
        z = (z * (1 + 2 * trip) + 0.1 * trip * (1 + np.arange(C)[:, None])).astype(f32)
        steps.append(z)
    hi, bad, out = _last(trip, 51), _last(trip, 53), _last(trip, 57)
    steps[0][:, hi] = -7.0 - np.arange(C)
    bad2 = _beyond(trip, block, 9)
    steps[0][:, [bad, bad2]] = np.nan
    steps[0][:, out] = np.inf
    mask = density_mask(rng, trip)
    mask[[hi, bad, bad2]] = True
    mask[out] = False
    return trip, block, steps, mask


def _residual_hist(rec_key, seed):
    from tests import _residual_check as S
    rec = RECORD[rec_key]
    trip, block, steps, mask = residual_draw(rec, seed)
    C, V = steps[0].shape

    def one(z, idx):
        return S.reference_histogram(z[:, idx].reshape(C, 1, 1, 1, -1), mask[idx].reshape(1, 1, 1, 1, -1), RES_HALF, RES_BINS)

    def reference(weight):
        idx = gather(weight)
        hist, counts, sums = S.accumulate(one(steps[0], idx), one(steps[1], idx))
        out = {}
        for c in range(C):
            out[f'{c}/hist'] = hist[c]
            out.update({f'{c}/{k}': int(counts[c, j]) for j, k in enumerate(S.COUNTS)})
            out.update({f'{c}/{k}': float(sums[c, j]) for j, k in enumerate(('sum_z', 'sum_z2', 'sum_z4', 'max_abs_z'))})
        return out

    tol = {}
    for c in range(C):
        d = np.concatenate([z[c][mask & np.isfinite(z[c])] for z in steps]).astype(np.float64)
        rel = RES_MARGIN * d.size * 2.0 ** -53  # test_gpu_residual_check.py:66-70
        tol.update({f'{c}/hist': 0, f'{c}/n': 0, f'{c}/n_nonfinite': 0, f'{c}/n_clipped': 0, f'{c}/max_abs_z': 0,
                    f'{c}/sum_z': rel * math.fsum(np.abs(d)), f'{c}/sum_z2': rel * math.fsum(d * d), f'{c}/sum_z4': rel * math.fsum((d * d) ** 2)})
    exempt = {}
    for c in range(C):
        exempt.update(_extreme_exemptions((f'{c}/max_abs_z',)))
    return {'record': rec, 'trip': trip, 'block': block, 'steps': steps, 'mask': mask, 'reference': reference, 'tol': tol, 'exempt': exempt,
            'any': tuple(f'{c}/hist' for c in range(C))}


_case('residual_check/histogram scalar')(lambda: _residual_hist('residual_check/residual_histogram_kernel<scalar>', 808))
_case('residual_check/histogram vector')(lambda: _residual_hist('residual_check/residual_histogram_kernel<VEC>', 818))


@_case('residual_check/finalize')
def _residual_finalize():
    from tests import _residual_check as S
    rec = RECORD['residual_check/residual_nll_finalize_kernel']
    trip, block, V, mean, _, count, mask, _ = _map_state(rec, 909)

    def reference(weight):
        idx = gather(weight)
        ints, floats = S.reference_nll_summary(mean[idx], count[idx], mask[idx])
        return {'voxels': ints[0], 'empty': ints[1], 'sum_mean': floats[0], 'max_mean': floats[1]}

    full = reference(np.ones(V, np.int64))
    tol = {k: 0 for k in full}
    tol['sum_mean'] = RES_MARGIN * full['voxels'] * 2.0 ** -53 * float(np.abs(mean).sum())  # test_gpu_residual_check.py:194
    return {'record': rec, 'trip': trip, 'block': block, 'mean': mean.reshape(rec.shape), 'count': count.reshape(rec.shape),
            'mask': mask.reshape(rec.shape), 'reference': reference, 'tol': tol, 'exempt': _extreme_exemptions(('max_mean',)), 'any': ()}


# ---- image similarity
SIM_BINS, SIM_UNIT = 32, (0.0, 1.0)


def _similarity(rec_key, seed):
    from tests import _image_similarity as S
    rec = RECORD[rec_key]
    trip, block, g = trips_of(rec)
    V, C = g.elements, rec.chains
    rng = np.random.default_rng(seed)
    fixed = rng.random((C, V), dtype=f32)
    noise = rng.random((C, V), dtype=f32)
    moving = np.where(trip == 0, f32(0.7) * fixed + f32(0.3) * noise, f32(0.2) * fixed + f32(1.1) * noise).astype(f32)  # later: looser, and clipped
    fixed = np.where(trip == 0, fixed, f32(0.5) * fixed + f32(0.6)).astype(f32)
    bad, out = _last(trip, 61), _last(trip, 67)
    also = [_beyond(trip, block, 11)] if g.blocks > BLOCK else []
    moving[:, [bad] + also] = np.nan
    fixed[:, out] = -np.inf
    mask = density_mask(rng, trip)
    mask[[bad] + also] = True
    if also:  # and a clipped value there
        fixed[:, _beyond(trip, block, 13)], mask[_beyond(trip, block, 13)] = 1.5, True
    mask[out] = False
    COL = {k: j for j, k in enumerate(S.COLUMNS)}

    def reference(weight):
        idx = gather(weight)
        shape5 = (C, 1, 1, 1, idx.size)
        hist, stats = S.reference(fixed[:, idx].reshape(shape5), moving[:, idx].reshape(shape5), mask[idx].reshape(1, 1, 1, 1, -1),
                                  SIM_BINS, SIM_UNIT, SIM_UNIT)
        out_ = {}
        for c in range(C):
            out_[f'{c}/hist'] = hist[c]
            out_.update({f'{c}/{k}': stats[c, COL[k]] for k in S.COLUMNS})
        return out_

    full = reference(np.ones(V, np.int64))
    tol = {}
    for k, v in full.items():  # test_gpu_image_similarity.py:59-69
        name = k.split('/')[1]
        tol[k] = 0 if name in ('hist', 'n', 'n_nonfinite', 'n_clipped') else 1e-9 * (v if name == 'mse' else 1.0)
    return {'record': rec, 'trip': trip, 'block': block, 'fixed': fixed, 'moving': moving, 'mask': mask, 'reference': reference, 'tol': tol,
            'exempt': {}, 'any': tuple(f'{c}/hist' for c in range(C))}


for _name in ('scalar> C=8', 'VEC> C=8', 'scalar> C=1', 'VEC> C=1'):
    _case(f'image_similarity/{_name}')(functools.partial(_similarity, f'image_similarity/similarity_accumulate_kernel<{_name}', 1000 + len(_CASES)))


# ---- label posterior
LABELS3 = (10, 16, 58)


def label_draw(rec, labels, steps, seed):
    """records (steps * C, V) int16 in record order, the fixed map (V,) and the mask (V,).  Every label lives in every trip, in
    other proportions after the first; two records of a voxel share a base map, so a voxel of the first trip sees at most two
    classes -- in the last trip some see four: the largest entropy"""
    trip, block, g = trips_of(rec)
    V, n = g.elements, steps * rec.chains
    rng = np.random.default_rng(seed)
    pool = np.array(list(labels) + [0, 777], np.int16)
    K = len(labels)
    p_first = np.array([0.5, 0.2, 0.05][:K] + [0.2, 0.05])
    p_later = np.array([0.05, 0.3, 0.4][:K] + [0.05, 0.2])
    p_first, p_later = p_first / p_first.sum(), p_later / p_later.sum()

    def draw():
        return np.where(trip == 0, rng.choice(pool, V, p=p_first), rng.choice(pool, V, p=p_later)).astype(np.int16)

    bases = [draw(), draw()]
    records = np.stack([bases[k % 2] for k in range(n)])  # the chains of a step differ
    fixed = np.where(rng.random(V) < 0.7, bases[0], draw()).astype(np.int16)
    if n >= 4:
        for j in range(60, 90):  # four classes at one voxel
            records[:4, _last(trip, j)] = pool[:4] if K >= 3 else pool[[0, 1, K, K + 1]]
    mask = density_mask(rng, trip)
    mask[[_last(trip, j) for j in range(60, 75)]] = True
    mask[[_last(trip, j) for j in range(75, 90)]] = False
    return trip, block, records, fixed, mask


def _label_columns(ref):
    out = {}
    for j in range(ref['summary'].shape[0]):
        out.update({f'{j}/S{k}': int(ref['summary'][j, k]) for k in range(6)})
        out[f'{j}/bins'] = ref['summary'][j, 6:]
        out[f'{j}/vol_mean'], out[f'{j}/vol_m2'] = float(ref['vol_mean'][j]), float(ref['vol_m2'][j])
    out.update({'voxels': ref['entropy_voxels'], 'entropy_sum': ref['entropy_sum'], 'entropy_max': ref['entropy_max']})
    return out


@_case('label_posterior/scalar')
def _label():
    from tests._label_posterior import label_posterior_np
    rec = RECORD['label_posterior/label_update_kernel<scalar>']
    trip, block, records, fixed, mask = label_draw(rec, LABELS3, 2, 1111)
    n, V = records.shape

    def reference(weight):
        idx = gather(weight)
        return _label_columns(label_posterior_np(records[:, idx].reshape(n, 1, 1, -1), fixed[idx].reshape(1, 1, -1), list(LABELS3),
                                                 mask[idx].reshape(1, 1, -1)))

    full = reference(np.ones(V, np.int64))
    tol = {}
    for k, v in full.items():  # tests/test_gpu_label_posterior.py:41-58
        name = k.split('/')[-1]
        tol[k] = (1e-12 * abs(v) if name in ('vol_mean', 'vol_m2') else 1e-6 * full['voxels'] if name == 'entropy_sum' else
                  1e-6 if name == 'entropy_max' else 0)
    exempt = _extreme_exemptions(('entropy_max',))
    return {'record': rec, 'trip': trip, 'block': block, 'records': records, 'fixed': fixed, 'mask': mask, 'labels': LABELS3,
            'reference': reference, 'tol': tol, 'exempt': exempt, 'any': tuple(f'{j}/bins' for j in range(len(LABELS3)))}


@_case('label_posterior/vector')
def _label_vec():
    rec = RECORD['label_posterior/label_update_kernel<VEC>']
    labels = LABELS3[:2]
    trip, block, records, fixed, mask = label_draw(rec, labels, 2, 1212)
    n, V = records.shape
    hit = [(records == lab) for lab in labels]

    def reference(weight):
        out = {}
        for j, h in enumerate(hit):  # the Welford fold of tests/_label_posterior.py:41-46 over the per-record volumes
            mean = m2 = 0.0
            for k in range(1, n + 1):
                x = float((h[k - 1] * weight).sum())
                d = x - mean
                mean += d / k
                m2 += d * (x - mean)
            out[f'{j}/vol_mean'], out[f'{j}/vol_m2'] = mean, m2
        return out

    full = reference(np.ones(V, np.int64))
    return {'record': rec, 'trip': trip, 'block': block, 'records': records, 'labels': labels, 'reference': reference,
            'tol': {k: 1e-12 * abs(v) for k, v in full.items()}, 'exempt': {}, 'any': ()}


# ---- surface posterior: the finalize
SURF_LEVELS = (0.5, 0.9)


@_case('surface_posterior/finalize')
def _surface():
    from tests import _hausdorff as HD
    from tests import _surface_posterior as S
    rec = RECORD['surface_posterior/surface_finalize_kernel']
    shape = rec.shape
    D, H, W = shape
    rows = D * H
    g = geometry(rec)
    rtrip, rblock = trip_of(np.arange(rows), 1, g.blocks, g.per_block)
    trip, block = np.repeat(rtrip, W), np.repeat(rblock, W)
    rng = np.random.default_rng(1313)
    seg = HD.random_seg(rng, shape, list(S.LABELS3))
    seg[D - 3:, H - 16:H - 4, 2:7] = S.LABELS3[2]           # contours in the last trip (rows 2048 .. 2114: z = 45 from y = 23, z = 46)
    seg[D - 2:, 2:12, 1:6] = S.LABELS3[1]
    seg[D - 1, H - 3:, :4] = S.LABELS3[0]
    V = volume(shape)
    count = rng.integers(0, 6, V).astype(np.int32)
    mean = (rng.standard_normal(V) * (1 + 2 * trip) + 0.5 * trip).astype(f32)
    m2 = (rng.random(V) * count * (1 + 3 * trip)).astype(f32)
    mask = density_mask(rng, trip)
    li = S.fixed_contours(seg, list(S.LABELS3)).reshape(-1)
    last_on = [np.flatnonzero((trip == trip.max()) & (li == j)) for j in range(3)]
    assert all(len(x) >= 8 for x in last_on), [len(x) for x in last_on]
    for j, on in enumerate(last_on):                         # per label, in the last trip: the largest |bias| and std, an empty voxel
        mean[on[0]], count[on[0]] = -60.0 - j, 3
        m2[on[1]], count[on[1]] = 5e4 + j, 2
        count[on[2]] = 0
        mask[on[:3]] = True
        mask[on[3]] = False
    bias, std = S.maps(mean.reshape(shape), m2.reshape(shape), count.reshape(shape))
    count3, mask3 = count.reshape(shape), mask.reshape(shape)

    def columns(sel):
        isum, fsum = S.summary(bias, std, count3, seg, list(S.LABELS3), SURF_LEVELS, mask3 & sel.reshape(shape))
        return isum, fsum

    def reference(weight):
        isum, fsum = columns(weight > 0)
        if weight.max() > 1:  # the sums are additive, the two maxima are not touched by a second count
            i2, f2 = columns(weight > 1)
            isum = isum + i2
            fsum[:, (0, 1, 2, 4)] += f2[:, (0, 1, 2, 4)]
        out = {}
        for j in range(3):
            out.update({f'{j}/i{k}': int(isum[j, k]) for k in range(isum.shape[1])})
            out.update({f'{j}/f{k}': float(fsum[j, k]) for k in range(6)})
        return out

    full = reference(np.ones(V, np.int64))
    tol = {k: 0 for k in full}
    for j in range(3):  # float64 sums in another order: 1e-12 of the sum of magnitudes (tests/_surface_posterior.py:25, 174-175)
        sel = (li == j) & mask
        one, two = sel & (count >= 1), sel & (count >= 2)
        b, sd = np.abs(bias.reshape(-1)[one].astype(np.float64)), std.reshape(-1)[two].astype(np.float64)
        tol[f'{j}/f0'] = tol[f'{j}/f1'] = 1e-12 * b.sum()
        tol[f'{j}/f2'], tol[f'{j}/f4'] = 1e-12 * (b * b).sum(), 1e-12 * sd.sum()
    exempt = {}
    for j in range(3):
        exempt.update(_extreme_exemptions((f'{j}/f3', f'{j}/f5')))
    return {'record': rec, 'trip': trip, 'block': block, 'seg': seg, 'mean': mean.reshape(shape), 'm2': m2.reshape(shape), 'count': count3,
            'mask': mask3, 'bias': bias, 'std': std, 'reference': reference, 'tol': tol, 'exempt': exempt, 'any': ()}


# ---- masks
MASK_BINS, MASK_RANGE = 256, (-3.0, 3.0)


@_case('masks/histogram')
def _mask_histogram():
    from tests import _masks as S
    rec = RECORD['masks/intensity_histogram_kernel']
    trip, block, g = trips_of(rec)
    V, C = g.elements, rec.chains
    rng = np.random.default_rng(1414)
    im = (rng.standard_normal((C, V)) * (1 + 0.5 * trip) + 0.75 * trip * (1 + np.arange(C)[:, None])).astype(f32)
    hi, lo, bad, out = _last(trip, 71), _last(trip, 73), _last(trip, 79), _last(trip, 83)
    im[:, hi], im[:, lo], im[:, bad], im[:, out] = 9.0, -9.0, np.nan, 2.5
    mask = np.stack([density_mask(rng, trip) for _ in range(C)])
    mask[:, [hi, lo, bad]] = True
    mask[:, out] = False

    def reference(weight):
        idx = gather(weight)
        return {f'{c}/hist': S.intensity_histogram(im[c][idx], MASK_BINS, MASK_RANGE, mask[c][idx]) for c in range(C)}

    return {'record': rec, 'trip': trip, 'block': block, 'im': im, 'mask': mask, 'reference': reference,
            'tol': {f'{c}/hist': 0 for c in range(C)}, 'exempt': {}, 'any': tuple(f'{c}/hist' for c in range(C))}


def sparse_components(shape):
    """a sparse mask of line segments along x on a lattice of every third plane and row, every other slot taken: more than 1024
    components of 1 .. 48 voxels spread over the whole volume (1025 distinct sizes would take half a million voxels, too many
    for a breadth-first reference: the sizes repeat, but for the three that are kept), three of 60, 59 and 58 voxels that start
    late in linear order, and one in the last voxels of the volume"""
    D, H, W = shape
    m = np.zeros(shape, bool)
    taken = [(z, y, x0) for z in range(0, D - 1, 3) for y in range(0, H - 1, 3) for x0 in range(0, W - 48, 52)
             if (z // 3 + y // 3 + x0 // 52) % 2 == 0]
    for i, (z, y, x0) in enumerate(taken):
        m[z, y, x0:x0 + 1 + (i * 7) % 48] = True
    for k, i in enumerate((len(taken) - 5, len(taken) - 40, len(taken) - 90)):  # the three largest: late, and not in size order
        z, y, _ = taken[i]
        m[z, y, :] = False
        m[z, y, 20:20 + 60 - k] = True
    m[D - 1, H - 1, W - 3:] = True
    return m


@_case('masks/components')
def _components():
    from tests import _masks as S
    rec = RECORD['masks/cc_scan_kernel']
    shape = rec.shape
    first = sparse_components(shape)
    volumes = np.stack([first, np.ascontiguousarray(first[::-1, :, ::-1])])
    labels, sizes, roots = [], [], []
    chunks = cc_blocks(volume(shape))
    for v in volumes:
        lab, n = S.connected_components(v, 26)
        labels.append(lab)
        flat = lab.reshape(-1)
        sizes.append(np.bincount(flat, minlength=n + 1)[1:])
        where = np.flatnonzero(flat)
        _, at = np.unique(flat[where], return_index=True)
        roots.append(np.bincount(where[at] // 1024, minlength=chunks))
    trip, block, g = trips_of(rec)
    C = len(volumes)

    def reference(weight):  # over the chunks: the roots the scan adds up
        return {f'{c}/components': int((roots[c] * weight).sum()) for c in range(C)}

    exempt = {(f'{c}/components', MUTANTS[3]): 'one block of 1024 threads: its thread 0 adds the 1024 shares in a serial loop' for c in range(C)}
    return {'record': rec, 'trip': trip, 'block': block, 'volumes': volumes, 'labels': labels, 'sizes': sizes, 'roots': roots,
            'reference': reference, 'tol': {f'{c}/components': 0 for c in range(C)}, 'exempt': exempt, 'any': ()}


def kept_components(sizes, keep):
    """tests/_masks.py:54: the `keep` largest, ties to the smaller number -> component numbers (1-based)"""
    return [i + 1 for i in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))[:keep]]


@_case('masks/select')
def _select():
    comp = case('masks/components')
    rec = RECORD['masks/select_largest_kernel']
    sizes = comp['sizes']
    C = len(sizes)
    n = min(s.size for s in sizes)
    trip, block = trip_of(np.arange(n), 1, 1, 1024)

    def reference(weight):
        out = {}
        for c in range(C):
            s = np.sort(sizes[c][:n][weight > 0])[::-1]
            out[f'{c}/largest'], out[f'{c}/third'] = int(s[0]), int(s[2])
        return out

    exempt = {}
    for c in range(C):
        for col in ('largest', 'third'):
            exempt[(f'{c}/{col}', MUTANTS[2])] = 'the sweep picks maxima: counting a component twice changes nothing'
            exempt[(f'{c}/{col}', MUTANTS[3])] = 'one block: the 1024 candidates meet in a tree in LDS, there are no rows of partials'
        exempt.update({(f'1/{col}', MUTANTS[1]): 'in the reversed volume the three largest components come first' for col in ('largest', 'third')})
    return {'record': rec, 'trip': trip, 'block': block, 'n': n, 'reference': reference,
            'tol': {f'{c}/{k}': 0 for c in range(C) for k in ('largest', 'third')},
            'exempt': exempt, 'any': ()}


# the records a case proves its inputs for (a case may serve several launches of one geometry)
CASE_RECORDS = {
    'modes/gram': ['modes/modes_gram_partial_kernel'],
    'preconditioner/smooth0': records_of('preconditioner'),
    'preconditioner/smooth1': records_of('preconditioner'),
    'diagnostics/finalize': ['diagnostics/split_rhat_kernel', 'diagnostics/split_ess_kernel'],
    'inverse_consistency/main': ['inverse_consistency/inverse_consistency_kernel'],
    'inverse_consistency/finalize': ['inverse_consistency/inverse_consistency_finalize_kernel'],
    'local_similarity/main': ['local_similarity/local_similarity_kernel<1>'],
    'local_similarity/finalize': ['local_similarity/local_similarity_finalize_kernel'],
    'residual_check/histogram scalar': ['residual_check/residual_histogram_kernel<scalar>'],
    'residual_check/histogram vector': ['residual_check/residual_histogram_kernel<VEC>'],
    'residual_check/finalize': ['residual_check/residual_nll_finalize_kernel'],
    'image_similarity/scalar> C=8': ['image_similarity/similarity_accumulate_kernel<scalar> C=8'],
    'image_similarity/VEC> C=8': ['image_similarity/similarity_accumulate_kernel<VEC> C=8'],
    'image_similarity/scalar> C=1': ['image_similarity/similarity_accumulate_kernel<scalar> C=1'],
    'image_similarity/VEC> C=1': ['image_similarity/similarity_accumulate_kernel<VEC> C=1'],
    'label_posterior/scalar': ['label_posterior/label_update_kernel<scalar>', 'label_posterior/label_finalize_kernel'],
    'label_posterior/vector': ['label_posterior/label_update_kernel<VEC>'],
    'surface_posterior/finalize': ['surface_posterior/surface_finalize_kernel'],
    'masks/histogram': ['masks/intensity_histogram_kernel'],
    'masks/components': ['masks/cc_scan_kernel'],
    'masks/select': ['masks/select_largest_kernel'],
}
# launches that write per-voxel outputs only: nothing is summed, so the four evaluations have no column to tell apart; a voxel
# that was not visited, or visited twice, shows in the element-by-element comparison of the GPU test
PER_VOXEL_ONLY = ('diagnostics/chain_moments_kernel<VEC>', 'diagnostics/chain_moments_kernel<scalar>', 'diagnostics/chain_variogram_kernel<VEC>',
                  'diagnostics/chain_variogram_kernel<scalar>', 'inverse_consistency/inverse_consistency_update_kernel',
                  'inverse_consistency/negate_kernel', 'local_similarity/local_similarity_update_kernel',
                  'residual_check/residual_nll_update_kernel')
