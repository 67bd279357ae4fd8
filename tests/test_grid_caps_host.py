"""The table of capped launches (tests/_grid_caps.py) against the source, its shapes against the launchers' rules, and the inputs
of tests/test_gpu_grid_caps.py against the mistakes they are meant to catch.  CPU only.

1. Every record's cap is read from the source by the regular expression on its constant's name and equals the restated value:
   when a cap changes, this fails instead of the GPU test falling back to one trip without a word.
2. Every chosen shape crosses its cap, ends in a ragged last trip, takes the scalar or the vector form as meant and is no
   larger than 1.5 x the threshold (the work-item loop of the local similarity aside), by the restated launcher rule.
3. Where the library answers for a block count -- the workspace queries of split R-hat, split ESS and the modes Gram rows -- the
   restated rule gives the same number.
4. Every family's float64 reference is evaluated on the chosen input as is, with everything after the first trip dropped, with
   the last trip counted twice and with only the first 256 rows of partials folded.  Every summary column, and of a histogram
   at least one bin, differs from the true value by at least 1000 times the tolerance the GPU test holds it to.  A column that
   cannot differ says why (`exempt` of the case): a maximum under a second count is the usual one.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _grid_caps as G

KEYS = [G.key(r) for r in G.RECORDS]


@pytest.mark.parametrize('name', KEYS)
def test_the_cap_in_the_source_is_the_restated_one(name):
    rec = G.RECORD[name]
    assert G.source_cap(rec) == G.restated_cap(rec), (name, rec.source, rec.constant)


def test_the_block_size_and_the_chunk_of_the_component_scan():
    import os
    import re
    text = open(os.path.join(G.ROOT, G.CSRC, 'common.h')).read()
    assert [int(x) for x in re.findall(r'constexpr int kBlock = (\d+);', text)] == [G.BLOCK]
    text = open(os.path.join(G.ROOT, G.CSRC, 'mask_kernels.hip')).read()
    assert [int(x) * G.BLOCK for x in re.findall(r'constexpr int kChunk = (\d+) \* kBlock;', text)] == [1024]
    text = open(os.path.join(G.ROOT, G.CSRC, 'surface_kernels.hip')).read()
    assert 'kBlock / kWave - 1) / (kBlock / kWave), IRS_SURFACE_MAX_BLOCKS)' in text  # 4 rows per block


def test_a_wrong_cap_is_noticed():
    """a record whose restated cap is wrong fails the comparison with the source, and a cap that has grown in the source (the
    restated rule fed the new value) turns the chosen shape into a one-trip shape, which the shape check reports"""
    for name in ('preconditioner/precond_field_kernel', 'image_similarity/similarity_accumulate_kernel<scalar> C=8',
                 'inverse_consistency/inverse_consistency_update_kernel', 'residual_check/residual_nll_finalize_kernel'):
        rec = G.RECORD[name]
        assert G.source_cap(rec) == G.restated_cap(rec)
        for wrong in (rec._replace(cap=rec.cap * 2), rec._replace(cap=rec.cap // 2)):
            assert G.source_cap(wrong) != G.restated_cap(wrong), name
    rec = G.RECORD['preconditioner/precond_field_kernel']
    assert G.shape_problems(rec) == [] and G.shape_problems(rec._replace(cap=rec.cap * 2)) != []


@pytest.mark.parametrize('name', KEYS)
def test_the_chosen_shape_is_past_the_cap_and_ragged(name):
    rec = G.RECORD[name]
    g = G.geometry(rec)
    print(name, rec.shape, 'chains', rec.chains, g)
    assert G.shape_problems(rec) == []
    assert g.trips == 2  # the smallest shapes past the cap: one wrap


def test_every_family_of_the_issue_is_in_the_table():
    assert G.FAMILIES == ('modes', 'preconditioner', 'diagnostics', 'inverse_consistency', 'local_similarity', 'residual_check',
                          'image_similarity', 'label_posterior', 'surface_posterior', 'masks')
    covered = {k for keys in G.CASE_RECORDS.values() for k in keys} | set(G.PER_VOXEL_ONLY)
    assert covered == set(KEYS)


def test_trip_of():
    assert [tuple(int(x) for x in G.trip_of(i, 1, 4)) for i in (0, 255, 256, 1023, 1024, 1280, 2047, 2048)] == \
        [(0, 0), (0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (1, 3), (2, 0)]
    assert tuple(int(x) for x in G.trip_of(8 * 1024 * 256 + 7, 8, 1024)) == (1, 0)   # units of eight
    assert tuple(int(x) for x in G.trip_of(2048 + 5, 1, 512, 4)) == (1, 1)           # rows, four to a block
    trip, block = G.trip_of(np.arange(3000), 1, 2)
    assert np.array_equal(trip, np.arange(3000) // 512) and np.array_equal(block, np.arange(3000) % 512 // 256)


def test_the_library_counts_the_same_blocks():
    """the workspace queries are plain host functions: 5 doubles per block for split R-hat and split ESS, n_new x 3 x 1024 doubles
    per chunk for the Gram rows"""
    from ir_sgmcmc_amd import _lib as L
    lib = L.load()
    nbytes = C.c_size_t()
    for name, query in (('diagnostics/split_rhat_kernel', lib.irs_split_rhat_workspace),
                        ('diagnostics/split_ess_kernel', lib.irs_split_ess_workspace)):
        rec = G.RECORD[name]
        L.check(query(1, *rec.shape, C.byref(nbytes)))
        assert nbytes.value == 5 * 8 * G.geometry(rec).blocks == 5 * 8 * rec.cap
        L.check(query(1, 9, 17, 33, C.byref(nbytes)))
        assert nbytes.value == 5 * 8 * G.stream_blocks(9 * 17 * 33, rec.cap)
    rec = G.RECORD['modes/modes_gram_partial_kernel']
    L.check(lib.irs_modes_gram_workspace(*rec.shape, 3, C.byref(nbytes)))
    assert nbytes.value == G.geometry(rec).blocks * 3 * 3 * L.IRS_MODES_MAX_RECORDS * 8 and G.geometry(rec).blocks == rec.cap


def differs(true, other, tol):
    """whether `other` is at least 1000 tol away from `true` -> per entry.  tol = 0 (integers, histograms, extrema: the GPU test
    asks for equality): away at all"""
    true, other, tol = np.asarray(true, np.float64), np.asarray(other, np.float64), np.asarray(tol, np.float64)
    return (np.abs(other - true) >= 1000.0 * tol) & (other != true)


@pytest.mark.parametrize('name', list(G.CASE_RECORDS))
def test_the_inputs_tell_the_mistakes_apart(name):
    case = G.case(name)
    w = G.weights(case['trip'], case['block'])
    true = case['reference'](w[G.MUTANTS[0]])
    assert set(true) == set(case['tol']), set(true) ^ set(case['tol'])
    worst = {}
    for mutant in G.MUTANTS[1:]:
        if mutant == G.MUTANTS[3] and (case['block'] < G.BLOCK).all():
            continue  # at most 256 rows of partials (the cap of the modes, similarity's 1024 / 8): one round folds them all
        got = case['reference'](w[mutant])
        for col, value in true.items():
            reason = case['exempt'].get((col, mutant))
            if reason is not None:
                assert len(reason) > 20
                continue
            d = differs(value, got[col], case['tol'][col])
            ok = d.any() if col in case['any'] else d.all()
            worst[(col, mutant)] = (value, got[col]) if np.ndim(value) == 0 else int(d.sum())
            assert ok, (name, col, mutant, value, got[col], case['tol'][col])
    print(name, {k: v for k, v in list(worst.items())[:12]})


def test_the_preconditioner_clips_on_both_sides_in_the_last_trip():
    for name in ('preconditioner/smooth0', 'preconditioner/smooth1'):
        case = G.case(name)
        last = case['trip'] == case['trip'].max()
        assert case['low'][last].sum() > 0 and case['high'][last].sum() > 0 and case['low'][~last].sum() > 0 and case['high'][~last].sum() > 0


def test_the_component_mask_is_what_the_issue_asks_for():
    comp = G.case('masks/components')
    for c, (v, sizes, roots) in enumerate(zip(comp['volumes'], comp['sizes'], comp['roots'])):
        assert sizes.size > 1024 and 10_000 < int(v.sum()) < 100_000 and int(v.sum()) == int(sizes.sum())
        assert roots[-1] > 0 or c == 1 and v.reshape(-1)[-1024:].any()   # the last 1024-voxel chunk holds a component
        assert all(part.any() for part in np.array_split(roots, 32))       # spread over the whole volume
        top = np.sort(sizes)[::-1][:4]
        assert top.tolist()[:3] == [60, 59, 58] and top[3] < 58           # keep = 1 and keep = 3 have one answer
    assert min(G.kept_components(comp['sizes'][0], 3)) > 1024              # the sweep finds them in its second trip
