"""Host side of tests/test_gpu_sparse_configs.py: what each case asserts about its lists holds for the mask's geometry.  Every list a case
calls strictly sparse marches, at its reach, at least one plane and fewer than D x tile columns -- for every transition's mask and
every chain -- so the GPU test's "fewer planes than the dense launch" is a statement the case can meet, and its equality is about
memory that really is left unwritten.  The forward lists are taken at width 1 per step, the narrowest plan; the GPU test asserts that
width wherever it relies on the first list."""
import pytest

from tests import _sparse_configs as SC
from tests.test_gpu_sparse_data import BIG, planes_of, run_lengths


@pytest.mark.parametrize('c', SC.CASES, ids=[c['id'] for c in SC.CASES])
def test_strict_lists_are_strictly_sparse(c):
    S, n, tot = SC.half_width(c), SC.steps(c), SC.totals(c['dims'])
    assert set(c['strict']) <= {'warp', 'map', 'data_term', 'fwd_first', 'fwd_last', 'adj_last'} and 'warp' in c['strict']
    if c['cfg'].get('cps'):                     # dense forward steps under SVFFD
        assert not {'fwd_first', 'fwd_last'} & set(c['strict'])
    if c['cfg'].get('data_loss') == 'SSD':      # no LCC lists behind the SSD term
        assert not {'map', 'data_term'} & set(c['strict'])
    if c['C'] > 1 and dict(c['options']).get('data_batch', 1) == 0:     # the per-chain data term keeps its full columns
        assert 'data_term' not in c['strict']
    seen = set()
    for entry in c['masks']:
        if entry in seen:
            continue
        seen.add(entry)
        m = SC.mask_of(entry, c['dims'])
        assert m.shape[0] in (1, c['C'])
        for ch in range(m.shape[0]):
            exp = SC.expected(m[ch, 0], S, n)
            figures = SC.strict_figures(exp, tot, n)
            print(c['id'], entry, 'chain', ch, figures)
            for name in c['strict']:
                planes, whole = figures[name]
                assert 0 < planes < whole, (name, planes, whole)
            # the reach shrinks towards the warp, and grows from the adjoint's first launched step to its last
            assert all(a >= b for a, b in zip(exp['forward'][:-1], exp['forward'][1:])) and exp['forward'][n - 1] == exp['warp']
            assert all(a >= b for a, b in zip(exp['adjoint'][:-1], exp['adjoint'][1:]))
            assert exp['map'] <= exp['data_term']


def test_every_case_has_five_transitions_and_the_file_stays_small():
    assert len(SC.CASES) <= 25 and len({c['id'] for c in SC.CASES}) == len(SC.CASES)
    assert all(len(c['masks']) == SC.T == 5 for c in SC.CASES)
    assert all(c['dims'][0] * c['dims'][1] * c['dims'][2] <= 70000 for c in SC.CASES)


def test_centred_ball_at_half_width_two():
    """the centred ball on (72, 24, 40) at S = 2, twelve steps of width 1"""
    m = SC.mask_of('ball', BIG)[0, 0]
    exp, tot = SC.expected(m, 2, 12), SC.totals(BIG)
    assert (exp['map'], exp['data_term'], tot['lcc']) == (40, 48, 288)
    assert (exp['warp'], tot['warp']) == (84, 216)
    # forward list k reaches 3 S + h_{k+1} + ... + h_{n-1}: 17 voxels for the first, 6 -- the warp's hull -- for the last
    assert (exp['forward'][0], exp['forward'][11]) == (150, 84)
    # (one width further, 3 S + 12 and 3 S + 1, the same columns give 156 and 90: still strictly sparse)
    assert planes_of(run_lengths(m, SC.WARP_TILE, 18)) == 156 and planes_of(run_lengths(m, SC.WARP_TILE, 7)) == 90
    # a column of the ball is cut at least three times by pieces of 8 planes
    assert max(b - a for a, b in run_lengths(m, SC.LCC_TILE, 4)) > 16
