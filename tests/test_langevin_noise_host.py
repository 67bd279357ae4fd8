"""The restatement of the in-kernel Langevin noise (tests/_langevin_noise.py), host side: Random123's known answers for Philox4x32-10,
split21 as a bijection of 126 bits, the counter layout, the statistics of the restated normals (the GPU's follow from the
per-element match of tests/test_gpu_langevin_noise.py), and the tolerance: a correctly rounded float32 evaluation stays below a
quarter of it, every mistake it is for exceeds it at 99 % or more of the elements the mistake touches."""
import math

import numpy as np
import pytest
import torch

from tests import _langevin_noise as N

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, result)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ---------------------------------------------------------------- 1. known answers
def test_philox4x32_10_known_answers_scalar():
    for ctr, key, want in KAT:
        got = N.philox4x32_10(*ctr, *key)
        assert tuple(int(t) for t in got) == want, [hex(int(t)) for t in got]


def test_philox4x32_10_known_answers_vectorised():
    """all three in one call, among other lanes, in a 2-D array: no lane leaks into another"""
    lanes = [KAT[i % 3] for i in range(12)]
    args = [np.array([[ln[0][j] for ln in lanes]] * 2, dtype=np.uint64) for j in range(4)]
    args += [np.array([[ln[1][j] for ln in lanes]] * 2, dtype=np.uint64) for j in range(2)]
    got = N.philox4x32_10(*args)
    for j in range(4):
        assert got[j].shape == (2, 12) and got[j].dtype == np.uint64
        assert got[j].tolist() == [[ln[2][j] for ln in lanes]] * 2


# ---------------------------------------------------------------- 2. split21
def test_split21_is_a_bijection_of_126_bits():
    hits = np.zeros((6, 21), dtype=int)
    unused = []
    for word in range(4):
        for bit in range(32):
            call = [0, 0, 0, 0]
            call[word] = 1 << bit
            w = N.split21(*call)
            assert w.shape == (6,)
            set_bits = [(i, j) for i in range(6) for j in range(64) if (int(w[i]) >> j) & 1]
            assert len(set_bits) <= 1
            if set_bits:
                (i, j), = set_bits
                assert j < 21
                hits[i, j] += 1
            else:
                unused.append((word, bit))
    assert (hits == 1).all()
    assert unused == [(3, 30), (3, 31)]
    # common.h's layout: words 0..2 the high 21 bits of x / y / z; words 3..5 their 11 low bits under bits 0..9, 10..19, 20..29 of w
    w = N.split21(0xFFFFF800, 0, 0x7FF, 0x3FF << 10)
    assert [int(t) for t in w] == [0x1FFFFF, 0, 0, 0, 0x3FF << 11, 0x7FF]


def test_split21_words_are_below_2_to_21():
    rng = np.random.default_rng(0)
    call = [rng.integers(0, 2 ** 32, 4096, dtype=np.uint64) for _ in range(4)]
    w = N.split21(*call)
    assert w.shape == (4096, 6) and int(w.max()) < 2 ** 21
    assert int(N.split21(*[0xFFFFFFFF] * 4).min()) == 2 ** 21 - 1


# ---------------------------------------------------------------- 3. layout
DIMS, CHAINS = (5, 6, 70), 3


def test_counters_are_pairwise_distinct():
    c0, c1, c2, c3, k0, k1 = N.noise_counters(5, 7, CHAINS, DIMS)
    assert c0.shape == (CHAINS, 3, 6, 70)
    idx = (c1 << np.uint64(32)) | c0
    assert np.unique(idx).size == idx.size
    assert (c2 == 7).all() and (c3 == 0x5347).all() and int(k0) == 5 and int(k1) == 0
    # idx = chain * Vg + voxel index of the pair's even plane
    V = 5 * 6 * 70
    assert int(idx[2, 1, 3, 4]) == 2 * V + (2 * 6 + 3) * 70 + 4
    # a high index word reaches the counter (chains x voxels beyond 2^32 exist on the host only)
    c0, c1, *_ = N.noise_counters(5, 7, 2, DIMS, Vg=2 ** 33 + 1)
    assert int(c1[1, 0, 0, 0]) == 2 and int(c0[1, 0, 0, 0]) == 1


def test_chain_c_is_the_same_volume_further_along_the_index():
    """chain c of a C-chain call == chain 1 of a call whose chain stride is c times as long; chain 0 does not see the stride"""
    V = DIMS[0] * DIMS[1] * DIMS[2]
    w = N.noise_words(5, 7, CHAINS, DIMS)
    for c in range(1, CHAINS):
        shifted = N.noise_words(5, 7, 2, DIMS, Vg=c * V)
        assert np.array_equal(w[c], shifted[1])
        assert np.array_equal(w[0], shifted[0])
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2])


def test_iteration_and_seed_high_words_count():
    w = {it: N.noise_words(5, it, CHAINS, DIMS) for it in (7, 2 ** 32 + 7, 8)}
    for a, b in ((7, 2 ** 32 + 7), (7, 8), (8, 2 ** 32 + 7)):
        assert (w[a] != w[b]).mean() > 0.99
    assert (N.noise_words(5 + 2 ** 32, 7, CHAINS, DIMS) != w[7]).mean() > 0.99
    c0, c1, c2, c3, k0, k1 = N.noise_counters(5 + 2 ** 32, 2 ** 32 + 7, 1, DIMS)
    assert (c2 == 7).all() and (c3 == (0x5347 ^ 1)).all() and int(k0) == 5 and int(k1) == 1


# ---------------------------------------------------------------- 4. statistics of the restatement
SDIMS, SC = (12, 120, 120), 2          # 2 x 3 x 172 800 = 1 036 800 draws


@pytest.fixture(scope='module')
def draws():
    return {key: N.normals(seed, it, SC, SDIMS)[0] for key, (seed, it) in
            {'base': (5, 3), 'next_iteration': (5, 4), 'iteration_hi': (5, 2 ** 32 + 3), 'next_seed': (6, 3), 'seed_hi': (5 + 2 ** 32, 3)}.items()}


def uncorrelated(a, b, squares=False):
    """5 sigma: mean(a b) of independent standard normals has variance 1 / n; mean((a^2 - 1)(b^2 - 1)) has 4 / n"""
    a, b = a.flatten(), b.flatten()
    n = a.numel()
    assert abs(float((a * b).mean())) < 5.0 / math.sqrt(n)
    if squares:
        assert abs(float(((a * a - 1.0) * (b * b - 1.0)).mean())) < 5.0 * 2.0 / math.sqrt(n)


def test_moments(draws):
    x = draws['base'].flatten()
    n = x.numel()
    assert n > 10 ** 6
    assert abs(float(x.mean())) < 5.0 / math.sqrt(n)
    assert abs(float(x.var()) - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert abs(float((x ** 4).mean()) - 3.0) < 5.0 * math.sqrt(96.0 / n)          # var x^4 = E x^8 - 9 = 96
    assert float(x.abs().max()) <= N.R_MAX


def test_chains_iterations_and_seeds_are_uncorrelated(draws):
    x = draws['base']
    uncorrelated(x[0], x[1], squares=True)
    for other in ('next_iteration', 'iteration_hi', 'next_seed', 'seed_hi'):
        uncorrelated(x, draws[other], squares=True)


def test_channels_are_uncorrelated(draws):
    """(0, 1) share a Box-Muller pair on even planes, (1, 2) on odd ones: same radius, so the squares are looked at too"""
    x = draws['base']
    for a, b in ((0, 1), (0, 2), (1, 2)):
        uncorrelated(x[:, a], x[:, b], squares=True)
        uncorrelated(x[:, a, 0::2], x[:, b, 0::2], squares=True)
        uncorrelated(x[:, a, 1::2], x[:, b, 1::2], squares=True)


def test_neighbours_are_uncorrelated(draws):
    x = draws['base']
    for ax in (-1, -2, -3):
        n = x.shape[ax]
        uncorrelated(x.narrow(ax, 0, n - 1), x.narrow(ax, 1, n - 1), squares=True)
    # inside a pair of planes: every channel against every channel of the plane above; (2 even, 0 odd) share a Box-Muller pair
    for a in range(3):
        for b in range(3):
            uncorrelated(x[:, a, 0::2], x[:, b, 1::2], squares=True)
    # across pairs
    for a in range(3):
        uncorrelated(x[:, a, 1:-1:2], x[:, a, 2::2], squares=True)


# ---------------------------------------------------------------- 5. the tolerance
def exceed_share(wrong, where=None, iteration=7):
    """share of the elements `where` at which a planted mistake is further than `tol` from the restatement"""
    n, r = N.normals(5, iteration, CHAINS, DIMS)
    out = (torch.from_numpy(wrong) - n).abs() > N.tol(r)
    return float((out if where is None else out[where]).double().mean())


def test_tolerance_is_small_and_a_rounded_float32_evaluation_uses_a_quarter_at_most():
    worst = 0.0
    for it in (0, 7, 2 ** 32 + 7, 5, 65, 30):          # the last three hold the edge words
        words = N.noise_words(5, it, CHAINS, DIMS)
        n, r = N.normals_from_words(words, DIMS[0])
        assert float(N.tol(r).max()) < 1e-4 and float(N.tol(N.R_MAX)) < 1e-4
        dev = np.abs(N.normals_float32(words, DIMS[0]).astype(np.float64) - n)
        assert (dev <= N.floor(r)).all()               # FLOOR_C is a bound (derivation: the restatement's docstring)
        worst = max(worst, float((dev / N.tol(r)).max()))
    assert worst < 0.25
    print(f'correctly rounded float32 evaluation: worst deviation / tolerance = {worst:.4f}')


def test_tolerance_catches_the_chain_index_ignored():
    n0 = N.normals_from_words(N.noise_words(5, 7, 1, DIMS), DIMS[0])[0]
    wrong = np.repeat(n0, CHAINS, axis=0)
    assert exceed_share(wrong, np.s_[1:]) >= 0.99      # (chain 0 is drawn right by such a kernel)


def test_tolerance_catches_the_odd_plane_repeating_the_even_one():
    wrong = N.normals(5, 7, CHAINS, DIMS)[0].numpy().copy()
    wrong[:, :, 1::2] = wrong[:, :, 0:DIMS[0] - 1:2]
    assert exceed_share(wrong, np.s_[:, :, 1::2]) >= 0.99


def test_tolerance_catches_swapped_words():
    words = N.noise_words(5, 7, CHAINS, DIMS).copy()
    words[..., [1, 2]] = words[..., [2, 1]]
    wrong = N.normals_from_words(words, DIMS[0])[0]
    # e0, e1 (their b), e2 and o0 (their a) are touched; o1, o2 are not
    assert exceed_share(wrong, np.s_[:, :, 0::2]) >= 0.99
    assert exceed_share(wrong, np.s_[:, 0, 1::2]) >= 0.99
    assert exceed_share(wrong, np.s_[:, 1:, 1::2]) == 0.0


def test_tolerance_catches_sin_and_cos_swapped():
    wrong = N.normals_from_words(N.noise_words(5, 7, CHAINS, DIMS), DIMS[0], swap_trig=True)[0]
    assert exceed_share(wrong) >= 0.99


def test_tolerance_catches_20_bit_scaling_of_the_angle():
    wrong = N.normals_from_words(N.noise_words(5, 7, CHAINS, DIMS), DIMS[0], b_bits=20)[0]
    assert exceed_share(wrong) >= 0.99


def test_tolerance_catches_the_high_iteration_word_ignored():
    it = 2 ** 32 + 7
    wrong = N.normals_from_words(N.noise_words(5, it, CHAINS, DIMS, iteration_hi=False), DIMS[0])[0]
    assert np.array_equal(wrong, N.normals(5, 7, CHAINS, DIMS)[0].numpy())
    assert exceed_share(wrong, iteration=it) >= 0.99


def test_tolerance_catches_the_stream_word_omitted():
    wrong = N.normals_from_words(N.noise_words(5, 7, CHAINS, DIMS, stream=0), DIMS[0])[0]
    assert exceed_share(wrong) >= 0.99


# ---------------------------------------------------------------- 6. edge words
def test_edge_constants_are_what_the_search_finds():
    assert (N.EDGE_DIMS, N.EDGE_CHAINS, N.EDGE_SEED) == (DIMS, CHAINS, 5)
    assert N.find_edge('a_min') == N.EDGE_A_MIN
    assert N.find_edge('a_max') == N.EDGE_A_MAX
    assert N.find_edge('b_zero') == N.EDGE_B_ZERO


def test_edge_elements_are_what_they_are_for():
    for (it, c, vox, ch), kind in ((N.EDGE_A_MIN, 'a_min'), (N.EDGE_A_MAX, 'a_max'), (N.EDGE_B_ZERO, 'b_zero')):
        a, b, is_sin = N.element_words(N.noise_words(5, it, CHAINS, DIMS), DIMS[0])
        n, r = N.normals(5, it, CHAINS, DIMS)
        assert bool(torch.isfinite(n).all())
        at = (c, ch) + vox
        other = N.partner(DIMS, vox, ch)
        assert not is_sin[at] and other is not None
        at2 = (c, other[1]) + other[0]
        assert is_sin[at2] and a[at2] == a[at] and b[at2] == b[at]
        if kind == 'a_min':
            assert a[at] == 0 and float(r[at]) == pytest.approx(N.R_MAX, rel=1e-15)
            assert float(n[at] ** 2 + n[at2] ** 2) == pytest.approx(42.0 * math.log(2.0), rel=1e-14)
        if kind == 'a_max':
            assert a[at] == N.A_MAX and float(r[at]) == 0.0 and float(n[at]) == 0.0 and float(n[at2]) == 0.0
        if kind == 'b_zero':
            assert b[at] == 0 and float(n[at]) == float(r[at]) and float(n[at2]) == 0.0
