"""Integer restatement of the in-kernel Langevin noise (csrc/common.h: philox4x32_10, split21, box_muller21; drawn by perturb_kernel
in csrc/field_kernels.hip and perturb_sobolev_march_kernel in csrc/stencil_kernels.hip).  CPU only: numpy uint64 for the words,
float64 for the normals.

One Philox4x32-10 call per voxel PAIR (z even, z + 1) and chain: counter (idx lo, idx hi, iteration lo, 0x5347 ^ iteration hi), key
(seed lo, seed hi), idx = chain * Vg + voxel index of the pair's even plane.  split21 cuts the 128 bits into six 21-bit words
w0..w5; three Box-Muller pairs (a, b) = (w0,w1), (w2,w3), (w4,w5) give (n0, n1) = r (cos, sin)(2 pi b / 2^21) with
r = sqrt(-2 ln((a + 1) / 2^21)), assigned to (e0,e1), (e2,o0), (o1,o2): e the even plane, o the odd one, the index the channel.

Tolerance.  The words are exact; only box_muller21 rounds.  A correctly rounded float32 evaluation of the kernel's formula,
n = fl(fl(sqrt(fl(K fl(log2 u)))) fl(trig(v))) with K = fl32(-2 ln 2) and u, v exact, carries the relative errors d1 (log2), dK
(the constant), d2 (the product), d3 (sqrt), d4 (cos / sin, correctly rounded: relative) and d5 (the last product), each at most
2^-24: r is off by (d1 + dK + d2) / 2 + d3 <= 2.5 * 2^-24 relative, n by 4.5 * 2^-24 relative, and |n| <= r.  With the second-order
terms (below 21 * 2^-48) that is below FLOOR_C * 2^-24 * r with FLOOR_C = 5, a fortiori below the floor FLOOR_C * 2^-24 * (1 + r);
`tol` is 16 times the floor: room for units that are good to about an ulp instead of correctly rounded, and -- the `1 +` -- for a
sin / cos whose error is absolute near its zeros.  max tol = 80 * 2^-24 * (1 + sqrt(42 ln 2)) = 3.05e-5."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
BITS = 21
SCALE = float(1 << BITS)
STREAM = 0x5347
R_MAX = float(np.sqrt(42.0 * np.log(2.0)))      # a = 0: u = 2^-21, r = sqrt(2 * 21 ln 2) = 5.3956
FLOOR_C = 5.0
MARGIN = 16.0

# (pair k, which of its two normals) of the element (plane parity, channel): e0 e1 e2 / o0 o1 o2
SLOT = {(0, 0): (0, 0), (0, 1): (0, 1), (0, 2): (1, 0), (1, 0): (1, 1), (1, 1): (2, 0), (1, 2): (2, 1)}


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on uint64 arrays (or ints) holding 32-bit words -> (x, y, z, w), csrc/common.h's output order"""
    c0, c1, c2, c3, k0, k1 = (_u64(t) & M32 for t in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def split21(x, y, z, w):
    """the 128 bits of one call -> six 21-bit words, (..., 6): words 0..2 the 21 high bits of x / y / z, words 3..5 their 11 low bits
    under 10 bits of w each (w's bits 0..9, 10..19, 20..29; its two top bits are unused)"""
    x, y, z, w = (_u64(t) for t in (x, y, z, w))
    s11, lo11, lo10 = np.uint64(11), np.uint64(0x7FF), np.uint64(0x3FF)
    return np.stack([x >> s11, y >> s11, z >> s11,
                     (x & lo11) | ((w & lo10) << s11),
                     (y & lo11) | (((w >> np.uint64(10)) & lo10) << s11),
                     (z & lo11) | (((w >> np.uint64(20)) & lo10) << s11)], axis=-1)


def noise_counters(seed, iteration, C, dims, Vg=None, stream=STREAM, iteration_hi=True):
    """(c0, c1, c2, c3, k0, k1) of every call: arrays (C, pairs, H, W) and two scalars"""
    D, H, W = dims
    Vg = D * H * W if Vg is None else Vg
    seed, iteration = int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1)
    chain = np.arange(C, dtype=np.uint64).reshape(C, 1, 1, 1)
    pair = np.arange((D + 1) // 2, dtype=np.uint64).reshape(1, -1, 1, 1)
    y = np.arange(H, dtype=np.uint64).reshape(1, 1, H, 1)
    x = np.arange(W, dtype=np.uint64).reshape(1, 1, 1, W)
    idx = chain * np.uint64(Vg) + (np.uint64(2) * pair * np.uint64(H) + y) * np.uint64(W) + x
    c2 = np.full(idx.shape, iteration & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(idx.shape, stream ^ ((iteration >> 32) if iteration_hi else 0), dtype=np.uint64)
    return idx & M32, idx >> np.uint64(32), c2, c3, np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)


def noise_words(seed, iteration, C, dims, Vg=None, **kw):
    """the six 21-bit words of every call, uint64 (C, pairs, H, W, 6): per (chain, pair, column (y, x), word)"""
    return split21(*philox4x32_10(*noise_counters(seed, iteration, C, dims, Vg, **kw)))


def element_words(words, D):
    """words (C, pairs, H, W, 6) -> (a, b, is_sin), each (C, 3, D, H, W): the two words of the Box-Muller pair an element is drawn
    from and which of the pair's two normals it is; the odd plane of the last pair is dropped when D is odd"""
    C, P, H, W, _ = words.shape
    a, b = (np.empty((C, 3, 2 * P, H, W), dtype=np.uint64) for _ in range(2))
    is_sin = np.empty((C, 3, 2 * P, H, W), dtype=bool)
    for (parity, ch), (k, second) in SLOT.items():
        a[:, ch, parity::2], b[:, ch, parity::2], is_sin[:, ch, parity::2] = words[..., 2 * k], words[..., 2 * k + 1], bool(second)
    return a[:, :, :D], b[:, :, :D], is_sin[:, :, :D]


def radius(a):
    """float64 r = sqrt(-2 ln u), u = (a + 1) / 2^21 in (0, 1]"""
    return np.sqrt(-2.0 * np.log((a.astype(np.float64) + 1.0) / SCALE))


def cos_sin_revolutions(b, bits=BITS):
    """float64 (cos, sin)(2 pi b / 2^bits): the quadrant is taken off in integers, so the zeros and +-1 are exact"""
    b = _u64(b) & np.uint64((1 << bits) - 1)
    q = (b >> np.uint64(bits - 2)).astype(np.int64)
    f = (b & np.uint64((1 << (bits - 2)) - 1)).astype(np.float64) * (2.0 * np.pi / float(1 << bits))     # [0, pi / 2)
    c, s = np.cos(f), np.sin(f)
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def normals_from_words(words, D, swap_trig=False, b_bits=BITS):
    """words -> (normals, radius), float64 numpy (C, 3, D, H, W); the two switches plant mistakes (tests)"""
    a, b, is_sin = element_words(words, D)
    r = radius(a)
    c, s = cos_sin_revolutions(b, b_bits)
    return r * np.where(is_sin != swap_trig, s, c), r


def normals(seed, iteration, C, dims):
    """-> (n, r): the standard normals perturb_kernel draws and the Box-Muller radius of each, torch float64 (C, 3, D, H, W)"""
    n, r = normals_from_words(noise_words(seed, iteration, C, dims), dims[0])
    return torch.from_numpy(n), torch.from_numpy(r)


def normals_float32(words, D):
    """the kernel's formula with every operation correctly rounded to float32 (computed in float64 and rounded once; log2, sqrt
    and the products are far from double-rounding trouble at 53 against 24 bits); cos / sin of the EXACT revolution count,
    rounded -- the hardware takes revolutions.  -> float32 numpy (C, 3, D, H, W)"""
    f32 = lambda t: t.astype(np.float32).astype(np.float64)
    a, b, is_sin = element_words(words, D)
    u = (a.astype(np.float64) + 1.0) / SCALE                                  # exact in float32: 21 bits times a power of two
    K = float(np.float32(-1.3862943611198906))
    r = f32(np.sqrt(f32(K * f32(np.log2(u)))))
    c, s = cos_sin_revolutions(b)
    return f32(r * f32(np.where(is_sin, s, c))).astype(np.float32)


def floor(r):
    return FLOOR_C * 2.0 ** -24 * (1.0 + r)


def tol(r):
    """per-element tolerance of a float32 Box-Muller normal with radius r against the float64 restatement"""
    return MARGIN * floor(r)


# ---------------------------------------------------------------- edge words
EDGE_DIMS, EDGE_CHAINS, EDGE_SEED = (5, 6, 70), 3, 5
A_MAX = (1 << BITS) - 1
# the first EDGE_* call (iteration ascending, then storage order) that holds each edge word, as (iteration, chain, voxel, channel) of
# the COS element of the Box-Muller pair; re-derived by
# tests/test_langevin_noise_host.py (find_edge below)
EDGE_A_MIN = (5, 2, (4, 1, 39), 0)      # a = 0: u = 2^-21, the 5.4-sigma tail
EDGE_A_MAX = (65, 2, (3, 5, 14), 1)     # a = 2^21 - 1: u = 1, radius 0
EDGE_B_ZERO = (30, 1, (0, 4, 38), 0)    # b = 0: angle 0, the sin element is exactly 0


def partner(dims, voxel, channel):
    """the element that shares a Box-Muller pair with the COS element (voxel, channel) -- its sin element -- or None where the
    volume has no such element (the odd plane of the last pair of an odd D)"""
    z, y, x = voxel
    k, second = SLOT[z & 1, channel]
    assert second == 0
    (parity, ch), = [key for key, v in SLOT.items() if v == (k, 1)]
    zp = (z & ~1) + parity
    return ((zp, y, x), ch) if zp < dims[0] else None


def find_edge(kind, max_iteration=1000):
    """the first iteration (then chain, voxel, channel in storage order) of the EDGE_* call whose words hold an `a` of 0
    ('a_min'), an `a` of 2^21 - 1 ('a_max') or a `b` of 0 ('b_zero') in a pair whose cos element exists, and for 'b_zero' its sin
    element too -> (iteration, chain, (z, y, x), channel of the cos element)"""
    for it in range(max_iteration):
        a, b, is_sin = element_words(noise_words(EDGE_SEED, it, EDGE_CHAINS, EDGE_DIMS), EDGE_DIMS[0])
        hit = ~is_sin & {'a_min': a == 0, 'a_max': a == A_MAX, 'b_zero': b == 0}[kind]
        for c, ch, z, y, x in np.argwhere(hit):
            if kind != 'b_zero' or partner(EDGE_DIMS, (z, y, x), ch) is not None:
                return int(it), int(c), (int(z), int(y), int(x)), int(ch)
    return None
