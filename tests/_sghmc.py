"""numpy float32 restatement of the SGHMC step (csrc/sghmc_device.h).  CPU only.  numpy rounds every float32 operation once and
contracts nothing, as the __f*_rn intrinsics of the kernels do, so results are compared bit for bit:

    t  = fsub(fmul(oma, m), fmul(lr, gs))                      oma = (float)(1 - (double)friction)
    m' = T > 0 ? fadd(t, fmul(fmul(amp, sigma), n)) : t        amp = (float)sqrt(2 friction lr T), in double
    v' = fadd(v, m')

friction, temperature and lr arrive in the library as C floats: the constants are formed from their float32 values.  The noise of
the Philox path is tests/_langevin_noise.py's with the stream word STREAM."""
import numpy as np

from tests import _langevin_noise as N

F32 = np.float32
STREAM = 0x484D


def constants(lr, friction, temperature):
    """(lr, oma, amp) as float32, rounded as the host code rounds them"""
    lr, friction, temperature = F32(lr), F32(friction), F32(temperature)
    oma = F32(1.0 - float(friction))
    amp = F32(np.sqrt(2.0 * float(friction) * float(lr) * float(temperature)))
    return lr, oma, amp


def step(v, m, grad, sigma, n, lr, friction, temperature):
    """one step on float32 arrays of one shape (sigma: None = 1; n: unused at temperature 0) -> (v', m')"""
    lr32, oma, amp = constants(lr, friction, temperature)
    v, m, grad = (np.asarray(t, dtype=F32) for t in (v, m, grad))
    t = oma * m - lr32 * grad
    assert t.dtype == F32
    if float(F32(temperature)) > 0.0:
        sg = F32(1.0) if sigma is None else np.asarray(sigma, dtype=F32)
        m1 = t + (amp * sg) * np.asarray(n, dtype=F32)
    else:
        m1 = t
    v1 = v + m1
    assert m1.dtype == F32 and v1.dtype == F32
    return v1, m1


def normals(seed, iteration, C, dims):
    """the standard normals of the SGHMC stream in float64 and their Box-Muller radii, numpy (C, 3, D, H, W)"""
    return N.normals_from_words(N.noise_words(seed, iteration, C, dims, stream=STREAM), dims[0])


def ar1_variance(amp, oma, n):
    """variance of the momentum after n gradient-free steps from zero, per unit sigma^2: amp^2 (1 - oma^(2n)) / (1 - oma^2)"""
    amp, oma = float(amp), float(oma)
    return amp * amp * n if oma == 1.0 else amp * amp * (1.0 - oma ** (2 * n)) / (1.0 - oma * oma)
