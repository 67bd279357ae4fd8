// Per-element arithmetic of the posterior principal modes ("Displacement modes"): the one term a record
// adds to a Gram sum, the one term it adds to a mode, and the explained-variance ratio of a voxel.  Plain host / device
// functions over scalars, so every kernel computes the same thing and a host build can check them.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace irs {

// acc + a b for two float32 values: the product of two 24-bit significands is exact in double, so whether the compiler fuses
// the multiply into the add or not, the result is the correctly rounded acc + (exact a b)
__host__ __device__ inline double modes_gram_term(double acc, float a, float b) { return acc + (double)a * (double)b; }

// acc + coeff x with the product and the sum each rounded once: never one fused operation (the helpers are functions of their
// own, which -ffp-contract=on does not look through)
__host__ __device__ inline double modes_mul(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dmul_rn(a, b);
#else
    const double p = a * b;
    return p;
#endif
}
__host__ __device__ inline double modes_add(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(a, b);
#else
    const double s = a + b;
    return s;
#endif
}
__host__ __device__ inline double modes_axpy(double acc, double coeff, float x) { return modes_add(acc, modes_mul(coeff, (double)x)); }

// one channel's sample variance from the sum and the sum of squares of its n >= 2 records: (sum x^2 - (sum x)^2 / n) / (n - 1)
__host__ __device__ inline double modes_variance(double sum, double sumsq, int n) {
    const double sq = modes_mul(sum, sum);
    const double corr = sq / (double)n;
    return modes_add(sumsq, -corr) / (double)(n - 1);
}

// num = sum_c s_c^2 sum_m mode_{m,c}^2, den = sum_c s_c^2 var_c -> explained: 0 where den is 0 (a voxel that never moved) and
// for n < 2; no clamp; a non-finite num or den propagates
__host__ __device__ inline float modes_explained(double num, double den, int n) {
    if (n < 2 || den == 0.0) return 0.0f;
    return (float)(num / den);
}

}  // namespace irs
