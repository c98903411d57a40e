// a / 9.0f without the division: the divisor of every 3x3 / stride 1 / pad 1 average pool (vq_tsn_kernels.h: pool_unit).
// No HIP include: tests/test_pool_path.py compiles this header into a host program that walks all 2^32 floats.
#pragma once

#if defined(__HIPCC__)
#define VQ_DIV9_FN __host__ __device__ __forceinline__
#else
#define VQ_DIV9_FN static inline
#endif

namespace vq {

// The bits of the IEEE division a / 9.0f for EVERY float a (NaN payloads aside): q is within one ulp of the quotient (the rounded
// reciprocal times a), one FMA gives the exact remainder a - 9 q, a second folds the correction in (Markstein's sequence for a
// constant divisor).  Zeros and infinities -- where the remainder is (+0) + (-0) or inf - inf -- keep q, which is already right; so
// do quotients that underflow to zero.  Five instructions per value where the division takes eleven.
VQ_DIV9_FN float div9(float a) {
    const float z = 1.0f / 9.0f;
    const float q = a * z;
    const float r = __builtin_fmaf(-9.0f, q, a);
    const float c = __builtin_fmaf(r, z, q);
    return (q == 0.0f || __builtin_isinf(q)) ? q : c;
}

}  // namespace vq
