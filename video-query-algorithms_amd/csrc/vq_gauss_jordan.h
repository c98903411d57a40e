// The dense solve of target bootstrapping (csrc/vq_boot.hip, csrc/vq_round_targets.hip): ONE definition, so that every kernel that
// solves a bootstrapping system performs the same operations in the same order -- the batched targets promise the bits of the
// one-draw call.
#pragma once
#include "vq_common.h"

namespace vq {

// A pivot counts only above the rounding noise of its column: dim * kPivotTol * the largest entry the column had before
// elimination.  Linearly dependent rows (a clip validated twice, a multiple of another row) leave a column of residues of a
// few ulps of that size; an exact zero is the exception there, not the rule (dozens of percent of such inputs used to come
// back as a finite "target").  The floor scales with the data, sits 2^-40 (256 rows) .. 2^-48 (1 row) below the column and
// never changes which pivot is taken, so every accepted system is solved to the same bits as without it.
constexpr double kPivotTol = 16.0 * 2.220446049250313e-16;     // per row of the system, in units of the column's largest entry

// Solve A Z = R in place on the augmented matrix aug[dim][dim + nrhs] (row stride ld): Gauss-Jordan with partial
// pivoting, whole workgroup.  Returns false on a negligible (see above) / non-finite pivot.  piv_floor: dim doubles of LDS.
static __device__ bool gauss_jordan(double* aug, int dim, int nrhs, int ld, int* piv_shared, double* piv_floor) {
    const int tid = threadIdx.x, nt = blockDim.x, width = dim + nrhs;
    for (int c = tid; c < dim; c += nt) {
        double cm = 0.0;
        for (int r = 0; r < dim; ++r) {
            const double v = fabs(aug[(size_t)r * ld + c]);
            if (v > cm) cm = v;
        }
        piv_floor[c] = (kPivotTol * dim) * cm;
    }
    __syncthreads();
    for (int k = 0; k < dim; ++k) {
        if (tid == 0) {
            int best = k;
            double bv = fabs(aug[(size_t)k * ld + k]);
            for (int r = k + 1; r < dim; ++r) {
                const double v = fabs(aug[(size_t)r * ld + k]);
                if (v > bv) {
                    bv = v;
                    best = r;
                }
            }
            *piv_shared = (bv > piv_floor[k] && bv < 1.0e300) ? best : -1;
        }
        __syncthreads();
        const int p = *piv_shared;
        if (p < 0) return false;
        if (p != k)
            for (int c = tid; c < width; c += nt) {
                const double t = aug[(size_t)k * ld + c];
                aug[(size_t)k * ld + c] = aug[(size_t)p * ld + c];
                aug[(size_t)p * ld + c] = t;
            }
        __syncthreads();
        const double inv = 1.0 / aug[(size_t)k * ld + k];
        __syncthreads();
        for (int c = tid; c < width; c += nt) aug[(size_t)k * ld + c] *= inv;
        __syncthreads();
        // eliminate column k from every other row; the factor is read before anybody overwrites column k
        for (int idx = tid; idx < dim * (width - k - 1); idx += nt) {
            const int r = idx / (width - k - 1), c = k + 1 + idx % (width - k - 1);
            if (r != k) aug[(size_t)r * ld + c] -= aug[(size_t)r * ld + k] * aug[(size_t)k * ld + c];
        }
        __syncthreads();
        for (int r = tid; r < dim; r += nt)
            if (r != k) aug[(size_t)r * ld + k] = 0.0;
        __syncthreads();
    }
    return true;
}

}  // namespace vq
