// The score of a clip from its stream means, shared by the scans of csrc/vq_sim.hip, the ranking of csrc/vq_rank.hip and the batched fit and rescore of
// csrc/vq_rounds.hip.  One definition; every unit that includes it is compiled with -ffp-contract=off.
#pragma once
#include "vq_common.h"

// ticket.py:172-180 -- same IEEE operations in the same order (contraction is off for this file).
__device__ __forceinline__ double score_from_avg(const double* a, const double* w, int S) {
    double ssum = 0.0, denom = 0.0;
    for (int s = 0; s < S; ++s) {
        const double term = w[s] * (1.0 - a[s]);
        ssum = ssum + term * term;
        denom = denom + w[s] * w[s];
    }
    return 1.0 - sqrt(ssum / denom);
}
