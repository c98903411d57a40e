// What the selection kernels of csrc/vq_sim.hip (vq_db_select, vq_db_topk, the partitions of the batched rounds) share with the batched
// top-k of csrc/vq_round_topk.hip: the order-mapped key of a score, the two predicates of the stable compaction, the block scan of its
// two counters, and the two wave-level steps of the MSB-first radix select (the histogram add and the pick of the next digit).  One
// definition each, as with csrc/vq_gauss_jordan.h.
#pragma once
#include "vq_common.h"

constexpr int SEL_ITEMS = 8;                       // consecutive rows per thread (keeps order)
constexpr int SEL_BLOCK = 256;
constexpr int SEL_CHUNK = SEL_ITEMS * SEL_BLOCK;   // rows per block
// a top-k of at most kTopkSmallK rows out of at most kTopkSmallN is ONE workgroup with the order keys in LDS (topk_small_kernel)
constexpr int kTopkSmallN = 16384, kTopkSmallK = 1024, kTopkSmallThreads = 1024;

// predicate mode 0: bit0 = v >= th, bit1 = lower <= v < th   (select)
// predicate mode 1: bit0 = key > pivot,  bit1 = key == pivot  (top-k; keys are order-mapped scores)
__device__ __forceinline__ uint64_t order_key(double v) {
    if (v != v) return 0ull;                                  // NaN sorts last
    if (v == 0.0) v = 0.0;                                     // -0 == +0
    uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);       // ascending in v; > 0 for every non-NaN
}

struct SelPred {
    int mode;
    double th, lower;
    uint64_t pivot;
    __device__ __forceinline__ int operator()(double v) const {
        if (mode == 0) return (v >= th ? 1 : 0) | ((lower <= v && v < th) ? 2 : 0);
        const uint64_t k = order_key(v);
        return (k > pivot ? 1 : 0) | ((k == pivot && k != 0ull) ? 2 : 0);
    }
};

__device__ __forceinline__ int2 block_scan_excl2(int2 v, int2* total) {
    // exclusive scan of two counters over the 256 threads of a block (4 waves)
    __shared__ int2 wsum[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int2 inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int ax = __shfl_up(inc.x, off, 64), ay = __shfl_up(inc.y, off, 64);
        if (lane >= off) {
            inc.x += ax;
            inc.y += ay;
        }
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    int2 base = make_int2(0, 0), tot = make_int2(0, 0);
    for (int i = 0; i < 4; ++i) {
        if (i < wid) {
            base.x += wsum[i].x;
            base.y += wsum[i].y;
        }
        tot.x += wsum[i].x;
        tot.y += wsum[i].y;
    }
    __syncthreads();
    *total = tot;
    return make_int2(base.x + inc.x - v.x, base.y + inc.y - v.y);
}

// One wave's add into a 256-bin histogram in LDS; call with the whole wave.  The keys of a pass crowd into few bins (every score of a
// ranking shares its sign and most of its exponent): the lanes that agree with the wave's first live lane are counted by ONE atomic,
// the others add themselves.  digit = -1 for a lane that is not live.
__device__ __forceinline__ void radix_hist_add(unsigned int* hist, bool live, int digit, int lane) {
    const unsigned long long act = __ballot(live);
    if (act) {
        const int lead = __ffsll((long long)act) - 1;
        const int first = __shfl(digit, lead, 64);
        const unsigned long long same = __ballot(digit == first);
        if (lane == lead)
            atomicAdd(&hist[first], (unsigned)__popcll(same));
        else if (live && digit != first)
            atomicAdd(&hist[digit], 1u);
    }
}

// topk_pick_kernel by one wave (call with lanes 0..63 of it, behind a barrier after the histogram): lane l owns bins 4l .. 4l+3.  The
// bin b the serial walk from 255 downwards stops in is the highest b with count(bins >= b) >= need (b = 0 if none); *prefix_out gets
// prefix | b << shift and *need_out what is still to find inside that bin, written by one lane.
__device__ __forceinline__ void radix_pick_wave(const unsigned int* hist, int lane, unsigned need, uint64_t prefix, int shift, uint64_t* prefix_out,
                                                unsigned int* need_out) {
    const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    unsigned above = h0 + h1 + h2 + h3;                      // inclusive suffix sum over the lanes: bins >= 4l
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_down(above, off, 64);
        if (lane + off < 64) above += o;
    }
    const unsigned gt3 = above - (h0 + h1 + h2 + h3);        // elements in bins > 4l+3
    int found = -1;
    unsigned rest = 0;
    if (gt3 + h3 >= need) {
        found = 4 * lane + 3;
        rest = need - gt3;
    } else if (gt3 + h3 + h2 >= need) {
        found = 4 * lane + 2;
        rest = need - gt3 - h3;
    } else if (gt3 + h3 + h2 + h1 >= need) {
        found = 4 * lane + 1;
        rest = need - gt3 - h3 - h2;
    } else if (gt3 + h3 + h2 + h1 + h0 >= need) {
        found = 4 * lane;
        rest = need - gt3 - h3 - h2 - h1;
    }
    const unsigned long long have = __ballot(found >= 0 && gt3 < need);   // lanes whose own bins contain the stop
    // the stop lies in the HIGHEST lane for which bins above it hold fewer than `need` and its own close the gap
    const int top = have ? 63 - __builtin_clzll(have) : -1;
    if (top < 0) {
        if (lane == 0) {                                     // fewer than `need` keys under this prefix: bin 0, need minus all above it
            *prefix_out = prefix;
            *need_out = need - (above - h0);
        }
    } else if (lane == top) {
        if (found == 0) rest = need - (above - h0);          // the serial walk never tests bin 0: it takes what is left
        *prefix_out = prefix | ((uint64_t)found << shift);
        *need_out = rest;
    }
}
