// What the selection kernels of csrc/vq_rank.hip (vq_db_select, vq_db_topk) share with the partitions of the batched rounds
// (csrc/vq_rounds.hip) and the batched top-k of csrc/vq_round_topk.hip: the order-mapped key of a score, the two predicates of the
// stable compaction, the block scan of its two counters, the four blocks of the stable partition, and the two wave-level steps of the
// MSB-first radix select (the histogram add and the pick of the next digit).  One definition each, as with csrc/vq_gauss_jordan.h.
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

// ---- the stable partition of a score array (ticket.py:325-340), as the blocks that the one-query kernels of csrc/vq_rank.hip and the
// batched ones of csrc/vq_rounds.hip are made of ----
// pass 1: per-block counts of both classes + block-local first-argmax of class 1 (near band)
__device__ __forceinline__ void select_count_block(const double* scores, int64_t n, SelPred pred, int2* blk_cnt, double* blk_max,
                                                   int64_t* blk_arg) {
    const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_ITEMS;
    int2 cnt = make_int2(0, 0);
    double bmax = -INFINITY;
    int64_t barg = -1;
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int64_t r = base + i;
        if (r < n) {
            const double v = scores[r];
            const int f = pred(v);
            cnt.x += f & 1;
            cnt.y += (f >> 1) & 1;
            if ((f & 2) && (barg < 0 || v > bmax)) {
                bmax = v;
                barg = r;
            }
        }
    }
    int2 tot;
    block_scan_excl2(cnt, &tot);
    // first-argmax across the block: larger value wins, ties go to the smaller row
    __shared__ double smax[SEL_BLOCK];
    __shared__ int64_t sarg[SEL_BLOCK];
    smax[threadIdx.x] = bmax;
    sarg[threadIdx.x] = barg;
    __syncthreads();
    for (int off = SEL_BLOCK / 2; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            const double ov = smax[threadIdx.x + off];
            const int64_t oa = sarg[threadIdx.x + off];
            const int64_t ma = sarg[threadIdx.x];
            if (oa >= 0 && (ma < 0 || ov > smax[threadIdx.x] || (ov == smax[threadIdx.x] && oa < ma))) {
                smax[threadIdx.x] = ov;
                sarg[threadIdx.x] = oa;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = tot;
        blk_max[blockIdx.x] = smax[0];
        blk_arg[blockIdx.x] = sarg[0];
    }
}

// pass 2 (one block): exclusive scan of the block counts, totals and global first-argmax
// result[0] = n_class0, result[1] = n_class1, result[2] = argmax row (-1 if none)
__device__ __forceinline__ void select_scan_block(int2* blk_cnt, const double* blk_max, const int64_t* blk_arg, int nblk, int64_t* result,
                                                  int64_t limit1 /* cap on class-1 picks, <0 = none */) {
    __shared__ int2 carry;
    __shared__ double gmax;
    __shared__ int64_t garg;
    if (threadIdx.x == 0) {
        carry = make_int2(0, 0);
        gmax = -INFINITY;
        garg = -1;
    }
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += SEL_BLOCK) {
        const int b = b0 + threadIdx.x;
        int2 v = b < nblk ? blk_cnt[b] : make_int2(0, 0);
        int2 tot;
        const int2 ex = block_scan_excl2(v, &tot);
        const int2 c0 = carry;
        if (b < nblk) blk_cnt[b] = make_int2(c0.x + ex.x, c0.y + ex.y);
        __syncthreads();
        if (threadIdx.x == 0) {
            carry = make_int2(c0.x + tot.x, c0.y + tot.y);
            for (int i = b0; i < min(nblk, b0 + SEL_BLOCK); ++i) {   // serial, in order: first max wins
                if (blk_arg[i] >= 0 && (garg < 0 || blk_max[i] > gmax)) {
                    gmax = blk_max[i];
                    garg = blk_arg[i];
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        result[0] = carry.x;
        result[1] = (limit1 >= 0 && carry.y > limit1) ? limit1 : carry.y;
        result[2] = garg;
    }
}

// pass 3: scatter rows in original order.  class-1 rows beyond `limit1` (in order) are dropped.
__device__ __forceinline__ void select_scatter_block(const double* scores, int64_t n, SelPred pred, const int2* blk_off, int64_t* out0,
                                                     int64_t* out1, int64_t limit1, int64_t* pre0, int64_t* pre1, int64_t prefix) {
    const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_ITEMS;
    int flags[SEL_ITEMS];
    int2 cnt = make_int2(0, 0);
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int64_t r = base + i;
        flags[i] = r < n ? pred(scores[r]) : 0;
        cnt.x += flags[i] & 1;
        cnt.y += (flags[i] >> 1) & 1;
    }
    int2 tot;
    const int2 ex = block_scan_excl2(cnt, &tot);
    int64_t o0 = (int64_t)blk_off[blockIdx.x].x + ex.x;
    int64_t o1 = (int64_t)blk_off[blockIdx.x].y + ex.y;
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        if (flags[i] & 1) {
            if (o0 < prefix) pre0[o0] = base + i;            // the head of each list a second time, next to the counts (one copy back)
            out0[o0++] = base + i;
        }
        if (flags[i] & 2) {
            if (limit1 < 0 || o1 < limit1) {
                out1[o1] = base + i;
                if (o1 < prefix) pre1[o1] = base + i;
            }
            ++o1;
        }
    }
}

// The three passes above as ONE launch of one workgroup for a small database (n <= kSelSmallN): a thread owns a run of consecutive
// rows, counts / first-arg-max / offsets meet in LDS.  Same lists, same counts, same arg-max as the three-kernel form (tested).
constexpr int kSelSmallN = 16384, kSelSmallThreads = 1024;
__device__ __forceinline__ void select_small_block(const double* scores, int n, SelPred pred, int64_t* result, int64_t* out0, int64_t* out1,
                                                   int64_t* pre0, int64_t* pre1, int prefix) {
    __shared__ int2 s_wave[kSelSmallThreads / 64];
    __shared__ double s_max[kSelSmallThreads / 64];
    __shared__ int s_arg[kSelSmallThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = (n + kSelSmallThreads - 1) / kSelSmallThreads;          // <= 16
    const int r0 = tid * per, r1 = min(n, r0 + per);
    int2 cnt = make_int2(0, 0);
    unsigned flags = 0;                                                     // 2 bits per row of the run
    double bmax = -INFINITY;
    int barg = -1;
    for (int r = r0; r < r1; ++r) {
        const double v = scores[r];
        const int f = pred(v);
        flags |= (unsigned)f << (2 * (r - r0));
        cnt.x += f & 1;
        cnt.y += (f >> 1) & 1;
        if ((f & 2) && (barg < 0 || v > bmax)) {                             // first maximum of the run
            bmax = v;
            barg = r;
        }
    }
    int2 inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int ax = __shfl_up(inc.x, off, 64), ay = __shfl_up(inc.y, off, 64);
        if (lane >= off) {
            inc.x += ax;
            inc.y += ay;
        }
    }
    // first arg-max across the wave: larger value wins, ties go to the smaller row
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_down(bmax, off, 64);
        const int oa = __shfl_down(barg, off, 64);
        if (lane + off < 64 && oa >= 0 && (barg < 0 || ov > bmax || (ov == bmax && oa < barg))) {
            bmax = ov;
            barg = oa;
        }
    }
    if (lane == 63) s_wave[wid] = inc;
    if (lane == 0) {
        s_max[wid] = bmax;
        s_arg[wid] = barg;
    }
    __syncthreads();
    int2 base = make_int2(0, 0), tot = make_int2(0, 0);
    for (int i = 0; i < kSelSmallThreads / 64; ++i) {
        if (i < wid) {
            base.x += s_wave[i].x;
            base.y += s_wave[i].y;
        }
        tot.x += s_wave[i].x;
        tot.y += s_wave[i].y;
    }
    int o0 = base.x + inc.x - cnt.x, o1 = base.y + inc.y - cnt.y;
    for (int r = r0; r < r1; ++r) {
        const unsigned f = (flags >> (2 * (r - r0))) & 3u;
        if (f & 1u) {
            if (o0 < prefix) pre0[o0] = r;
            out0[o0++] = r;
        }
        if (f & 2u) {
            if (o1 < prefix) pre1[o1] = r;
            out1[o1++] = r;
        }
    }
    if (tid == 0) {
        double gmax = -INFINITY;
        int garg = -1;
        for (int i = 0; i < kSelSmallThreads / 64; ++i)                      // in row order: the first maximum wins
            if (s_arg[i] >= 0 && (garg < 0 || s_max[i] > gmax)) {
                gmax = s_max[i];
                garg = s_arg[i];
            }
        result[0] = tot.x;
        result[1] = tot.y;
        result[2] = garg;
    }
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
