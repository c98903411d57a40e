// Batched query rounds on gfx950: the k best clips of every query of the last batched round in one call (include/vq_amd_round_topk.h).
//
// What it replaces (paths relative to the reference checkout):
//   src/models/ticket.py:266   the stable descending sort of the report -- here per query of a batched round: descending score, ties by
//                              ascending position, -0 == +0, NaN excluded (the rules of vq_db_topk and order_key, csrc/vq_select.h)
//
// vq_db_topk ranks the handle's one-query scores: 19 launches, three synchronisations and a sort on the host.  The scores of a batched
// round sit in the round's own device block, [M_q] per query; this unit ranks all of them in one call -- one upload (the k's), one
// synchronisation, one copy back -- with the query as a grid dimension, so the launch count depends neither on Q nor on k:
//
//   short pieces (M_q <= kTopkSmallN and k_q <= kTopkSmallK): ONE launch, a workgroup per query -- topk_small_kernel's eight radix
//       passes over keys in LDS and its stable compaction, then a bitonic sort of the survivors in LDS, then the stores
//   long pieces: eight histogram launches (a workgroup's LDS histogram, one global add per bin; the pick of the digit before is
//       redone by every workgroup from the histogram of the pass before, so pivot and need never leave the device and no launch sits
//       between two passes), the count / scan / scatter compaction with predicate mode 1 and the pivot read from device memory (ties
//       at the pivot keep the FIRST `need` positions) into this call's own lists, and one sort launch, a workgroup per query
//
// A workgroup of the form its query does not take returns at once.  Nothing of the round's snapshot or of the handle's one-query
// state is written.
#include <algorithm>
#include <climits>

#include "vq_db.h"
#include "vq_select.h"

using namespace vq;

namespace {

constexpr int kTopkSlots = 16;             // queries per call (the slots of a batched round)
constexpr int kTopkCap = 4096;             // the largest k: 48 KB of (key, position) pairs in the sort kernel's local memory
constexpr int kTopkSortThreads = 1024;
constexpr int kTopkHistBlocks = 256;       // workgroups per query of a histogram pass, at the most (each walks its piece grid-strided)

// off[6]: see include/vq_amd_round_topk.h
void topk_layout(int Q, int64_t k_max, int64_t* off) {
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * 8);
    off[2] = off[1] + up64((int64_t)Q * 8);
    off[3] = off[2] + up64((int64_t)Q * k_max * 8);
    off[4] = off[3] + up64((int64_t)Q * k_max * 8);
    off[5] = kTopkCap;
}

int topk_shape(int Q, int64_t k_max) {
    VQ_REQUIRE(Q >= 1 && Q <= kTopkSlots, "n_queries must be in [1,%d] (got %d)", kTopkSlots, Q);
    VQ_REQUIRE(k_max >= 1 && k_max <= kTopkCap, "k_max must be in [1,%d] (got %lld)", kTopkCap, (long long)k_max);
    return VQ_OK;
}

struct TopkBatchArgs {
    const double* scores;      // the scores of the round: query q's piece is scores[qoff[q] .. qoff[q] + m[q])
    const int64_t* k;          // [Q], the uploaded piece of the block
    int64_t* count;            // [Q]
    int64_t* rows;             // [Q][k_max]
    double* vals;              // [Q][k_max]
    int64_t k_max;
    uint64_t* state;           // [9][16][2]: prefix | need BEFORE pass p (p = 8: pivot | ties to keep); entry 0 is never stored
    unsigned int* hist;        // [8][16][256]
    int64_t* total;            // [16][2]: keys above the pivot | ties kept
    int2* blk_cnt;             // the blocks of the long pieces, query after query
    int64_t* cand;             // [16][k_max]: the survivors of a long piece in position order, keys above the pivot first
    int64_t qoff[kTopkSlots], m[kTopkSlots];
    int32_t bstart[kTopkSlots + 1];   // the first block of query q; a short or skipped piece has none
};

// sorts P (a power of two) pairs in LDS: key descending, position ascending; call with the whole workgroup
__device__ __forceinline__ void bitonic_sort_pairs(uint64_t* key, int32_t* pos, int P, int tid, int nthreads) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nthreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t ki = key[i], kl = key[l];
                    const int32_t pi = pos[i], pl = pos[l];
                    const bool l_first = kl > ki || (kl == ki && pl < pi), i_first = ki > kl || (ki == kl && pi < pl);
                    if ((i & k) == 0 ? l_first : i_first) {
                        key[i] = kl;
                        key[l] = ki;
                        pos[i] = pl;
                        pos[l] = pi;
                    }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- short pieces: one workgroup per query ----------------------------------------------------------------------------------------
// topk_small_kernel (csrc/vq_rank.hip) per query of the round, with the final order made here: keys in LDS, eight histogram passes
// separated by barriers, the stable compaction into LDS, a bitonic sort of the at most kTopkSmallK survivors, the stores.
__global__ __launch_bounds__(kTopkSmallThreads) void topk_batch_small_kernel(TopkBatchArgs a) {
    const int q = blockIdx.x;
    const int64_t kq = a.k[q];
    if (kq <= 0 || a.bstart[q + 1] != a.bstart[q]) return;             // skipped, or a long piece
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(topk_lds);          // [n]
    __shared__ unsigned int hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ unsigned int s_need;
    __shared__ int2 s_wave[kTopkSmallThreads / 64];
    __shared__ uint64_t s_key[kTopkSmallK];
    __shared__ int32_t s_pos[kTopkSmallK];
    const int tid = threadIdx.x;
    const int n = (int)a.m[q];
    if (n <= 0) {                                                    // an empty view
        if (tid == 0) a.count[q] = 0;
        return;
    }
    const double* scores = a.scores + a.qoff[q];
    const int k = (int)(kq < (int64_t)n ? kq : (int64_t)n);
    for (int i = tid; i < n; i += kTopkSmallThreads) keys[i] = order_key(scores[i]);
    if (tid == 0) {
        s_prefix = 0ull;
        s_need = (unsigned)k;
    }
    for (int pass = 0; pass < 8; ++pass) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const int shift = 56 - 8 * pass;
        const uint64_t prefix = s_prefix;
        const uint64_t mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
        for (int i0 = 0; i0 < n; i0 += kTopkSmallThreads) {
            const int i = i0 + tid;
            const uint64_t key = i < n ? keys[i] : 0ull;
            const bool live = key != 0ull && (key & mask) == prefix;
            radix_hist_add(hist, live, live ? (int)((key >> shift) & 255) : -1, tid & 63);
        }
        __syncthreads();
        if (tid < 64) radix_pick_wave(hist, tid, s_need, prefix, shift, &s_prefix, &s_need);
        __syncthreads();
    }
    const uint64_t pivot = s_prefix;
    const int need = (int)s_need;
    // stable compaction: a thread owns a run of consecutive positions
    const int per = (n + kTopkSmallThreads - 1) / kTopkSmallThreads;
    const int r0 = min(n, tid * per), r1 = min(n, r0 + per);
    int2 cnt = make_int2(0, 0);
    for (int r = r0; r < r1; ++r) {
        const uint64_t key = keys[r];
        cnt.x += key > pivot ? 1 : 0;
        cnt.y += (key == pivot && key != 0ull) ? 1 : 0;
    }
    const int lane = tid & 63, wid = tid >> 6;
    int2 inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int ax = __shfl_up(inc.x, off, 64), ay = __shfl_up(inc.y, off, 64);
        if (lane >= off) {
            inc.x += ax;
            inc.y += ay;
        }
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    int2 base = make_int2(0, 0), tot = make_int2(0, 0);
    for (int i = 0; i < kTopkSmallThreads / 64; ++i) {
        if (i < wid) {
            base.x += s_wave[i].x;
            base.y += s_wave[i].y;
        }
        tot.x += s_wave[i].x;
        tot.y += s_wave[i].y;
    }
    int o0 = base.x + inc.x - cnt.x, o1 = base.y + inc.y - cnt.y;
    const int n_gt = min(tot.x, k), n_eq = min(min(tot.y, need), k - n_gt);
    const int total = n_gt + n_eq;                                   // <= k <= kTopkSmallK
    for (int r = r0; r < r1; ++r) {
        const uint64_t key = keys[r];
        if (key > pivot) {
            if (o0 < n_gt) {
                s_key[o0] = key;
                s_pos[o0] = r;
            }
            ++o0;
        } else if (key == pivot && key != 0ull) {
            if (o1 < n_eq) {
                s_key[n_gt + o1] = key;
                s_pos[n_gt + o1] = r;
            }
            ++o1;
        }
    }
    if (total == 0) {                                                // nothing but NaN
        if (tid == 0) a.count[q] = 0;
        return;
    }
    const int P = pow2_at_least(total);                              // <= kTopkSmallK, a power of two itself
    for (int i = total + tid; i < P; i += kTopkSmallThreads) {
        s_key[i] = 0ull;
        s_pos[i] = INT_MAX;
    }
    __syncthreads();
    bitonic_sort_pairs(s_key, s_pos, P, tid, kTopkSmallThreads);
    int64_t* out_rows = a.rows + (int64_t)q * a.k_max;
    double* out_vals = a.vals + (int64_t)q * a.k_max;
    for (int i = tid; i < total && i < a.k_max; i += kTopkSmallThreads) {
        const int r = s_pos[i];
        out_rows[i] = r;
        out_vals[i] = r < n ? scores[r] : 0.0;
    }
    if (tid == 0) a.count[q] = total;
}

// ---- long pieces ------------------------------------------------------------------------------------------------------------------
// The state BEFORE pass p of query q into LDS, by every workgroup on its own: pass 0 starts from (no prefix, min(k, M)); a later one
// redoes topk_pick_kernel's step on the histogram of the pass before (complete: that pass was the launch before) and the state before
// it.  The first workgroup of the query stores it for the launch after this one.  p = 8: the pivot and the ties to keep.
__device__ __forceinline__ void topk_load_state(const TopkBatchArgs& a, int q, int p, uint64_t* s_prefix, unsigned int* s_need) {
    const int tid = threadIdx.x;
    const unsigned first = (unsigned)(a.k[q] < a.m[q] ? a.k[q] : a.m[q]);
    if (p == 0) {
        if (tid == 0) {
            *s_prefix = 0ull;
            *s_need = first;
        }
    } else if (tid < 64) {
        const uint64_t* before = a.state + ((p - 1) * kTopkSlots + q) * 2;
        const uint64_t prefix = p == 1 ? 0ull : before[0];
        const unsigned need = p == 1 ? first : (unsigned)before[1];
        radix_pick_wave(a.hist + ((p - 1) * kTopkSlots + q) * 256, tid, need, prefix, 56 - 8 * (p - 1), s_prefix, s_need);
    }
    __syncthreads();
    if (p > 0 && blockIdx.x == 0 && tid == 0) {
        uint64_t* now = a.state + (p * kTopkSlots + q) * 2;
        now[0] = *s_prefix;
        now[1] = *s_need;
    }
}

__global__ __launch_bounds__(256) void topk_batch_hist_kernel(TopkBatchArgs a, int pass) {
    const int q = blockIdx.y;
    if (a.bstart[q + 1] == a.bstart[q]) return;                      // a short or skipped piece
    __shared__ unsigned int h[256];
    __shared__ uint64_t s_prefix;
    __shared__ unsigned int s_need;
    const int tid = threadIdx.x;
    h[tid] = 0u;
    topk_load_state(a, q, pass, &s_prefix, &s_need);                 // ends behind a barrier
    const int shift = 56 - 8 * pass;
    const uint64_t prefix = s_prefix;
    const uint64_t mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    const double* scores = a.scores + a.qoff[q];
    const int64_t n = a.m[q], stride = (int64_t)gridDim.x * 256;
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < n; r0 += stride) {
        const int64_t r = r0 + tid;
        const uint64_t key = r < n ? order_key(scores[r]) : 0ull;
        const bool live = key != 0ull && (key & mask) == prefix;
        radix_hist_add(h, live, live ? (int)((key >> shift) & 255) : -1, tid & 63);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&a.hist[(pass * kTopkSlots + q) * 256 + tid], h[tid]);
}

// the count / scan / scatter compaction of csrc/vq_rank.hip with predicate mode 1, the pivot of each query read on the device
__global__ __launch_bounds__(SEL_BLOCK) void topk_batch_count_kernel(TopkBatchArgs a) {
    const int q = blockIdx.y, b0 = a.bstart[q];
    if ((int)blockIdx.x >= a.bstart[q + 1] - b0) return;
    __shared__ uint64_t s_prefix;
    __shared__ unsigned int s_need;
    topk_load_state(a, q, 8, &s_prefix, &s_need);
    SelPred pred;
    pred.mode = 1;
    pred.th = pred.lower = 0.0;
    pred.pivot = s_prefix;
    const double* scores = a.scores + a.qoff[q];
    const int64_t n = a.m[q], base = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_ITEMS;
    int2 cnt = make_int2(0, 0);
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        const int64_t r = base + i;
        if (r < n) {
            const int f = pred(scores[r]);
            cnt.x += f & 1;
            cnt.y += (f >> 1) & 1;
        }
    }
    int2 tot;
    block_scan_excl2(cnt, &tot);
    if (threadIdx.x == 0) a.blk_cnt[b0 + blockIdx.x] = tot;
}

__global__ __launch_bounds__(SEL_BLOCK) void topk_batch_scan_kernel(TopkBatchArgs a) {
    const int q = blockIdx.x, b0 = a.bstart[q], nblk = a.bstart[q + 1] - b0;
    if (nblk <= 0) return;
    __shared__ int2 carry;
    if (threadIdx.x == 0) carry = make_int2(0, 0);
    __syncthreads();
    int2* blk_cnt = a.blk_cnt + b0;
    for (int c0 = 0; c0 < nblk; c0 += SEL_BLOCK) {
        const int b = c0 + threadIdx.x;
        const int2 v = b < nblk ? blk_cnt[b] : make_int2(0, 0);
        int2 tot;
        const int2 ex = block_scan_excl2(v, &tot);
        const int2 c = carry;
        if (b < nblk) blk_cnt[b] = make_int2(c.x + ex.x, c.y + ex.y);
        __syncthreads();
        if (threadIdx.x == 0) carry = make_int2(c.x + tot.x, c.y + tot.y);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t need = (int64_t)a.state[(8 * kTopkSlots + q) * 2 + 1], cap = a.k_max;
        const int64_t n_gt = carry.x < cap ? carry.x : cap;
        int64_t n_eq = carry.y < need ? carry.y : need;
        if (n_eq > cap - n_gt) n_eq = cap - n_gt;
        a.total[2 * q] = n_gt;
        a.total[2 * q + 1] = n_eq;
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void topk_batch_scatter_kernel(TopkBatchArgs a) {
    const int q = blockIdx.y, b0 = a.bstart[q];
    if ((int)blockIdx.x >= a.bstart[q + 1] - b0) return;
    SelPred pred;
    pred.mode = 1;
    pred.th = pred.lower = 0.0;
    pred.pivot = a.state[(8 * kTopkSlots + q) * 2];
    const int64_t n_gt = a.total[2 * q], n_eq = a.total[2 * q + 1];
    const double* scores = a.scores + a.qoff[q];
    const int64_t n = a.m[q], base = (int64_t)blockIdx.x * SEL_CHUNK + (int64_t)threadIdx.x * SEL_ITEMS;
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
    int64_t o0 = (int64_t)a.blk_cnt[b0 + blockIdx.x].x + ex.x;
    int64_t o1 = (int64_t)a.blk_cnt[b0 + blockIdx.x].y + ex.y;
    int64_t* cand = a.cand + (int64_t)q * a.k_max;                   // n_gt + n_eq <= k_max (topk_batch_scan_kernel)
#pragma unroll
    for (int i = 0; i < SEL_ITEMS; ++i) {
        if (flags[i] & 1) {
            if (o0 < n_gt) cand[o0] = base + i;
            ++o0;
        }
        if (flags[i] & 2) {
            if (o1 < n_eq) cand[n_gt + o1] = base + i;               // ties at the pivot: the first ones in position order
            ++o1;
        }
    }
}

// the final order of a long piece's survivors: one workgroup per query, (key, position) pairs in LDS
__global__ __launch_bounds__(kTopkSortThreads) void topk_batch_sort_kernel(TopkBatchArgs a) {
    const int q = blockIdx.x;
    if (a.bstart[q + 1] == a.bstart[q]) return;
    __shared__ uint64_t s_key[kTopkCap];
    __shared__ int32_t s_pos[kTopkCap];
    const int tid = threadIdx.x;
    int64_t t64 = a.total[2 * q] + a.total[2 * q + 1];
    if (t64 > a.k_max) t64 = a.k_max;
    if (t64 > kTopkCap) t64 = kTopkCap;
    const int total = (int)t64;
    if (total <= 0) {
        if (tid == 0) a.count[q] = 0;
        return;
    }
    const double* scores = a.scores + a.qoff[q];
    const int64_t n = a.m[q];
    const int64_t* cand = a.cand + (int64_t)q * a.k_max;
    const int P = pow2_at_least(total);
    for (int i = tid; i < P; i += kTopkSortThreads) {
        const int64_t r = i < total ? cand[i] : -1;
        const bool ok = r >= 0 && r < n;
        s_key[i] = ok ? order_key(scores[r]) : 0ull;
        s_pos[i] = ok ? (int32_t)r : INT_MAX;
    }
    __syncthreads();
    bitonic_sort_pairs(s_key, s_pos, P, tid, kTopkSortThreads);
    int64_t* out_rows = a.rows + (int64_t)q * a.k_max;
    double* out_vals = a.vals + (int64_t)q * a.k_max;
    for (int i = tid; i < total; i += kTopkSortThreads) {
        const int64_t r = s_pos[i];
        out_rows[i] = r;
        out_vals[i] = r < n ? scores[r] : 0.0;
    }
    if (tid == 0) a.count[q] = total;
}

}  // namespace

extern "C" {

int vq_db_batch_topk_layout(vq_db* db, int32_t n_queries, int64_t k_max, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = topk_shape(n_queries, k_max);
    if (rc != VQ_OK) return rc;
    topk_layout(n_queries, k_max, off);
    return VQ_OK;
}

int vq_db_batch_round_topk(vq_db* db, int32_t n_queries, int64_t k_max, void* block, int64_t block_bytes) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = topk_shape(n_queries, k_max);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries;
    int64_t off[6];
    topk_layout(Q, k_max, off);
    VQ_REQUIRE(block_bytes >= off[4], "the block of this batched top-k needs %lld bytes (vq_db_batch_topk_layout), got %lld", (long long)off[4],
               (long long)block_bytes);
    char* host = (char*)block;
    const int64_t* k = (const int64_t*)(host + off[0]);
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->round.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    // ---- every check, and the plan of the launches, on the host
    TopkBatchArgs a;
    a.bstart[0] = 0;
    bool any_served = false, any_short = false, all_served = true;
    int max_nb = 0;
    int64_t short_m = 0, long_m = 0;
    for (int q = 0; q < kTopkSlots; ++q) {
        const int64_t kq = q < Q ? k[q] : 0;
        VQ_REQUIRE(kq >= 0 && kq <= k_max, "query %d: k = %lld outside [0, k_max = %lld]", q, (long long)kq, (long long)k_max);
        if (kq > 0 && q >= db->round.q) return fail(VQ_E_STATE, "the last batched round had %d queries (k for query %d)", db->round.q, q);
        const int64_t m = kq > 0 ? db->round.m(q) : 0;
        if (m > INT_MAX) return fail(VQ_E_UNSUPPORTED, "query %d: a batched top-k ranks at most %d positions (got %lld)", q, INT_MAX, (long long)m);
        a.qoff[q] = db->round.start[q];
        a.m[q] = m;
        int nb = 0;
        if (kq > 0) {
            any_served = true;
            if (m <= kTopkSmallN && std::min(kq, m) <= kTopkSmallK) {
                any_short = true;
                short_m = std::max(short_m, m);
            } else {
                nb = (int)cdiv(m, SEL_CHUNK);
                long_m = std::max(long_m, m);
            }
        } else if (q < Q) {
            all_served = false;
        }
        max_nb = std::max(max_nb, nb);
        a.bstart[q + 1] = a.bstart[q] + nb;
    }
    if (!any_served) return VQ_OK;                        // every query skipped: nothing to launch
    DeviceGuard g(db->device);
    const int64_t cand_at = off[4], state_at = cand_at + up64((int64_t)kTopkSlots * k_max * 8), total_at = state_at + up64(9 * kTopkSlots * 2 * 8);
    const int64_t hist_at = total_at + up64(kTopkSlots * 2 * 8), cnt_at = hist_at + up64(8 * kTopkSlots * 256 * 4);
    VQ_HIP(db->btopk_buf.grow((size_t)(cnt_at + up64((int64_t)a.bstart[kTopkSlots] * 8))));
    char* base = db->btopk_buf;
    VQ_HIP(hipMemcpyAsync(base + off[0], host + off[0], (size_t)(off[1] - off[0]), hipMemcpyHostToDevice, db->stream));      // the k's
    a.scores = (const double*)(db->bround_dev + db->round.off[5]);
    a.k = (const int64_t*)(base + off[0]);
    a.count = (int64_t*)(base + off[1]);
    a.rows = (int64_t*)(base + off[2]);
    a.vals = (double*)(base + off[3]);
    a.k_max = k_max;
    a.cand = (int64_t*)(base + cand_at);
    a.state = (uint64_t*)(base + state_at);
    a.total = (int64_t*)(base + total_at);
    a.hist = (unsigned int*)(base + hist_at);
    a.blk_cnt = (int2*)(base + cnt_at);
    if (any_short) {
        auto kern = topk_batch_small_kernel;
        VQ_DYN_LDS(kern, (size_t)kTopkSmallN * 8);
        kern<<<Q, kTopkSmallThreads, (size_t)std::max<int64_t>(short_m, 1) * 8, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
    }
    if (max_nb > 0) {
        VQ_HIP(hipMemsetAsync(base + state_at, 0, (size_t)(cnt_at - state_at), db->stream));      // state | total | histograms
        const int bx = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(long_m, 2048), kTopkHistBlocks));
        for (int pass = 0; pass < 8; ++pass) {
            topk_batch_hist_kernel<<<dim3(bx, Q), 256, 0, db->stream>>>(a, pass);
            VQ_CHECK_LAUNCH();
        }
        topk_batch_count_kernel<<<dim3(max_nb, Q), SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
        topk_batch_scan_kernel<<<Q, SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
        topk_batch_scatter_kernel<<<dim3(max_nb, Q), SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
        topk_batch_sort_kernel<<<Q, kTopkSortThreads, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
    }
    if (all_served) {                                     // count | rows | vals: adjacent, one copy
        VQ_HIP(hipMemcpyAsync(host + off[1], base + off[1], (size_t)(off[4] - off[1]), hipMemcpyDeviceToHost, db->stream));
    } else {                                              // the entries of a skipped slot stay what the caller left there
        for (int q = 0; q < Q;) {
            if (k[q] == 0) {
                ++q;
                continue;
            }
            int e = q;
            while (e + 1 < Q && k[e + 1] > 0) ++e;
            const int64_t nq = e + 1 - q;
            VQ_HIP(hipMemcpyAsync(host + off[1] + q * 8, base + off[1] + q * 8, (size_t)(nq * 8), hipMemcpyDeviceToHost, db->stream));
            VQ_HIP(hipMemcpyAsync(host + off[2] + q * k_max * 8, base + off[2] + q * k_max * 8, (size_t)(nq * k_max * 8), hipMemcpyDeviceToHost, db->stream));
            VQ_HIP(hipMemcpyAsync(host + off[3] + q * k_max * 8, base + off[3] + q * k_max * 8, (size_t)(nq * k_max * 8), hipMemcpyDeviceToHost, db->stream));
            q = e + 1;
        }
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

}  // extern "C"
