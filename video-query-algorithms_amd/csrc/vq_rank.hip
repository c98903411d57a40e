// Ranking on a resident feature DB (the handle: csrc/vq_db.hip): scores again from the cached similarities, the weight grid, the
// stable partition of the scores, top-k.  Compiled with -ffp-contract=off like the scans: the score arithmetic rounds like the
// reference's numpy scalars.
//   src/models/ticket.py:165-180   compute_scores        -> score_from_avg (rescore_kernel)
//   src/models/ticket.py:311-356   select_clips_to_review-> select_* kernels (stable partition + near argmax)
//   src/models/ticket.py:266       final report ordering -> topk (radix select + stable compaction)
//   src/models/hyperparameter.py:57-58 40 rescorings     -> grid_kernel
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vq_db.h"
#include "vq_score.h"
#include "vq_select.h"

using namespace vq;

__global__ void rescore_kernel(const double* avg, const double* w, double* scores, int64_t n, int S) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    double av[8];
    for (int s = 0; s < S; ++s) av[s] = avg[c * S + s];
    scores[c] = score_from_avg(av, w, S);
}

// out[g][l] = score(rows[l]; w_grid[g])  (hyperparameter.py:57-58 restricted to labelled clips)
__global__ void grid_kernel(const double* avg, const double* w_grid, const int64_t* rows, double* out, int G, int L,
                            int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * L) return;
    const int g = i / L, l = i % L;
    double av[8], w[8];
    for (int s = 0; s < S; ++s) {
        av[s] = avg[rows[l] * S + s];
        w[s] = w_grid[g * S + s];
    }
    out[i] = score_from_avg(av, w, S);
}

// hyperparameter.py:57-64 in one launch: the 40 rescorings of the labelled rows AND the loss surface over the threshold grid.  Block g =
// grid weight g: its L scores (score_from_avg, as grid_kernel) go to LDS, then thread t walks the labels IN ORDER for threshold t:
//     surface[g][t] = 0.5 th[t] + sum_l (heaviside(score_l - th[t], 1) - y_l) * (score_l - th[t]) * (1 + y_l * ballast)
// -- the elementwise operations of the reference's numpy expression in its order (this file is compiled without contraction), one clip
// at a time in the dict's order: every cell sees the reference's sequence of fp64 operations (the division by L stays on the host).
__global__ void loss_surface_kernel(const double* avg, const double* w_grid, const int64_t* rows, const double* labels, const double* th_grid,
                                    double* out, int L, int T, int S, double ballast) {
    extern __shared__ double ls_scores[];                      // [L]
    const int g = blockIdx.x;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        double av[8], w[8];
        for (int s = 0; s < S; ++s) {
            av[s] = avg[rows[l] * S + s];
            w[s] = w_grid[g * S + s];
        }
        ls_scores[l] = score_from_avg(av, w, S);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const double th = th_grid[t];
        double surf = 0.5 * th;
        for (int l = 0; l < L; ++l) {
            const double y = labels[l];
            const double margin = ls_scores[l] - th;
            const double h = margin < 0.0 ? 0.0 : (margin >= 0.0 ? 1.0 : margin);     // np.heaviside(margin, 1); NaN stays NaN
            const double c = 1.0 + y * ballast;
            surf = surf + ((h - y) * margin) * c;
        }
        out[g * T + t] = surf;
    }
}

// ------------------------------------------------------------------------------------------------
// selection: stable partition of the score array (ticket.py:325-340)
// ------------------------------------------------------------------------------------------------
// SEL_ITEMS / SEL_BLOCK / SEL_CHUNK, order_key, the two predicates (SelPred), block_scan_excl2 and the blocks of the three passes and of
// the one-workgroup form (n <= kSelSmallN): csrc/vq_select.h.  The partitions of the batched rounds: csrc/vq_rounds.hip

__global__ __launch_bounds__(SEL_BLOCK) void select_count_kernel(const double* scores, int64_t n, SelPred pred,
                                                                  int2* blk_cnt, double* blk_max, int64_t* blk_arg) {
    select_count_block(scores, n, pred, blk_cnt, blk_max, blk_arg);
}

__global__ __launch_bounds__(SEL_BLOCK) void select_scan_kernel(int2* blk_cnt, const double* blk_max,
                                                                 const int64_t* blk_arg, int nblk, int64_t* result,
                                                                 int64_t limit1 /* cap on class-1 picks, <0 = none */) {
    select_scan_block(blk_cnt, blk_max, blk_arg, nblk, result, limit1);
}

__global__ __launch_bounds__(SEL_BLOCK) void select_scatter_kernel(const double* scores, int64_t n, SelPred pred,
                                                                    const int2* blk_off, int64_t* out0, int64_t* out1,
                                                                    int64_t limit1, int64_t* pre0, int64_t* pre1, int64_t prefix) {
    select_scatter_block(scores, n, pred, blk_off, out0, out1, limit1, pre0, pre1, prefix);
}

__global__ __launch_bounds__(kSelSmallThreads) void select_small_kernel(const double* scores, int n, SelPred pred, int64_t* result, int64_t* out0,
                                                                        int64_t* out1, int64_t* pre0, int64_t* pre1, int prefix) {
    select_small_block(scores, n, pred, result, out0, out1, pre0, pre1, prefix);
}

// ------------------------------------------------------------------------------------------------
// top-k: MSB-first radix select on the order-mapped scores, then the stable compaction above
// ------------------------------------------------------------------------------------------------
// state[0] = prefix (high bits fixed so far), state[1] = k still to find inside the prefix bucket
__global__ __launch_bounds__(256) void topk_hist_kernel(const double* scores, int64_t n, int pass,
                                                         const uint64_t* state, unsigned int* hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const uint64_t prefix = state[0];
    const uint64_t mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = order_key(scores[r]);
        if (k != 0ull && (k & mask) == prefix) atomicAdd(&h[(k >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void topk_pick_kernel(int pass, uint64_t* state, unsigned int* hist) {
    if (threadIdx.x != 0) return;
    const int shift = 56 - 8 * pass;
    uint64_t need = state[1];
    int b = 255;
    for (; b > 0; --b) {
        if (hist[b] >= need) break;
        need -= hist[b];
    }
    state[0] |= (uint64_t)b << shift;
    state[1] = need;
    for (int i = 0; i < 256; ++i) hist[i] = 0;
}

// The same selection for a SMALL database (n <= kTopkSmallN, k <= kTopkSmallK) as ONE launch of one workgroup: the order keys live in
// LDS, the eight histogram passes and the stable compaction are separated by barriers instead of 19 launches and three
// synchronisations (a 10k-clip top-20: ~0.15 ms of launch sequence -> one launch and one copy).  Same survivors in the same (row)
// order as the general path: keys above the pivot first, then the first `need` rows that tie with it.
// kTopkSmallN, kTopkSmallK, kTopkSmallThreads: csrc/vq_select.h (the batched top-k takes its short form at the same sizes)
__global__ __launch_bounds__(kTopkSmallThreads) void topk_small_kernel(const double* scores, int n, int k, int64_t* out_rows, double* out_vals,
                                                                       int64_t* out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(topk_lds);          // [n]
    __shared__ unsigned int hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ unsigned int s_need;
    __shared__ int2 s_wave[kTopkSmallThreads / 64];
    const int tid = threadIdx.x;
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
        // one atomic per wave for the lanes that agree with its first live lane (radix_hist_add, csrc/vq_select.h)
        for (int i0 = 0; i0 < n; i0 += kTopkSmallThreads) {
            const int i = i0 + tid;
            const uint64_t key = i < n ? keys[i] : 0ull;
            const bool live = key != 0ull && (key & mask) == prefix;
            radix_hist_add(hist, live, live ? (int)((key >> shift) & 255) : -1, tid & 63);
        }
        __syncthreads();
        if (tid < 64) radix_pick_wave(hist, tid, s_need, prefix, shift, &s_prefix, &s_need);      // topk_pick_kernel, by one wave
        __syncthreads();
    }
    const uint64_t pivot = s_prefix;
    const int need = (int)s_need;
    // stable compaction: a thread owns a run of consecutive rows
    const int per = (n + kTopkSmallThreads - 1) / kTopkSmallThreads;
    const int r0 = tid * per, r1 = min(n, r0 + per);
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
    const int n_gt = tot.x, n_eq = min(tot.y, need);
    for (int r = r0; r < r1; ++r) {
        const uint64_t key = keys[r];
        if (key > pivot) {
            out_rows[o0] = r;
            out_vals[o0] = scores[r];
            ++o0;
        } else if (key == pivot && key != 0ull) {
            if (o1 < need) {
                out_rows[n_gt + o1] = r;
                out_vals[n_gt + o1] = scores[r];
            }
            ++o1;
        }
    }
    if (tid == 0) out_count[0] = n_gt + n_eq;
}

__global__ void gather_scores_kernel(const double* scores, const int64_t* rows, int64_t cnt, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) out[i] = scores[rows[i]];
}

static int run_select(vq_db* db, const SelPred& pred, int64_t limit1, int64_t host_result[3], bool with_prefix = false) {
    const int64_t n = db->na;                            // the clips the scores cover: N, or the M of the row view in use
    const int nblk = (int)cdiv(n, SEL_CHUNK);
    if (n == 0) {                                        // an empty view: empty lists, no near-band maximum
        static const int64_t kEmpty[4] = {0, 0, -1, 0};
        VQ_HIP(hipMemcpyAsync(db->sel_result, kEmpty, 3 * 8, hipMemcpyHostToDevice, db->stream));
        if (host_result) memcpy(host_result, kEmpty, 3 * 8);
        return VQ_OK;
    }
    if (n <= kSelSmallN && limit1 < 0) {             // a small database: one launch
        select_small_kernel<<<1, kSelSmallThreads, 0, db->stream>>>(db->scores, (int)n, pred, db->sel_result, db->rows0, db->rows1, db->matchp,
                                                                    db->nearp, with_prefix ? (int)kRoundPrefix : 0);
        VQ_CHECK_LAUNCH();
        if (!host_result) return VQ_OK;
        VQ_HIP(hipMemcpyAsync(host_result, db->sel_result, 3 * 8, hipMemcpyDeviceToHost, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
        return VQ_OK;
    }
    select_count_kernel<<<nblk, SEL_BLOCK, 0, db->stream>>>(db->scores, n, pred, db->blk_cnt, db->blk_max,
                                                                 db->blk_arg);
    VQ_CHECK_LAUNCH();
    select_scan_kernel<<<1, SEL_BLOCK, 0, db->stream>>>(db->blk_cnt, db->blk_max, db->blk_arg, nblk, db->sel_result,
                                                         limit1);
    VQ_CHECK_LAUNCH();
    select_scatter_kernel<<<nblk, SEL_BLOCK, 0, db->stream>>>(db->scores, n, pred, db->blk_cnt, db->rows0,
                                                                   db->rows1, limit1, db->matchp, db->nearp, with_prefix ? kRoundPrefix : 0);
    VQ_CHECK_LAUNCH();
    if (!host_result) return VQ_OK;                  // vq_db_query_round: the counts travel with the round's block
    VQ_HIP(hipMemcpyAsync(host_result, db->sel_result, 3 * 8, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

// the partition by a threshold and a lower bound (vq_db_select, vq_db_select_rows, vq_db_query_round)
int vq::select_threshold(vq_db* db, double threshold, double lower, int64_t res[3], bool with_prefix) {
    SelPred pred;
    pred.mode = 0;
    pred.th = threshold;
    pred.lower = lower;
    pred.pivot = 0;
    return run_select(db, pred, -1, res, with_prefix);
}

int vq::launch_rescore(vq_db* db) {
    if (db->na) rescore_kernel<<<cdiv(db->na, 256), 256, 0, db->stream>>>(db->avg, db->w, db->scores, db->na, db->S);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

// the scores at L > 0 rows (positions of the view in use) to the host, through the handle's gather scratch; waited for
static int scores_at_rows(vq_db* db, const int64_t* rows_host, int L, double* out_host) {
    VQ_HIP(db->grid_buf.grow((size_t)L * 16));
    int64_t* rdev = (int64_t*)db->grid_buf.get();
    double* vdev = (double*)(db->grid_buf + (int64_t)L * 8);
    VQ_HIP(hipMemcpyAsync(rdev, rows_host, (size_t)L * 8, hipMemcpyHostToDevice, db->stream));
    gather_scores_kernel<<<cdiv(L, 256), 256, 0, db->stream>>>(db->scores, rdev, L, vdev);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(out_host, vdev, (size_t)L * 8, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

// final ordering of the tot survivors of a top-k: descending score, ties by ascending row (ticket.py:266)
static void order_survivors(const int64_t* rows, const double* vals, int64_t tot, int64_t* rows_out, double* vals_out) {
    std::vector<int64_t> order((size_t)tot);
    for (int64_t i = 0; i < tot; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        if (vals[x] != vals[y]) return vals[x] > vals[y];
        return rows[x] < rows[y];
    });
    for (int64_t i = 0; i < tot; ++i) {
        rows_out[i] = rows[order[i]];
        vals_out[i] = vals[order[i]];
    }
}

extern "C" {

int vq_db_rescore(vq_db* db, const double* w_host) {
    VQ_REQUIRE(db && w_host, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_avg) return fail(VQ_E_STATE, "vq_db_rescore: no similarities cached (call vq_db_scan first)");
    DeviceGuard g(db->device);
    VQ_HIP(hipMemcpyAsync(db->w, w_host, db->S * 8, hipMemcpyHostToDevice, db->stream));
    const int rc = launch_rescore(db);
    if (rc != VQ_OK) return rc;
    db->have_scores = true;
    return VQ_OK;
}

int vq_db_read_scores_at(vq_db* db, const int64_t* rows_host, int32_t L, double* out_host) {
    VQ_REQUIRE(db && out_host, "NULL argument");
    VQ_REQUIRE(L >= 0 && (L == 0 || rows_host), "bad rows");
    std::lock_guard<std::mutex> lk(db->mu);              // the bound is the view in use: read under the lock
    for (int l = 0; l < L; ++l)
        VQ_REQUIRE(rows_host[l] >= 0 && rows_host[l] < db->na, "rows[%d] = %lld outside [0,%lld)", l, (long long)rows_host[l], (long long)db->na);
    if (L == 0) return VQ_OK;
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed (scan with weights, or rescore)");
    DeviceGuard g(db->device);
    return scores_at_rows(db, rows_host, L, out_host);
}

int vq_db_scores_grid(vq_db* db, const double* w_grid_host, int32_t G, const int64_t* rows_host, int32_t L,
                      double* out_host) {
    VQ_REQUIRE(db && w_grid_host && rows_host && out_host, "NULL argument");
    VQ_REQUIRE(G > 0 && L > 0, "G and L must be positive");
    std::lock_guard<std::mutex> lk(db->mu);
    for (int l = 0; l < L; ++l)
        VQ_REQUIRE(rows_host[l] >= 0 && rows_host[l] < db->na, "rows[%d] = %lld outside [0,%lld)", l,
                   (long long)rows_host[l], (long long)db->na);
    if (!db->have_avg) return fail(VQ_E_STATE, "no similarities cached (call vq_db_scan first)");
    DeviceGuard g(db->device);
    const int64_t wb = (int64_t)G * db->S * 8, rb = (int64_t)L * 8, ob = (int64_t)G * L * 8;
    VQ_HIP(db->grid_buf.grow((size_t)(wb + rb + ob)));
    char* base = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(base, w_grid_host, wb, hipMemcpyHostToDevice, db->stream));
    VQ_HIP(hipMemcpyAsync(base + wb, rows_host, rb, hipMemcpyHostToDevice, db->stream));
    grid_kernel<<<cdiv((int64_t)G * L, 256), 256, 0, db->stream>>>(db->avg, (const double*)base, (const int64_t*)(base + wb),
                                                                    (double*)(base + wb + rb), G, L, db->S);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(out_host, base + wb + rb, ob, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_loss_surface(vq_db* db, const double* w_grid_host, int32_t G, const int64_t* rows_host, const double* labels_host, int32_t L,
                       const double* th_grid_host, int32_t T, double ballast, double* out_host) {
    VQ_REQUIRE(db && w_grid_host && rows_host && labels_host && th_grid_host && out_host, "NULL argument");
    VQ_REQUIRE(G > 0 && L > 0 && T > 0 && L <= 4096, "G, L, T must be positive (L <= 4096 labelled clips)");
    std::lock_guard<std::mutex> lk(db->mu);
    for (int l = 0; l < L; ++l)
        VQ_REQUIRE(rows_host[l] >= 0 && rows_host[l] < db->na, "rows[%d] = %lld outside [0,%lld)", l, (long long)rows_host[l], (long long)db->na);
    if (!db->have_avg) return fail(VQ_E_STATE, "no similarities cached (call vq_db_scan first)");
    DeviceGuard g(db->device);
    // one staging block: weights | rows | labels | thresholds in, the surface out
    const int64_t wb = (int64_t)G * db->S * 8, rb = (int64_t)L * 8, tb = (int64_t)T * 8, ob = (int64_t)G * T * 8;
    VQ_HIP(db->grid_buf.grow((size_t)(wb + 2 * rb + tb + ob)));
    std::vector<char> stage((size_t)(wb + 2 * rb + tb));
    memcpy(stage.data(), w_grid_host, (size_t)wb);
    memcpy(stage.data() + wb, rows_host, (size_t)rb);
    memcpy(stage.data() + wb + rb, labels_host, (size_t)rb);
    memcpy(stage.data() + wb + 2 * rb, th_grid_host, (size_t)tb);
    char* base = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(base, stage.data(), stage.size(), hipMemcpyHostToDevice, db->stream));      // pageable: staged before the call returns
    loss_surface_kernel<<<G, 64, (size_t)L * 8, db->stream>>>(db->avg, (const double*)base, (const int64_t*)(base + wb), (const double*)(base + wb + rb),
                                                               (const double*)(base + wb + 2 * rb), (double*)(base + wb + 2 * rb + tb), L, T, db->S, ballast);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(out_host, base + wb + 2 * rb + tb, ob, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_select(vq_db* db, double threshold, double lower, int64_t* n_match, int64_t* n_near, int64_t* near_argmax) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed (scan with weights, or rescore)");
    DeviceGuard g(db->device);
    int64_t res[3];
    const int rc = select_threshold(db, threshold, lower, res);
    if (rc != VQ_OK) return rc;
    db->last_n0 = res[0];
    db->last_n1 = res[1];
    if (n_match) *n_match = res[0];
    if (n_near) *n_near = res[1];
    if (near_argmax) *near_argmax = res[2];
    return VQ_OK;
}

static int fetch_selected(vq_db* db, int64_t* match_rows_host, int64_t cap_match, int64_t* near_rows_host, int64_t cap_near);

int vq_db_select_fetch(vq_db* db, int64_t* match_rows_host, int64_t cap_match, int64_t* near_rows_host, int64_t cap_near) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    return fetch_selected(db, match_rows_host, cap_match, near_rows_host, cap_near);
}

int vq_db_select_rows(vq_db* db, double threshold, double lower, int64_t* match_rows_host, int64_t cap_match,
                      int64_t* near_rows_host, int64_t cap_near, int64_t* n_match, int64_t* n_near, int64_t* near_argmax) {
    VQ_REQUIRE(db && match_rows_host && near_rows_host && n_match && n_near, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);          // partition and copy-out under ONE lock: no other thread's
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed (scan with weights, or rescore)");
    DeviceGuard g(db->device);                       // selection or top-k can slip in between
    int64_t res[3];
    const int rc = select_threshold(db, threshold, lower, res);
    if (rc != VQ_OK) return rc;
    db->last_n0 = res[0];
    db->last_n1 = res[1];
    *n_match = res[0];
    *n_near = res[1];
    if (near_argmax) *near_argmax = res[2];
    return fetch_selected(db, match_rows_host, cap_match, near_rows_host, cap_near);
}

static int fetch_selected(vq_db* db, int64_t* match_rows_host, int64_t cap_match, int64_t* near_rows_host, int64_t cap_near) {
    if (db->last_n0 < 0 || db->last_n1 < 0)
        return fail(VQ_E_STATE, "the selection lists were overwritten by a later top-k on this handle (select again)");
    DeviceGuard g(db->device);
    if (match_rows_host) {
        VQ_REQUIRE(cap_match >= db->last_n0, "match buffer too small (%lld < %lld)", (long long)cap_match, (long long)db->last_n0);
        if (db->last_n0) VQ_HIP(hipMemcpyAsync(match_rows_host, db->rows0, db->last_n0 * 8, hipMemcpyDeviceToHost, db->stream));
    }
    if (near_rows_host) {
        VQ_REQUIRE(cap_near >= db->last_n1, "near buffer too small (%lld < %lld)", (long long)cap_near, (long long)db->last_n1);
        if (db->last_n1) VQ_HIP(hipMemcpyAsync(near_rows_host, db->rows1, db->last_n1 * 8, hipMemcpyDeviceToHost, db->stream));
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_topk(vq_db* db, int64_t k, int64_t* rows_host, double* vals_host, int64_t* k_out) {
    VQ_REQUIRE(db && rows_host && vals_host && k_out, "NULL argument");
    VQ_REQUIRE(k > 0, "k must be positive");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed (scan with weights, or rescore)");
    DeviceGuard g(db->device);
    const int64_t n = db->na;                                        // the clips the scores cover (a row view: its M positions)
    if (n == 0) {
        *k_out = 0;
        return VQ_OK;
    }
    if (k > n) k = n;
    if (n <= kTopkSmallN && k <= kTopkSmallK) {                  // a small resident database: one launch, one copy back
        const int64_t bytes = 64 + k * 16;
        VQ_HIP(db->grid_buf.grow((size_t)bytes));
        char* base = db->grid_buf;
        auto kern = topk_small_kernel;
        const size_t lds = (size_t)n * 8;
        VQ_DYN_LDS(kern, (size_t)kTopkSmallN * 8);
        kern<<<1, kTopkSmallThreads, lds, db->stream>>>(db->scores, (int)n, (int)k, (int64_t*)(base + 64), (double*)(base + 64 + k * 8), (int64_t*)base);
        VQ_CHECK_LAUNCH();
        std::vector<char> host((size_t)bytes);
        VQ_HIP(hipMemcpyAsync(host.data(), base, (size_t)bytes, hipMemcpyDeviceToHost, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
        const int64_t tot = *(const int64_t*)host.data();
        VQ_REQUIRE(tot >= 0 && tot <= k, "internal: top-k produced %lld > k=%lld rows", (long long)tot, (long long)k);
        order_survivors((const int64_t*)(host.data() + 64), (const double*)(host.data() + 64 + k * 8), tot, rows_host, vals_host);
        *k_out = tot;
        return VQ_OK;
    }
    // radix select: find the key of the k-th largest score
    uint64_t st[2] = {0ull, (uint64_t)k};
    VQ_HIP(hipMemcpyAsync(db->tk_state, st, 16, hipMemcpyHostToDevice, db->stream));
    VQ_HIP(hipMemsetAsync(db->tk_hist, 0, 256 * 4, db->stream));
    const unsigned hgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)db->cus * 8));
    for (int pass = 0; pass < 8; ++pass) {
        topk_hist_kernel<<<hgrid, 256, 0, db->stream>>>(db->scores, n, pass, db->tk_state, db->tk_hist);
        VQ_CHECK_LAUNCH();
        topk_pick_kernel<<<1, 64, 0, db->stream>>>(pass, db->tk_state, db->tk_hist);
        VQ_CHECK_LAUNCH();
    }
    VQ_HIP(hipMemcpyAsync(st, db->tk_state, 16, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    // st[0] = key of the k-th largest (0 if fewer than k non-NaN scores), st[1] = how many equal to it are needed
    SelPred pred;
    pred.mode = 1;
    pred.th = pred.lower = 0.0;
    pred.pivot = st[0];
    int64_t res[3];
    db->last_n0 = db->last_n1 = -1;      // the shared row lists no longer hold a vq_db_select partition
    int rc = run_select(db, pred, (int64_t)st[1], res);
    if (rc != VQ_OK) return rc;
    const int64_t n_gt = res[0], n_eq = res[1];
    const int64_t tot = n_gt + n_eq;
    VQ_REQUIRE(tot <= k, "internal: top-k produced %lld > k=%lld rows", (long long)tot, (long long)k);
    VQ_HIP(db->grid_buf.grow((size_t)std::max<int64_t>(tot, 1) * 8));
    std::vector<int64_t> rows((size_t)tot);
    std::vector<double> vals((size_t)tot);
    if (n_gt) VQ_HIP(hipMemcpyAsync(rows.data(), db->rows0, n_gt * 8, hipMemcpyDeviceToHost, db->stream));
    if (n_eq) VQ_HIP(hipMemcpyAsync(rows.data() + n_gt, db->rows1, n_eq * 8, hipMemcpyDeviceToHost, db->stream));
    if (n_gt) {
        gather_scores_kernel<<<cdiv(n_gt, 256), 256, 0, db->stream>>>(db->scores, db->rows0, n_gt, (double*)db->grid_buf.get());
        VQ_CHECK_LAUNCH();
        VQ_HIP(hipMemcpyAsync(vals.data(), db->grid_buf, n_gt * 8, hipMemcpyDeviceToHost, db->stream));
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    if (n_eq) {
        gather_scores_kernel<<<cdiv(n_eq, 256), 256, 0, db->stream>>>(db->scores, db->rows1, n_eq, (double*)db->grid_buf.get());
        VQ_CHECK_LAUNCH();
        VQ_HIP(hipMemcpyAsync(vals.data() + n_gt, db->grid_buf, n_eq * 8, hipMemcpyDeviceToHost, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    order_survivors(rows.data(), vals.data(), tot, rows_host, vals_host);
    *k_out = tot;
    return VQ_OK;
}

int vq_db_min_score(vq_db* db, const int64_t* rows_host, int32_t L, double* min_out) {
    VQ_REQUIRE(db && min_out, "NULL argument");
    VQ_REQUIRE(L >= 0 && (L == 0 || rows_host), "bad rows");
    std::lock_guard<std::mutex> lk(db->mu);
    for (int l = 0; l < L; ++l)
        VQ_REQUIRE(rows_host[l] >= 0 && rows_host[l] < db->na, "rows[%d] outside the DB", l);
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed");
    DeviceGuard g(db->device);
    double m = 1.0;   // ticket.py:302 min_score = 1
    if (L > 0) {
        std::vector<double> v((size_t)L);
        const int rc = scores_at_rows(db, rows_host, L, v.data());
        if (rc != VQ_OK) return rc;
        for (int l = 0; l < L; ++l) m = std::min(m, v[l]);   // Python min(a, b): b if b < a else a
    }
    *min_out = m;
    return VQ_OK;
}

}  // extern "C"
