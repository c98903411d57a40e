// Batched query rounds on gfx950: up to 16 queries per pass over a resident feature database -- over the whole database
// (include/vq_amd_rounds.h), over a row view per query (include/vq_amd_round_views.h) -- and the weight fit and the re-weighting of
// such a round's queries on what it left on the device (include/vq_amd_round_fit.h), the scores of chosen rows of such a round
// under a grid of weights, which a row-sharded database combines into its fit (include/vq_amd_round_grid.h), and a group's whole
// weight update -- fit, pick, rescore, review bands, partition -- as one chain on the handle's stream (include/vq_amd_round_update.h),
// and the two calls a row-sharded database makes one operation of that update with: the avg of chosen rows, verbatim, and the same
// chain on avg tables that come with the block (include/vq_amd_round_shard.h).
//
// Every kind of round is described by ONE table of pieces (BatchRound, csrc/vq_db.h): query q owns the entries start[q] ..
// start[q + 1] of the concatenated avg / scores / list arrays.  A whole-database round is the round whose pieces all have N rows.
// The partition of the score pieces has one kernel family and one launcher (launch_partition) for every kind of round and for every
// run of queries that vq_db_batch_round_rescore partitions again.  The 16-query passes themselves are the scan kernels of
// csrc/vq_sim_batch.hip (vq::launch_round_pass, vq::launch_view_pass).
#include <algorithm>
#include <cstring>

#include "vq_db.h"
#include "vq_score.h"
#include "vq_select.h"

using namespace vq;

// ---- the partition of the score pieces of a round: query q partitions its piece scores[start[q] .. start[q + 1]) under its own
// band[q] = (threshold, lower) into positions of its piece, in its own rows of every output.  The blocks of csrc/vq_select.h,
// unchanged: per query the lists, counts and arg-max are those of the one-query launches on that piece.  The one-workgroup form for a
// piece of at most kSelSmallN entries, the three passes for a longer one, per query: a workgroup of the form its query does not take
// returns at once.
struct SelPieceArgs {
    const double* scores;     // the concatenated pieces
    const double* band;       // [Q][2]: threshold, lower
    int64_t* out0;            // match rows, the concatenated pieces
    int64_t* out1;            // near rows
    int2* blk_cnt;            // the blocks of the long pieces, query after query
    double* blk_max;
    int64_t* blk_arg;
    int64_t* result;          // [Q][4]: n_match, n_near, near_argmax, 0 (cleared by the host)
    int64_t* pre0;            // [Q][prefix]
    int64_t* pre1;            // [Q][prefix]
    int64_t prefix;
    int64_t start[17];
    int32_t bstart[17];       // the first block of query q (a short piece has none)
};

__device__ __forceinline__ SelPred batch_pred(const SelPieceArgs& a, int q) {
    SelPred pred;
    pred.mode = 0;
    pred.th = a.band[2 * q];
    pred.lower = a.band[2 * q + 1];
    pred.pivot = 0;
    return pred;
}

__global__ __launch_bounds__(kSelSmallThreads) void select_small_view_kernel(SelPieceArgs v) {
    const int q = blockIdx.x;
    const int64_t s0 = v.start[q], m = v.start[q + 1] - s0;
    if (m > kSelSmallN) return;
    select_small_block(v.scores + s0, (int)m, batch_pred(v, q), v.result + 4 * q, v.out0 + s0, v.out1 + s0, v.pre0 + q * v.prefix,
                       v.pre1 + q * v.prefix, (int)v.prefix);
}

__global__ __launch_bounds__(SEL_BLOCK) void select_count_view_kernel(SelPieceArgs v) {
    const int q = blockIdx.y, b0 = v.bstart[q];
    if ((int)blockIdx.x >= v.bstart[q + 1] - b0) return;
    select_count_block(v.scores + v.start[q], v.start[q + 1] - v.start[q], batch_pred(v, q), v.blk_cnt + b0, v.blk_max + b0, v.blk_arg + b0);
}

__global__ __launch_bounds__(SEL_BLOCK) void select_scan_view_kernel(SelPieceArgs v) {
    const int q = blockIdx.x, b0 = v.bstart[q], nb = v.bstart[q + 1] - b0;
    if (nb == 0) return;
    select_scan_block(v.blk_cnt + b0, v.blk_max + b0, v.blk_arg + b0, nb, v.result + 4 * q, -1);
}

__global__ __launch_bounds__(SEL_BLOCK) void select_scatter_view_kernel(SelPieceArgs v) {
    const int q = blockIdx.y, b0 = v.bstart[q];
    if ((int)blockIdx.x >= v.bstart[q + 1] - b0) return;
    const int64_t s0 = v.start[q];
    select_scatter_block(v.scores + s0, v.start[q + 1] - s0, batch_pred(v, q), v.blk_cnt + b0, v.out0 + s0, v.out1 + s0, -1,
                         v.pre0 + q * v.prefix, v.pre1 + q * v.prefix, v.prefix);
}

// n_e of a whole-database round: the splits present per (clip, stream) under the handle's mask -- the same for every query of the pass
__global__ __launch_bounds__(256) void batch_ne_kernel(const uint8_t* present, int32_t* ne, int64_t total /* n * S */, int E) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int c = E;
    if (present) {
        c = 0;
        for (int e = 0; e < E; ++e) c += present[i * E + e] != 0 ? 1 : 0;
    }
    ne[i] = c;
}

// ---- a batched round over one row view per query (vq_db_query_round_views, include/vq_amd_round_views.h) ---------------------------------
// THE PLAN, built on the device per call: inv[q][row] = the position of database row `row` in query q's view (-1: not a member),
// filled by scattering each view's resident row list; then the union of the views -- its rows (row-major databases) or the tiles it
// touches (tiled ones) -- by a stable compaction of "some query holds this row": count / scan / scatter, a thread per tile of 16 rows.
struct ViewPlanArgs {
    const int64_t* rows[16];  // the resident row list of query q's view; null: the whole database, or an empty view
    int64_t m[16];            // the rows of query q's piece (N for the whole database)
    int64_t start[17];        // the first entry of query q's piece; start[Q] = the sum of m
    int32_t Q;
    int64_t n, stride;        // the database's rows; the rows of inv per query (n rounded up to whole tiles)
    int32_t* inv;             // [16][stride]
    int64_t* start_dev;       // [17]: start, for the kernels that index it per lane
};

__global__ __launch_bounds__(256) void view_scatter_kernel(ViewPlanArgs a) {
    const int q = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.start_dev[q] = a.start[q];
        if (q == a.Q - 1) a.start_dev[a.Q] = a.start[a.Q];
    }
    const int64_t* rows = a.rows[q];
    if (!rows) return;
    const int64_t m = a.m[q];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        a.inv[(int64_t)q * a.stride + rows[i]] = (int32_t)i;
}

struct ViewUnionArgs {
    const int32_t* inv;       // [16][stride], stride % 16 == 0, -1 behind row n
    int64_t stride;
    int64_t ntiles;           // tiles of the database
    uint32_t members;         // bit q: query q has a row list scattered into inv
    int2* blk;                // [nblk]: per block of 256 tiles (union rows, touched tiles) -> their exclusive scan
    int nblk;
    int32_t* rows_out;        // the union's rows, ascending, padded to a multiple of 16 with the last one | null
    int32_t* tiles_out;       // the touched tiles, ascending | null
    int64_t* counts;          // [0] union rows, [1] touched tiles
};

// bit i: row 16 tile + i is in some view of the round
__device__ __forceinline__ unsigned view_union_flags(const ViewUnionArgs& a, int64_t tile) {
    unsigned f = 0;
    if (tile >= a.ntiles) return 0;
    for (int q = 0; q < kBatchSlots; ++q) {
        if (!((a.members >> q) & 1u)) continue;
        const int4* p = reinterpret_cast<const int4*>(a.inv + (int64_t)q * a.stride + tile * 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int4 v = p[g];
            f |= (v.x >= 0 ? 1u : 0u) << (4 * g) | (v.y >= 0 ? 2u : 0u) << (4 * g) | (v.z >= 0 ? 4u : 0u) << (4 * g) | (v.w >= 0 ? 8u : 0u) << (4 * g);
        }
    }
    return f;
}

__global__ __launch_bounds__(SEL_BLOCK) void view_union_count_kernel(ViewUnionArgs a) {
    const unsigned f = view_union_flags(a, (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x);
    int2 tot;
    block_scan_excl2(make_int2(__popc(f), f ? 1 : 0), &tot);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SEL_BLOCK) void view_union_scan_kernel(ViewUnionArgs a) {   // one workgroup
    __shared__ int2 carry;
    if (threadIdx.x == 0) carry = make_int2(0, 0);
    __syncthreads();
    for (int b0 = 0; b0 < a.nblk; b0 += SEL_BLOCK) {
        const int b = b0 + threadIdx.x;
        int2 tot;
        const int2 ex = block_scan_excl2(b < a.nblk ? a.blk[b] : make_int2(0, 0), &tot);
        const int2 c0 = carry;
        if (b < a.nblk) a.blk[b] = make_int2(c0.x + ex.x, c0.y + ex.y);
        __syncthreads();
        if (threadIdx.x == 0) carry = make_int2(c0.x + tot.x, c0.y + tot.y);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.counts[0] = carry.x;
        a.counts[1] = carry.y;
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void view_union_scatter_kernel(ViewUnionArgs a) {
    const int64_t tile = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const unsigned f = view_union_flags(a, tile);
    int2 tot;
    const int2 ex = block_scan_excl2(make_int2(__popc(f), f ? 1 : 0), &tot);
    int64_t o = (int64_t)a.blk[blockIdx.x].x + ex.x;
    if (a.tiles_out && f) a.tiles_out[(int64_t)a.blk[blockIdx.x].y + ex.y] = (int32_t)tile;
    if (a.rows_out && f) {
        int32_t last = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((f >> i) & 1u) a.rows_out[o++] = last = (int32_t)(tile * 16 + i);
        const int64_t total = a.counts[0];                    // written by the scan launch before this one
        if (o == total)                                       // the thread that holds the union's last row pads the last virtual tile with it
            for (int64_t k = total; k < (total + 15) / 16 * 16; ++k) a.rows_out[k] = last;
    }
}

// n_e per query: the splits present per (position of the view, stream), read by database row
__global__ __launch_bounds__(256) void view_ne_kernel(ViewPlanArgs a, const uint8_t* present, int32_t* ne, int S, int E) {
    const int q = blockIdx.y;
    const int64_t* rows = a.rows[q];
    const int64_t total = a.m[q] * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pos = i / S;
        const int s = (int)(i - pos * S);
        int c = E;
        if (present) {
            const int64_t row = rows ? rows[pos] : pos;
            c = 0;
            for (int e = 0; e < E; ++e) c += present[(row * S + s) * E + e] != 0 ? 1 : 0;
        }
        ne[(a.start[q] + pos) * S + s] = c;
    }
}

// ---- the weight fit and the rescore of vq_db_loss_surface / vq_db_rescore (csrc/vq_rank.hip) for the queries of a batched round, on the
// avg that round left on the device (include/vq_amd_round_fit.h) ----
// loss_surface_kernel for every query with labels in ONE launch: block (g, q) = grid weight g of query q, over the avg entries of that
// query (qoff[q] on).  The labels walk through LDS in chunks of kFitChunk: all threads fill the chunk's scores, then thread t adds the
// chunk's terms to its running sum for threshold t IN LABEL ORDER -- the chunking changes nothing in a cell's sequence of fp64
// operations, so a cell has loss_surface_kernel's bits on the same avg, for any number of labels in 32 KB of LDS.
constexpr int kFitChunk = 4096, kFitThreads = 256, kFitMaxGrid = 64;
struct FitBatchArgs {
    const double* avg;        // the round's avg piece: [Q][N][S], or the concatenated pieces of a view round | a given table [sum L][S]
    const double* w_grid;     // [Q][G][8]
    const double* th_grid;    // [Q][T]
    const double* ballast;    // [Q]
    const int64_t* rows;      // [sum L]: positions inside each query's piece | null: label l of query q is entry l of its piece (a given table)
    const double* labels;     // [sum L]
    double* out;              // [Q][G][T]
    int64_t qoff[16];         // the first avg entry of query q (a given table: lstart[q])
    int64_t lstart[17];       // the first label of query q (lstart[q + 1] - lstart[q] = L_q; 0: nothing to do)
    int G, T, S;
};

__global__ __launch_bounds__(kFitThreads) void loss_surface_batch_kernel(FitBatchArgs a) {
    __shared__ double ls_scores[kFitChunk];
    const int g = blockIdx.x, q = blockIdx.y, S = a.S;
    const int64_t l0 = a.lstart[q], L = a.lstart[q + 1] - l0;
    if (L <= 0) return;                                        // the whole workgroup: a skipped query writes nothing
    double w[8];
    for (int s = 0; s < S; ++s) w[s] = a.w_grid[((int64_t)q * a.G + g) * 8 + s];
    const int t = threadIdx.x;
    const bool mine = t < a.T;                                 // T <= kFitMaxGrid < kFitThreads: one thread per threshold
    const double th = mine ? a.th_grid[q * a.T + t] : 0.0;
    const double ballast = a.ballast[q];
    const double* avg = a.avg + a.qoff[q] * S;
    double surf = 0.5 * th;
    for (int64_t c0 = 0; c0 < L; c0 += kFitChunk) {
        const int len = (int)(L - c0 < kFitChunk ? L - c0 : kFitChunk);
        for (int l = threadIdx.x; l < len; l += kFitThreads) {
            double av[8];
            const int64_t row = a.rows ? a.rows[l0 + c0 + l] : c0 + l;
            for (int s = 0; s < S; ++s) av[s] = avg[row * S + s];
            ls_scores[l] = score_from_avg(av, w, S);
        }
        __syncthreads();
        if (mine) {
            for (int l = 0; l < len; ++l) {
                const double y = a.labels[l0 + c0 + l];
                const double margin = ls_scores[l] - th;
                const double h = margin < 0.0 ? 0.0 : (margin >= 0.0 ? 1.0 : margin);     // np.heaviside(margin, 1); NaN stays NaN
                const double c = 1.0 + y * ballast;
                surf = surf + ((h - y) * margin) * c;
            }
        }
        __syncthreads();                                       // the next chunk overwrites the scores
    }
    if (mine) a.out[((int64_t)q * a.G + g) * a.T + t] = surf;
}

// rescore_kernel for the masked queries of a batched round: query q = blockIdx.y rescores its m[q] avg entries under w[q] into the
// round's own score array; a query outside the mask is left alone.
struct RescoreBatchArgs {
    const double* avg;
    const double* w;          // [16][8]
    double* scores;
    int64_t qoff[16];         // the first avg / score entry of query q
    int64_t m[16];
    uint32_t mask;
    int S;
};

__global__ __launch_bounds__(256) void rescore_batch_kernel(RescoreBatchArgs a) {
    const int q = blockIdx.y, S = a.S;
    if (!((a.mask >> q) & 1u)) return;
    double w[8];
    for (int s = 0; s < S; ++s) w[s] = a.w[q * 8 + s];
    const int64_t m = a.m[q], base = a.qoff[q];
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < m; c += (int64_t)gridDim.x * blockDim.x) {
        double av[8];
        for (int s = 0; s < S; ++s) av[s] = a.avg[(base + c) * S + s];
        a.scores[base + c] = score_from_avg(av, w, S);
    }
}

// ---- the two steps between those kernels that vq_db_batch_round_update keeps on the device (include/vq_amd_round_update.h) ----
// What both read and write of the update block's image, and the weights | bands staged behind it for the rescore and the partition.
constexpr int kPickThreads = 256;
struct UpdateBatchArgs {
    const double* surface;    // [Q][G][T]: raw sums
    const double* w_grid;     // [Q][G][8]
    const double* th_grid;    // [Q][T]
    const int64_t* L;         // [Q]: the divisor; 0: the slot is skipped
    const int32_t* second;    // [Q]
    const double* eps;        // [Q]
    const int32_t* band_mode; // [Q]
    const double* near;       // [Q]
    const int64_t* user_rows; // [sum U]: positions inside each query's piece
    const double* user_avg;   // null: a user row's score is read from `scores` | [sum U][S]: it is score_from_avg of this entry under w[q]
    const double* scores;     // the round's score pieces
    double* pick;             // [Q][8]
    int32_t* pick_idx;        // [Q][4]
    double* w;                // [16][8]: what rescore_batch_kernel reads
    double* band;             // [16][2]: what the partition reads
    int64_t qoff[16];         // the first score entry of query q
    int64_t ustart[17];       // the first user row of query q
    int G, T, S;
};

// is cell (a, i) in front of cell (b, j) in numpy.argmin's order: a NaN before every number, then the smaller value, then the smaller
// flat index (a < b is false for +-0 and for equal infinities: the index decides)
__device__ __forceinline__ bool pick_before(double a, int i, double b, int j) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (an) return i < j;
    return a < b || (a == b && i < j);
}

// hyperparameter.py:23-29 with the squares as products: vertex and curvature of the parabola through three points of one axis
__device__ __forceinline__ void parabola_through(double lo, double mid, double hi, double y_lo, double y_mid, double y_hi, double* vertex, double* curve) {
    const double rise = y_hi - y_lo, fall_hi = y_mid - y_hi, fall_lo = y_mid - y_lo;
    const double v = 0.5 * (rise * (mid * mid) + fall_hi * (lo * lo) - fall_lo * (hi * hi)) / (rise * mid + fall_hi * lo - fall_lo * hi);
    *vertex = v;
    *curve = fall_lo / ((mid - v) * (mid - v) - (lo - v) * (lo - v));
}

// hyperparameter.py:66-114 behind the arg-min: the grid values of cell (iw, it) on the rim of the grid, else the minimum of the
// separable parabola through the cell and its four neighbours, clamped to the neighbouring grid lines, or the cell itself when the
// five points are not reproduced.  surf: the query's raw cells, divided by `div` as they are read; wg [G][8] with the grid in column
// `second`.  Operation for operation Hyperparameter._pick_exact (the unit is compiled without contraction).
struct PickedCell {
    double w_best, th_best;
    bool on_rim, fell_back;
};

__device__ __forceinline__ PickedCell refine_cell(const double* surf, double div, const double* wg, const double* ths, int G, int T, int iw, int it,
                                                  int second) {
    PickedCell out;
    out.on_rim = iw == 0 || iw == G - 1 || it == 0 || it == T - 1;
    out.fell_back = false;
    out.w_best = wg[iw * 8 + second];
    out.th_best = ths[it];
    if (out.on_rim) return out;
    const double ws0 = wg[(iw - 1) * 8 + second], ws1 = out.w_best, ws2 = wg[(iw + 1) * 8 + second];
    const double th0g = ths[it - 1], th1g = out.th_best, th2g = ths[it + 1];
    const double centre = surf[iw * T + it] / div;
    const double west = surf[(iw - 1) * T + it] / div, east = surf[(iw + 1) * T + it] / div;
    const double south = surf[iw * T + it - 1] / div, north = surf[iw * T + it + 1] / div;
    double w0, ca, th0, cb;
    parabola_through(ws0, ws1, ws2, west, centre, east, &w0, &ca);
    parabola_through(th0g, th1g, th2g, south, centre, north, &th0, &cb);
    const double c = centre - ca * ((ws1 - w0) * (ws1 - w0)) - cb * ((th1g - th0) * (th1g - th0));
    w0 = ws2 < w0 ? ws2 : w0;                                  // max(min(w0, ws[2]), ws[0]) as Python evaluates it: a NaN stays
    w0 = ws0 > w0 ? ws0 : w0;
    th0 = th2g < th0 ? th2g : th0;
    th0 = th0g > th0 ? th0g : th0;
    auto model = [&](double w, double th) { return ca * ((w - w0) * (w - w0)) + cb * ((th - th0) * (th - th0)) + c; };
    const double misfit = fabs(west - model(ws0, th1g)) + fabs(south - model(ws1, th0g)) + fabs(centre - model(ws1, th1g)) +
                          fabs(north - model(ws1, th2g)) + fabs(east - model(ws2, th1g));
    out.fell_back = misfit > 1e-6;                             // FIT_TOLERANCE; false for a NaN misfit
    if (!out.fell_back) {
        out.w_best = w0;
        out.th_best = th0;
    }
    return out;
}

// Hyperparameter._pick_exact for every slot with labels: one workgroup per query.  All threads divide the cells by L and reduce
// (value, flat index) in LDS to numpy.argmin's cell; thread 0 then refines it and writes the pick, the query's weight row and its
// threshold.
__global__ __launch_bounds__(kPickThreads) void pick_refine_batch_kernel(UpdateBatchArgs a) {
    __shared__ double ls_val[kPickThreads];
    __shared__ int ls_idx[kPickThreads];
    const int q = blockIdx.x, G = a.G, T = a.T, t = threadIdx.x;
    const int64_t L = a.L[q];
    if (L <= 0) return;                                        // the whole workgroup
    const double div = (double)L;
    const double* surf = a.surface + (int64_t)q * G * T;
    double best = 0.0;
    int best_i = 0x7fffffff;                                   // no cell yet: every cell comes in front of it
    for (int i = t; i < G * T; i += kPickThreads) {
        const double v = surf[i] / div;                        // IEEE division first: it can create the ties the order then resolves
        if (best_i == 0x7fffffff || pick_before(v, i, best, best_i)) {
            best = v;
            best_i = i;
        }
    }
    ls_val[t] = best;
    ls_idx[t] = best_i;
    __syncthreads();
    for (int s = kPickThreads / 2; s > 0; s >>= 1) {
        if (t < s && ls_idx[t + s] != 0x7fffffff && (ls_idx[t] == 0x7fffffff || pick_before(ls_val[t + s], ls_idx[t + s], ls_val[t], ls_idx[t]))) {
            ls_val[t] = ls_val[t + s];
            ls_idx[t] = ls_idx[t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const int iw = ls_idx[0] / T, it = ls_idx[0] - iw * T, second = a.second[q];
    const double* wg = a.w_grid + (int64_t)q * G * 8;
    const PickedCell cell = refine_cell(surf, div, wg, a.th_grid + (int64_t)q * T, G, T, iw, it, second);
    const double w_best = cell.w_best, th_best = cell.th_best;
    const bool on_rim = cell.on_rim, fell_back = cell.fell_back;
    const double threshold = th_best - a.eps[q];
    for (int s = 0; s < 8; ++s) a.w[q * 8 + s] = s == second ? w_best : wg[iw * 8 + s];
    a.band[2 * q] = threshold;
    double* pick = a.pick + q * 8;
    pick[0] = w_best;
    pick[1] = threshold;
    pick[3] = threshold;
    pick[5] = pick[6] = pick[7] = 0.0;
    int32_t* idx = a.pick_idx + q * 4;
    idx[0] = iw;
    idx[1] = it;
    idx[2] = (on_rim ? 1 : 0) | (fell_back ? 2 : 0);
    idx[3] = 0;
}

// compute_matches.py:78-88 and ticket.py:301-316 behind the rescore: one workgroup per query.  Mode 1 lowers 1.0 by the scores at the
// query's user rows; thread t folds a contiguous run of them and the tree joins neighbouring runs, the earlier one on the left, so
// the value is the in-order fold's (also between +0 and -0).  Thread 0 then writes the band.  With user_avg (the rows may live on
// another handle: include/vq_amd_round_shard.h) a row's score is what rescore_batch_kernel gives at it, from the same avg and weights.
__global__ __launch_bounds__(kPickThreads) void review_band_batch_kernel(UpdateBatchArgs a) {
    __shared__ double ls_min[kPickThreads];
    const int q = blockIdx.x, t = threadIdx.x;
    if (a.L[q] <= 0) return;                                   // the whole workgroup
    const bool from_user = a.band_mode[q] == 1;
    double lowest = 1.0;
    if (from_user) {
        const int64_t u0 = a.ustart[q], U = a.ustart[q + 1] - u0, per = (U + kPickThreads - 1) / kPickThreads;
        const double* scores = a.scores + a.qoff[q];
        const int64_t hi = (t + 1) * per < U ? (t + 1) * per : U;
        double w[8];
        if (a.user_avg)
            for (int s = 0; s < a.S; ++s) w[s] = a.w[q * 8 + s];
        for (int64_t i = t * per; i < hi; ++i) {
            double v;
            if (a.user_avg) {
                double av[8];
                for (int s = 0; s < a.S; ++s) av[s] = a.user_avg[(u0 + i) * a.S + s];
                v = score_from_avg(av, w, a.S);
            } else {
                v = scores[a.user_rows[u0 + i]];
            }
            lowest = v < lowest ? v : lowest;                  // min(min_score, v)
        }
        ls_min[t] = lowest;
        __syncthreads();
        for (int s = 1; s < kPickThreads; s <<= 1) {
            if (t % (2 * s) == 0) ls_min[t] = ls_min[t + s] < ls_min[t] ? ls_min[t + s] : ls_min[t];
            __syncthreads();
        }
        lowest = ls_min[0];
    }
    if (t != 0) return;
    const double th = a.band[2 * q];
    double reach = a.near[q];
    if (from_user) {
        const double below = th - lowest, room = 1.0 - th, eps = a.eps[q];
        reach = (0.0 > below ? 0.0 : below) / (eps > room ? eps : room);                      // max(th - lowest, 0) / max(1 - th, eps)
    }
    const double lower = th - reach * (1.0 - th);
    a.band[2 * q + 1] = lower;
    a.pick[q * 8 + 2] = lowest;
    a.pick[q * 8 + 4] = lower;
}

// grid_kernel (csrc/vq_rank.hip) for the queries of a batched round: thread (q = blockIdx.y, i = g L_q + l) scores row rows[l] of query
// q's avg piece (qoff[q] on) under w_grid[q][g] into the query's [G][L_q] piece of `out`, which starts at entry G lstart[q].  A query
// without rows has no thread that passes the bound.
struct GridBatchArgs {
    const double* avg;        // the round's avg piece: [Q][N][S], or the concatenated pieces of a view round
    const double* w_grid;     // [Q][G][8]
    const int64_t* rows;      // [sum L]: positions inside each query's piece
    double* out;              // [G sum L]
    int64_t qoff[16];         // the first avg entry of query q
    int64_t lstart[17];       // the first row of query q (lstart[q + 1] - lstart[q] = L_q; 0: nothing to do)
    int G, S;
};

__global__ __launch_bounds__(256) void grid_scores_batch_kernel(GridBatchArgs a) {
    const int q = blockIdx.y;
    const int64_t l0 = a.lstart[q], L = a.lstart[q + 1] - l0;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.G * L) return;
    const int64_t g = i / L, l = i - g * L;
    const int64_t entry = a.qoff[q] + a.rows[l0 + l];
    a.out[(int64_t)a.G * l0 + i] = score_from_avg(a.avg + entry * a.S, a.w_grid + ((int64_t)q * a.G + g) * 8, a.S);
}

// vq_db_batch_round_avg_rows (include/vq_amd_round_shard.h): thread (q = blockIdx.y, i = l S + s) copies stream s of row rows[l] of query
// q's avg piece (qoff[q] on) into entry lstart[q] + l of `out`.  Loads and stores only: the bits arrive as they are.
struct AvgRowsArgs {
    const double* avg;        // the round's avg piece: [Q][N][S], or the concatenated pieces of a view round
    const int64_t* rows;      // [sum L]: positions inside each query's piece
    double* out;              // [sum L][S]
    int64_t qoff[16];         // the first avg entry of query q
    int64_t lstart[17];       // the first row of query q (lstart[q + 1] - lstart[q] = L_q; 0: nothing to do)
    int S;
};

__global__ __launch_bounds__(256) void avg_rows_batch_kernel(AvgRowsArgs a) {
    const int q = blockIdx.y, S = a.S;
    const int64_t l0 = a.lstart[q], total = (a.lstart[q + 1] - l0) * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = i / S;
        const int s = (int)(i - l * S);
        a.out[(l0 + l) * S + s] = a.avg[(a.qoff[q] + a.rows[l0 + l]) * S + s];
    }
}

// ---- the host steps that every round takes, each stated once ---------------------------------------------------------------------------
// The round of Q queries whose pieces hold m[q] entries.  off[0..11] is what the two layout calls hand out: the nine pieces of the
// host block, each rounded up to 64 bytes, off[9] = their bytes, off[10] = the prefix length, off[11] = 0 or the sum of m.  A view
// round holds n_e once per piece, a whole-database round (m[q] = N) once per database.  Behind the image of the host block, on the
// device only: the two full lists, then blk_cnt | blk_max | blk_arg of the long pieces.
static void fill_round(BatchRound& r, const vq_db* db, int Q, const int64_t* m, bool views) {
    r = BatchRound();
    r.q = Q;
    r.views = views;
    for (int q = 0; q < kBatchSlots; ++q) {
        const int64_t mq = q < Q ? m[q] : 0;
        r.start[q + 1] = r.start[q] + mq;
        r.bstart[q + 1] = r.bstart[q] + (mq > kSelSmallN ? cdiv(mq, SEL_CHUNK) : 0);
    }
    const int64_t sm = r.start[Q], nbt = r.bstart[Q];
    int64_t* off = r.off;
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * db->S * db->E * db->D * 8);
    off[2] = off[1] + up64((int64_t)Q * 8 * 8);
    off[3] = off[2] + up64((int64_t)Q * 2 * 8);
    off[4] = off[3] + up64((views ? sm : m[0]) * db->S * 4);
    off[5] = off[4] + up64(sm * db->S * 8);
    off[6] = off[5] + up64(sm * 8);
    off[7] = off[6] + up64((int64_t)Q * 4 * 8);
    off[8] = off[7] + up64((int64_t)Q * kRoundPrefix * 8);
    off[9] = off[8] + up64((int64_t)Q * kRoundPrefix * 8);
    off[10] = kRoundPrefix;
    off[11] = views ? sm : 0;
    r.rows0 = off[9];
    r.rows1 = r.rows0 + up64(sm * 8);
    r.cnt = r.rows1 + up64(sm * 8);
    r.max = r.cnt + nbt * 8;
    r.arg = r.max + nbt * 8;
    r.need = r.arg + nbt * 8 + 64;
}

// the checks of the two round entry points that need no lock
static int check_round_call(const vq_db* db, int n_queries, int flags, bool views) {
    VQ_REQUIRE(n_queries >= 1 && n_queries <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, n_queries);
    VQ_REQUIRE(db->D % 256 == 0 && db->D <= 1024, "a batched round needs D in {256,512,768,1024} (got %d)", db->D);
    VQ_REQUIRE(db->S <= 8, "at most 8 streams");
    if (views) VQ_REQUIRE(db->n < (int64_t)2147483647 - 16, "a view round indexes the database's rows with 32 bits (%lld rows)", (long long)db->n);
    VQ_REQUIRE((flags & ~15) == 0, "flags: 1 = avg and n_e back, 2 = scores back, 4 = partition, 8 = timed (got %d)", flags);
    return VQ_OK;
}

// the device block of round r and, for a timed round, the four events; what the block held is gone when it had to grow
static int ensure_round_block(vq_db* db, const BatchRound& r, bool timed) {
    const char* dev = db->bround_dev;
    if (db->bround_dev.bytes < (size_t)r.need && dev && (char*)db->batch_scores >= dev && (char*)db->batch_scores < dev + db->bround_dev.bytes) {
        db->batch_scores = nullptr;                   // the scores of the round before lived in the block that goes
        db->batch_q = 0;
    }
    VQ_HIP(db->bround_dev.grow((size_t)r.need));
    if (timed && !db->bround_ev[0])
        for (Event& ev : db->bround_ev) VQ_HIP(ev.create());
    return VQ_OK;
}

// The partition of the score pieces of queries q0 .. q1 of round r in the handle's block, under the bands d_band [q1 - q0 + 1][2] (on
// the device): their result rows cleared, the one-workgroup form if a piece of the run is short, count / scan / scatter if one is
// long.  The run's queries are the kernels' queries 0 .. q1 - q0.
static int launch_partition(vq_db* db, const BatchRound& r, int q0, int q1, const double* d_band) {
    char* dev = db->bround_dev;
    const int nq = q1 - q0 + 1;
    const int64_t P = r.off[10];
    SelPieceArgs a;
    for (int i = 0; i <= kBatchSlots; ++i) {
        const int q = std::min(q0 + i, kBatchSlots);
        a.start[i] = r.start[q];
        a.bstart[i] = r.bstart[q];
    }
    bool any_small = false;
    int max_nb = 0;
    for (int q = q0; q <= q1; ++q) {
        any_small |= r.m(q) <= kSelSmallN;
        max_nb = std::max(max_nb, r.bstart[q + 1] - r.bstart[q]);
    }
    a.scores = (const double*)(dev + r.off[5]);
    a.band = d_band;
    a.blk_cnt = (int2*)(dev + r.cnt);
    a.blk_max = (double*)(dev + r.max);
    a.blk_arg = (int64_t*)(dev + r.arg);
    a.result = (int64_t*)(dev + r.off[6]) + 4 * q0;
    a.out0 = (int64_t*)(dev + r.rows0);
    a.out1 = (int64_t*)(dev + r.rows1);
    a.pre0 = (int64_t*)(dev + r.off[7]) + q0 * P;
    a.pre1 = (int64_t*)(dev + r.off[8]) + q0 * P;
    a.prefix = P;
    VQ_HIP(hipMemsetAsync(dev + r.off[6] + (int64_t)q0 * 32, 0, (size_t)nq * 32, db->stream));
    if (any_small) {                                  // the pieces of at most kSelSmallN entries (an empty one: 0, 0, -1)
        select_small_view_kernel<<<nq, kSelSmallThreads, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
    }
    if (max_nb > 0) {                                 // count / scan / scatter for the longer ones, the query on blockIdx.y
        select_count_view_kernel<<<dim3(max_nb, nq), SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
        select_scan_view_kernel<<<nq, SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
        select_scatter_view_kernel<<<dim3(max_nb, nq), SEL_BLOCK, 0, db->stream>>>(a);
        VQ_CHECK_LAUNCH();
    }
    return VQ_OK;
}

// rescore_batch_kernel for the queries of `mask` in round r under the weights d_w [16][8] (on the device); max_m: their longest piece
static int launch_rescore(vq_db* db, const BatchRound& r, uint32_t mask, int64_t max_m, const double* d_w) {
    RescoreBatchArgs a;
    a.avg = (const double*)(db->bround_dev + r.off[4]);
    a.w = d_w;
    a.scores = (double*)(db->bround_dev + r.off[5]);
    for (int q = 0; q < kBatchSlots; ++q) {
        a.qoff[q] = r.start[q];
        a.m[q] = r.m(q);
    }
    a.mask = mask;
    a.S = db->S;
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>((max_m + 255) / 256, (int64_t)db->cus * 8));
    rescore_batch_kernel<<<dim3(bx, r.q), 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

// Per run [q0, q1] of adjacent queries of `mask` in round r: its partition under the bands d_band [16][2] (on the device), then the
// run's scores, results and prefixes into the round's host block in adjacent copies.  What vq_db_batch_round_rescore and
// vq_db_batch_round_update do behind their rescore launch.
static int partition_runs(vq_db* db, const BatchRound& r, uint32_t mask, const double* d_band, char* host, bool want_scores, bool do_select) {
    const int Q = r.q;
    const int64_t* off = r.off;
    const int64_t P = off[10];
    char* dev = db->bround_dev;
    auto in_mask = [&](int q) { return q < Q && ((mask >> q) & 1u); };
    for (int q0 = 0; q0 < Q;) {
        if (!in_mask(q0)) {
            ++q0;
            continue;
        }
        int q1 = q0;
        while (in_mask(q1 + 1)) ++q1;
        const int nq = q1 - q0 + 1;
        if (do_select) {
            const int rc = launch_partition(db, r, q0, q1, d_band + 2 * q0);
            if (rc != VQ_OK) return rc;
        }
        const int64_t s_lo = r.start[q0] * 8, s_len = r.start[q1 + 1] * 8 - s_lo;
        if (want_scores && s_len) VQ_HIP(hipMemcpyAsync(host + off[5] + s_lo, dev + off[5] + s_lo, (size_t)s_len, hipMemcpyDeviceToHost, db->stream));
        if (do_select) {
            VQ_HIP(hipMemcpyAsync(host + off[6] + (int64_t)q0 * 32, dev + off[6] + (int64_t)q0 * 32, (size_t)nq * 32, hipMemcpyDeviceToHost, db->stream));
            for (int piece = 7; piece <= 8; ++piece)
                VQ_HIP(hipMemcpyAsync(host + off[piece] + q0 * P * 8, dev + off[piece] + q0 * P * 8, (size_t)(nq * P * 8), hipMemcpyDeviceToHost, db->stream));
        }
        q0 = q1 + 1;
    }
    return VQ_OK;
}

// the handle's counts of the queries of `mask` from the result rows that came back (after the synchronisation)
static void adopt_counts(BatchRound& r, const char* host, uint32_t mask) {
    const int64_t* res = (const int64_t*)(host + r.off[6]);
    for (int q = 0; q < r.q; ++q)
        if ((mask >> q) & 1u) {
            r.n0[q] = res[4 * q];
            r.n1[q] = res[4 * q + 1];
        }
}

// back: n_e | avg, scores, results | prefixes -- the pieces asked for, adjacent ones in one copy
static int copy_round_back(vq_db* db, const BatchRound& r, char* host, bool want_avg, bool want_scores, bool do_select) {
    const int64_t* off = r.off;
    const int64_t piece[3][2] = {{off[3], off[5]}, {off[5], off[6]}, {off[6], off[9]}};
    const bool want[3] = {want_avg, want_scores, do_select};
    for (int i = 0; i < 3;) {
        if (!want[i]) {
            ++i;
            continue;
        }
        int j = i;
        while (j + 1 < 3 && want[j + 1]) ++j;
        VQ_HIP(hipMemcpyAsync(host + piece[i][0], db->bround_dev + piece[i][0], (size_t)(piece[j][1] - piece[i][0]), hipMemcpyDeviceToHost, db->stream));
        i = j + 1;
    }
    return VQ_OK;
}

// the results of the queries of `mask` when every piece among them is empty: nothing was launched for them
static void empty_results(BatchRound& r, char* host, uint32_t mask) {
    int64_t* res = (int64_t*)(host + r.off[6]);
    for (int q = 0; q < r.q; ++q)
        if ((mask >> q) & 1u) {
            res[4 * q] = res[4 * q + 1] = res[4 * q + 3] = 0;
            res[4 * q + 2] = -1;
            r.n0[q] = r.n1[q] = 0;
        }
}

// the round becomes the handle's last one, with the counts of the result rows `res` (null: it did not partition)
static void record_round(vq_db* db, BatchRound& r, const int64_t* res) {
    for (int q = 0; q < kBatchSlots; ++q) {
        r.n0[q] = res && q < r.q ? res[4 * q] : -1;
        r.n1[q] = res && q < r.q ? res[4 * q + 1] : -1;
    }
    db->round = r;
}

// m[q]: the rows of query q's piece.  Caller holds the lock.
static int view_round_sizes(vq_db* db, int Q, const int32_t* views, int64_t m[16]) {
    for (int q = 0; q < Q; ++q) {
        const int32_t v = views[q];
        if (v == -1) m[q] = db->n;
        else if (v < 0 || (size_t)v >= db->views.size() || !db->views[v].defined)
            return fail(VQ_E_INVALID, "query %d: no row view %d on this handle", q, v);
        else m[q] = db->views[v].m;
    }
    return VQ_OK;
}

// row_bytes: what a labelled row brings in piece 4 -- its position (8), or its S averaged similarities (a given table)
static void batch_fit_layout(int Q, int G, int T, int64_t n_labels, int64_t off[8], int64_t row_bytes = 8) {
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * G * 8 * 8);
    off[2] = off[1] + up64((int64_t)Q * T * 8);
    off[3] = off[2] + up64((int64_t)Q * 8);
    off[4] = off[3] + up64((int64_t)Q * 8);
    off[5] = off[4] + up64(n_labels * row_bytes);
    off[6] = off[5] + up64(n_labels * 8);
    off[7] = off[6] + up64((int64_t)Q * G * T * 8);
}

static int batch_fit_shape(int Q, int G, int T, int64_t n_labels) {
    VQ_REQUIRE(Q >= 1 && Q <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, Q);
    VQ_REQUIRE(G >= 1 && G <= kFitMaxGrid && T >= 1 && T <= kFitMaxGrid, "the grids of a batched fit hold 1 to %d weights and thresholds (got %d, %d)",
               kFitMaxGrid, G, T);
    VQ_REQUIRE(n_labels >= 0, "n_labels must not be negative");
    return VQ_OK;
}

// the fit block's pieces (off[0] .. off[6] are batch_fit_layout's), then the update's own inputs and its two outputs; row_bytes: of a
// labelled row and of a user row alike
static void batch_update_layout(int Q, int G, int T, int64_t n_labels, int64_t n_user_rows, int64_t off[16], int64_t row_bytes = 8) {
    batch_fit_layout(Q, G, T, n_labels, off, row_bytes);
    off[8] = off[7] + up64((int64_t)Q * 4);
    off[9] = off[8] + up64((int64_t)Q * 8);
    off[10] = off[9] + up64((int64_t)Q * 4);
    off[11] = off[10] + up64((int64_t)Q * 8);
    off[12] = off[11] + up64((int64_t)Q * 8);
    off[13] = off[12] + up64(n_user_rows * row_bytes);
    off[14] = off[13] + up64((int64_t)Q * 8 * 8);
    off[15] = off[14] + up64((int64_t)Q * 4 * 4);
}

static void batch_grid_layout(int Q, int G, int64_t n_rows, int64_t off[5]) {
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * G * 8 * 8);
    off[2] = off[1] + up64((int64_t)Q * 8);
    off[3] = off[2] + up64(n_rows * 8);
    off[4] = off[3] + up64((int64_t)G * n_rows * 8);
}

static void batch_avg_rows_layout(int Q, int S, int64_t n_rows, int64_t off[4]) {
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * 8);
    off[2] = off[1] + up64(n_rows * 8);
    off[3] = off[2] + up64(n_rows * S * 8);
}

static int batch_grid_shape(int Q, int G, int64_t n_rows) {
    VQ_REQUIRE(Q >= 1 && Q <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, Q);
    VQ_REQUIRE(G >= 1 && G <= kFitMaxGrid, "the grid of a batched round holds 1 to %d weights (got %d)", kFitMaxGrid, G);
    // 2^32 rows x 64 weights are 2^30 workgroups of 256: the launch's grid stays inside 31 bits
    VQ_REQUIRE(n_rows >= 0 && n_rows <= ((int64_t)1 << 32), "n_rows must be in [0, 2^32] (got %lld)", (long long)n_rows);
    return VQ_OK;
}

// The row lists of a call that reads chosen rows of round r (vq_db_batch_round_grid, vq_db_batch_round_avg_rows), checked: every L_q in
// [0, n_rows] and their sum n_rows, no rows for a slot the round lacked, every row inside its query's piece.  Gives the first row of
// every slot, the first avg entry of every query and the longest list.  Caller holds the lock and has seen that a round exists.
static int chosen_rows(const BatchRound& r, int Q, const int64_t* L, const int64_t* rows, int64_t n_rows, int64_t lstart[17], int64_t qoff[16],
                       int64_t* max_l) {
    lstart[0] = 0;
    *max_l = 0;
    for (int q = 0; q < kBatchSlots; ++q) {
        const int64_t lq = q < Q ? L[q] : 0;
        VQ_REQUIRE(lq >= 0 && lq <= n_rows, "query %d: L = %lld outside [0, n_rows = %lld]", q, (long long)lq, (long long)n_rows);
        if (lq > 0 && q >= r.q) return fail(VQ_E_STATE, "the last batched round had %d queries (rows for query %d)", r.q, q);
        lstart[q + 1] = lstart[q] + lq;
        qoff[q] = r.start[q];
        *max_l = std::max(*max_l, lq);
    }
    VQ_REQUIRE(lstart[kBatchSlots] == n_rows, "the L of the queries add up to %lld, n_rows is %lld", (long long)lstart[kBatchSlots], (long long)n_rows);
    for (int q = 0; q < Q; ++q)
        for (int64_t l = lstart[q]; l < lstart[q + 1]; ++l)
            VQ_REQUIRE(rows[l] >= 0 && rows[l] < r.m(q), "query %d: row %lld (entry %lld) outside [0,%lld)", q, (long long)rows[l],
                       (long long)(l - lstart[q]), (long long)r.m(q));
    return VQ_OK;
}

extern "C" {

// ---- batched rounds over the whole database (include/vq_amd_rounds.h) ----------------------------------------------------------------
int vq_db_batch_round_layout(vq_db* db, int32_t n_queries, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    VQ_REQUIRE(n_queries >= 1 && n_queries <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, n_queries);
    int64_t m[16];
    std::fill(m, m + 16, db->n);
    BatchRound r;
    fill_round(r, db, n_queries, m, false);
    memcpy(off, r.off, sizeof(r.off));
    return VQ_OK;
}

int vq_db_query_round_batch(vq_db* db, int32_t n_queries, void* block, int64_t block_bytes, int32_t flags) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = check_round_call(db, n_queries, flags, false);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries;
    int64_t m[16];
    std::fill(m, m + 16, db->n);
    BatchRound r;
    fill_round(r, db, Q, m, false);
    const int64_t* off = r.off;
    VQ_REQUIRE(block_bytes >= off[9], "the block of a batched round of %d queries needs %lld bytes (vq_db_batch_round_layout), got %lld", Q,
               (long long)off[9], (long long)block_bytes);
    const bool want_avg = flags & 1, want_scores = flags & 2, do_select = flags & 4, timed = flags & 8;
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->active >= 0)
        return fail(VQ_E_UNSUPPORTED, "vq_db_query_round_batch runs over the whole database: row view %d is in use (vq_db_rows_use(db, -1) first)", db->active);
    DeviceGuard g(db->device);
    const int64_t n = db->n;
    db->round.q = 0;                                  // the lists of the round before are gone from here on
    {
        const int rc = ensure_round_block(db, r, timed);
        if (rc != VQ_OK) return rc;
    }
    db->round.timed = false;
    char* host = (char*)block;
    char* dev = db->bround_dev;
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[0], db->stream));
    VQ_HIP(hipMemcpyAsync(dev, host, (size_t)off[3], hipMemcpyHostToDevice, db->stream));       // queries | weights | bands: adjacent
    double* d_scores = (double*)(dev + off[5]);
    {
        const int rc = launch_round_pass(db, Q, (const double*)(dev + off[0]), (const double*)(dev + off[1]), d_scores, (double*)(dev + off[4]));
        if (rc != VQ_OK) return rc;
    }
    db->batch_scores = d_scores;                      // vq_db_batch_scores_devptr: the scores of the last batched pass
    db->batch_q = Q;
    batch_ne_kernel<<<cdiv(n * db->S, 256), 256, 0, db->stream>>>(db->present, (int32_t*)(dev + off[3]), n * db->S, db->E);
    VQ_CHECK_LAUNCH();
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[1], db->stream));
    if (do_select) {
        const int rc = launch_partition(db, r, 0, Q - 1, (const double*)(dev + off[2]));
        if (rc != VQ_OK) return rc;
    }
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[2], db->stream));
    {
        const int rc = copy_round_back(db, r, host, want_avg, want_scores, do_select);
        if (rc != VQ_OK) return rc;
    }
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[3], db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    r.timed = timed;
    record_round(db, r, do_select ? (const int64_t*)(host + off[6]) : nullptr);
    return VQ_OK;
}

int vq_db_batch_round_fetch(vq_db* db, int32_t query, int64_t* match_rows_host, int64_t cap_match, int64_t* near_rows_host, int64_t cap_near) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    const BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    if (query < 0 || query >= r.q) return fail(VQ_E_STATE, "the last batched round had %d queries (asked for query %d)", r.q, query);
    const int64_t n0 = r.n0[query], n1 = r.n1[query];
    if (n0 < 0 || n1 < 0) return fail(VQ_E_STATE, "the last batched round did not partition (flag 4)");
    DeviceGuard g(db->device);
    if (match_rows_host) {
        VQ_REQUIRE(cap_match >= n0, "match buffer too small (%lld < %lld)", (long long)cap_match, (long long)n0);
        if (n0) VQ_HIP(hipMemcpyAsync(match_rows_host, db->bround_dev + r.rows0 + r.start[query] * 8, (size_t)n0 * 8, hipMemcpyDeviceToHost, db->stream));
    }
    if (near_rows_host) {
        VQ_REQUIRE(cap_near >= n1, "near buffer too small (%lld < %lld)", (long long)cap_near, (long long)n1);
        if (n1) VQ_HIP(hipMemcpyAsync(near_rows_host, db->bround_dev + r.rows1 + r.start[query] * 8, (size_t)n1 * 8, hipMemcpyDeviceToHost, db->stream));
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_batch_round_times(vq_db* db, float* ms) {
    VQ_REQUIRE(db && ms, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->round.timed) return fail(VQ_E_STATE, "the last batched round was not timed (flag 8)");
    for (int i = 0; i < 3; ++i) VQ_HIP(hipEventElapsedTime(&ms[i], db->bround_ev[i], db->bround_ev[i + 1]));
    return VQ_OK;
}

// ---- batched rounds over a row view per query (include/vq_amd_round_views.h) ---------------------------------------------------------
int vq_db_view_round_layout(vq_db* db, int32_t n_queries, const int32_t* views_host, int64_t* off, int64_t* start) {
    VQ_REQUIRE(db && views_host && off && start, "NULL argument");
    VQ_REQUIRE(n_queries >= 1 && n_queries <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, n_queries);
    std::lock_guard<std::mutex> lk(db->mu);
    int64_t m[16];
    const int rc = view_round_sizes(db, n_queries, views_host, m);
    if (rc != VQ_OK) return rc;
    BatchRound r;
    fill_round(r, db, n_queries, m, true);
    memcpy(off, r.off, sizeof(r.off));
    memcpy(start, r.start, sizeof(r.start));
    return VQ_OK;
}

int vq_db_query_round_views(vq_db* db, int32_t n_queries, const int32_t* views_host, void* block, int64_t block_bytes, int32_t flags) {
    VQ_REQUIRE(db && views_host && block, "NULL argument");
    {
        const int rc = check_round_call(db, n_queries, flags, true);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries;
    const bool want_avg = flags & 1, want_scores = flags & 2, do_select = flags & 4, timed = flags & 8;
    std::lock_guard<std::mutex> lk(db->mu);
    int64_t m[16];
    {
        const int rc = view_round_sizes(db, Q, views_host, m);
        if (rc != VQ_OK) return rc;
    }
    BatchRound r;
    fill_round(r, db, Q, m, true);
    const int64_t* off = r.off;
    const int64_t* start = r.start;
    VQ_REQUIRE(block_bytes >= off[9], "the block of this view round of %d queries needs %lld bytes (vq_db_view_round_layout), got %lld", Q,
               (long long)off[9], (long long)block_bytes);
    DeviceGuard g(db->device);
    const int64_t n = db->n, sm = start[Q];
    const bool tiled = db->tiled();
    uint32_t whole = 0, members = 0;                  // queries over the whole database | queries whose row list goes into the plan
    int64_t member_rows = 0, max_m = 0;
    for (int q = 0; q < Q; ++q) {
        if (views_host[q] < 0) whole |= 1u << q;
        else if (m[q] > 0) {
            members |= 1u << q;
            member_rows += m[q];
        }
        max_m = std::max(max_m, m[q]);
    }
    db->round.q = 0;                                  // the lists of the round before are gone from here on
    db->batch_scores = nullptr;                       // vq_db_batch_scores_devptr names [Q][N] scores: none until the next whole-database pass
    db->batch_q = 0;
    db->round.timed = false;
    db->vround_have = false;
    char* host = (char*)block;
    if (sm == 0) {                                    // every view is empty: nothing to launch
        record_round(db, r, nullptr);
        if (do_select) empty_results(db->round, host, (1u << Q) - 1);
        db->vround_have = true;
        db->vround_union = db->vround_tiles = 0;
        return VQ_OK;
    }
    {
        const int rc = ensure_round_block(db, r, timed);
        if (rc != VQ_OK) return rc;
    }
    // the plan's block (vq_db.h): 64 MB of inverse map at 16 x 1M rows, allocated on the first view round
    const int64_t stride = (n + 15) / 16 * 16, db_tiles = stride / 16;
    const int nblk_u = cdiv(db_tiles, SEL_BLOCK);
    const int64_t p_rows = (int64_t)kBatchSlots * stride * 4, p_tiles = p_rows + up64((stride + 16) * 4), p_counts = p_tiles + up64(db_tiles * 4);
    const int64_t p_start = p_counts + 64, p_blk = p_start + up64(17 * 8), p_need = p_blk + (int64_t)nblk_u * 8 + 64;
    VQ_HIP(db->vround_plan.grow((size_t)p_need));
    char* plan = db->vround_plan;
    char* dev = db->bround_dev;
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[0], db->stream));
    VQ_HIP(hipMemcpyAsync(dev, host, (size_t)off[3], hipMemcpyHostToDevice, db->stream));       // queries | weights | bands: adjacent
    // the plan
    ViewPlanArgs pa;
    for (int q = 0; q < kBatchSlots; ++q) {
        pa.rows[q] = (members >> q) & 1u ? db->views[views_host[q]].rows.get() : nullptr;
        pa.m[q] = r.m(q);
        pa.start[q] = start[q];
    }
    pa.start[kBatchSlots] = start[kBatchSlots];
    pa.Q = Q;
    pa.n = n;
    pa.stride = stride;
    pa.inv = (int32_t*)plan;
    pa.start_dev = (int64_t*)(plan + p_start);
    for (int q = 0; q < Q; ++q)
        if ((members >> q) & 1u) VQ_HIP(hipMemsetAsync(plan + (int64_t)q * stride * 4, 0xFF, (size_t)stride * 4, db->stream));
    const int fill_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((max_m + 255) / 256, (int64_t)db->cus * 8));
    view_scatter_kernel<<<dim3(fill_blocks, Q), 256, 0, db->stream>>>(pa);
    VQ_CHECK_LAUNCH();
    int64_t max_tiles = db_tiles;                     // a whole-database query: the union is the database, addressed as ever
    if (!whole) {
        ViewUnionArgs ua;
        ua.inv = pa.inv;
        ua.stride = stride;
        ua.ntiles = db_tiles;
        ua.members = members;
        ua.blk = (int2*)(plan + p_blk);
        ua.nblk = nblk_u;
        ua.rows_out = tiled ? nullptr : (int32_t*)(plan + p_rows);
        ua.tiles_out = tiled ? (int32_t*)(plan + p_tiles) : nullptr;
        ua.counts = (int64_t*)(plan + p_counts);
        view_union_count_kernel<<<nblk_u, SEL_BLOCK, 0, db->stream>>>(ua);
        VQ_CHECK_LAUNCH();
        view_union_scan_kernel<<<1, SEL_BLOCK, 0, db->stream>>>(ua);
        VQ_CHECK_LAUNCH();
        view_union_scatter_kernel<<<nblk_u, SEL_BLOCK, 0, db->stream>>>(ua);
        VQ_CHECK_LAUNCH();
        max_tiles = tiled ? std::min(db_tiles, member_rows) : (std::min(n, member_rows) + 15) / 16;
    }
    {
        BatchViewArgs f;
        f.feats = db->feats;
        f.t = (const double*)(dev + off[0]);
        f.w = (const double*)(dev + off[1]);
        f.present = db->present;
        f.scores = (double*)(dev + off[5]);
        f.n = n;
        f.Q = Q;
        f.S = db->S;
        f.E = db->E;
        f.D = db->D;
        f.avg = (double*)(dev + off[4]);
        f.items = whole ? nullptr : (tiled ? (const int32_t*)(plan + p_tiles) : (const int32_t*)(plan + p_rows));
        f.counts = (const int64_t*)(plan + p_counts);
        f.inv = pa.inv;
        f.inv_stride = stride;
        f.start = pa.start_dev;
        f.whole = whole;
        f.members = members;
        const int rc = launch_view_pass(db, f, max_tiles);
        if (rc != VQ_OK) return rc;
    }
    view_ne_kernel<<<dim3((int)std::max<int64_t>(1, std::min<int64_t>((max_m * db->S + 255) / 256, (int64_t)db->cus * 8)), Q), 256, 0, db->stream>>>(
        pa, db->present, (int32_t*)(dev + off[3]), db->S, db->E);
    VQ_CHECK_LAUNCH();
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[1], db->stream));
    if (do_select) {
        const int rc = launch_partition(db, r, 0, Q - 1, (const double*)(dev + off[2]));
        if (rc != VQ_OK) return rc;
    }
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[2], db->stream));
    {
        const int rc = copy_round_back(db, r, host, want_avg, want_scores, do_select);
        if (rc != VQ_OK) return rc;
    }
    int64_t counts[2] = {n, db_tiles};
    if (!whole) VQ_HIP(hipMemcpyAsync(counts, plan + p_counts, 16, hipMemcpyDeviceToHost, db->stream));
    if (timed) VQ_HIP(hipEventRecord(db->bround_ev[3], db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    r.timed = timed;
    record_round(db, r, do_select ? (const int64_t*)(host + off[6]) : nullptr);
    db->vround_have = true;
    db->vround_union = counts[0];
    db->vround_tiles = counts[1];
    return VQ_OK;
}

int vq_db_view_round_union(vq_db* db, int64_t* n_union, int64_t* n_tiles) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->vround_have) return fail(VQ_E_STATE, "no view round has run on this handle");
    if (n_union) *n_union = db->vround_union;
    if (n_tiles) *n_tiles = db->vround_tiles;
    return VQ_OK;
}

// ---- the weight fit and the re-weighting of a batched round's queries (include/vq_amd_round_fit.h) -----------------------------------
int vq_db_batch_fit_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = batch_fit_shape(n_queries, n_grid, n_thresholds, n_labels);
    if (rc != VQ_OK) return rc;
    batch_fit_layout(n_queries, n_grid, n_thresholds, n_labels, off);
    return VQ_OK;
}

int vq_db_batch_round_fit(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, void* block, int64_t block_bytes) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = batch_fit_shape(n_queries, n_grid, n_thresholds, n_labels);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries, G = n_grid, T = n_thresholds;
    int64_t off[8];
    batch_fit_layout(Q, G, T, n_labels, off);
    VQ_REQUIRE(block_bytes >= off[7], "the block of this batched fit needs %lld bytes (vq_db_batch_fit_layout), got %lld", (long long)off[7],
               (long long)block_bytes);
    char* host = (char*)block;
    const int64_t* L = (const int64_t*)(host + off[3]);
    const int64_t* rows = (const int64_t*)(host + off[4]);
    std::lock_guard<std::mutex> lk(db->mu);
    const BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    FitBatchArgs a;
    a.lstart[0] = 0;
    for (int q = 0; q < kBatchSlots; ++q) {
        const int64_t lq = q < Q ? L[q] : 0;
        VQ_REQUIRE(lq >= 0 && lq <= n_labels, "query %d: L = %lld outside [0, n_labels = %lld]", q, (long long)lq, (long long)n_labels);
        if (lq > 0 && q >= r.q) return fail(VQ_E_STATE, "the last batched round had %d queries (labels for query %d)", r.q, q);
        a.lstart[q + 1] = a.lstart[q] + lq;
        a.qoff[q] = r.start[q];
    }
    VQ_REQUIRE(a.lstart[kBatchSlots] == n_labels, "the L of the queries add up to %lld, n_labels is %lld", (long long)a.lstart[kBatchSlots], (long long)n_labels);
    for (int q = 0; q < Q; ++q)
        for (int64_t l = a.lstart[q]; l < a.lstart[q + 1]; ++l)
            VQ_REQUIRE(rows[l] >= 0 && rows[l] < r.m(q), "query %d: row %lld (label %lld) outside [0,%lld)", q, (long long)rows[l],
                       (long long)(l - a.lstart[q]), (long long)r.m(q));
    if (n_labels == 0) return VQ_OK;                  // every query skipped: nothing to launch
    DeviceGuard g(db->device);
    VQ_HIP(db->grid_buf.grow((size_t)off[7]));
    char* base = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(base, host, (size_t)off[6], hipMemcpyHostToDevice, db->stream));      // grids | ballast | L | rows | labels: adjacent
    a.avg = (const double*)(db->bround_dev + r.off[4]);
    a.w_grid = (const double*)(base + off[0]);
    a.th_grid = (const double*)(base + off[1]);
    a.ballast = (const double*)(base + off[2]);
    a.rows = (const int64_t*)(base + off[4]);
    a.labels = (const double*)(base + off[5]);
    a.out = (double*)(base + off[6]);
    a.G = G;
    a.T = T;
    a.S = db->S;
    loss_surface_batch_kernel<<<dim3(G, Q), kFitThreads, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    const int64_t cell = (int64_t)G * T * 8;
    for (int q = 0; q < Q;) {                         // the surfaces of the queries served, adjacent ones in one copy
        if (L[q] == 0) {
            ++q;
            continue;
        }
        int e = q;
        while (e + 1 < Q && L[e + 1] > 0) ++e;
        VQ_HIP(hipMemcpyAsync(host + off[6] + q * cell, base + off[6] + q * cell, (size_t)((e + 1 - q) * cell), hipMemcpyDeviceToHost, db->stream));
        q = e + 1;
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_batch_round_rescore(vq_db* db, int32_t mask, void* block, int64_t block_bytes, int32_t flags) {
    VQ_REQUIRE(db && block, "NULL argument");
    VQ_REQUIRE((flags & ~(VQ_BROUND_SCORES | VQ_BROUND_SELECT)) == 0, "flags: 2 = scores back, 4 = partition (got %d)", flags);
    VQ_REQUIRE(mask > 0 && mask < (1 << kBatchSlots), "mask: bit q = query q of the round, at least one of %d (got %d)", kBatchSlots, mask);
    const bool want_scores = flags & VQ_BROUND_SCORES, do_select = flags & VQ_BROUND_SELECT;
    std::lock_guard<std::mutex> lk(db->mu);
    BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    const int Q = r.q;
    if (mask >> Q) return fail(VQ_E_STATE, "the last batched round had %d queries (mask 0x%x)", Q, mask);
    const int64_t* off = r.off;
    VQ_REQUIRE(block_bytes >= off[9], "the block of the last batched round needs %lld bytes, got %lld", (long long)off[9], (long long)block_bytes);
    char* host = (char*)block;
    auto in_mask = [&](int q) { return q < Q && ((mask >> q) & 1); };
    int64_t max_m = 0;
    for (int q = 0; q < Q; ++q)
        if (in_mask(q)) max_m = std::max(max_m, r.m(q));
    if (max_m == 0) {                                 // only empty views: nothing to launch
        if (do_select) empty_results(r, host, (uint32_t)mask);
        return VQ_OK;
    }
    DeviceGuard g(db->device);
    const int64_t up_bytes = off[3] - off[1];         // weights | bands of the round's block: adjacent
    VQ_HIP(db->grid_buf.grow((size_t)up_bytes));
    // staged beside the round's image, whose weights and bands of the other queries stay what the round saw
    char* stage = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(stage, host + off[1], (size_t)up_bytes, hipMemcpyHostToDevice, db->stream));
    const double* d_band = (const double*)(stage + (off[2] - off[1]));
    {
        const int rc = launch_rescore(db, r, (uint32_t)mask, max_m, (const double*)stage);
        if (rc != VQ_OK) return rc;
    }
    {
        const int rc = partition_runs(db, r, (uint32_t)mask, d_band, host, want_scores, do_select);
        if (rc != VQ_OK) return rc;
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    if (do_select) adopt_counts(r, host, (uint32_t)mask);
    return VQ_OK;
}

// ---- a group's whole weight update on a batched round in one call (include/vq_amd_round_update.h) ------------------------------------
int vq_db_batch_update_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = batch_fit_shape(n_queries, n_grid, n_thresholds, n_labels);
    if (rc != VQ_OK) return rc;
    VQ_REQUIRE(n_user_rows >= 0, "n_user_rows must not be negative");
    batch_update_layout(n_queries, n_grid, n_thresholds, n_labels, n_user_rows, off);
    return VQ_OK;
}

// A group's whole weight update on the last batched round, stated once for its two entry points.  tables = false:
// vq_db_batch_round_update (include/vq_amd_round_update.h), the labelled and the user rows named by position.  tables = true:
// vq_db_batch_round_update_given (include/vq_amd_round_shard.h): pieces 4 and 12 of the block carry those rows' avg instead, S doubles
// per row, so there are no positions to check, the surface is never given and L_q counts labels that other handles may hold.
static int run_batch_update(vq_db* db, bool tables, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                            void* update_block, int64_t update_bytes, void* round_block, int64_t round_bytes, int32_t flags) {
    VQ_REQUIRE(db && update_block, "NULL argument");
    {
        const int rc = batch_fit_shape(n_queries, n_grid, n_thresholds, n_labels);
        if (rc != VQ_OK) return rc;
    }
    VQ_REQUIRE(n_user_rows >= 0, "n_user_rows must not be negative");
    if (tables) {
        constexpr int kKnown = VQ_BROUND_SCORES | VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE;
        VQ_REQUIRE((flags & ~kKnown) == 0, "flags: 2 = scores back, 4 = partition, 16 = surfaces back (got %d)", flags);
    } else {
        constexpr int kKnown = VQ_BROUND_SCORES | VQ_BROUND_SELECT | VQ_BUPDATE_SURFACE | VQ_BUPDATE_GIVEN_SURFACE;
        VQ_REQUIRE((flags & ~kKnown) == 0, "flags: 2 = scores back, 4 = partition, 16 = surfaces back, 32 = surfaces given (got %d)", flags);
    }
    const bool want_scores = flags & VQ_BROUND_SCORES, do_select = flags & VQ_BROUND_SELECT;
    const bool want_surface = flags & VQ_BUPDATE_SURFACE, given = flags & VQ_BUPDATE_GIVEN_SURFACE;
    VQ_REQUIRE(!(want_surface && given), "flags: a given surface (32) is not copied back (16)");
    VQ_REQUIRE(round_block || !(want_scores || do_select), "NULL argument: scores and partitions come back into the block of the round");
    const int Q = n_queries, G = n_grid, T = n_thresholds;
    int64_t off[16];
    batch_update_layout(Q, G, T, n_labels, n_user_rows, off, tables ? (int64_t)db->S * 8 : 8);
    VQ_REQUIRE(update_bytes >= off[15], "the block of this batched update needs %lld bytes (%s), got %lld", (long long)off[15],
               tables ? "vq_db_batch_update_given_layout" : "vq_db_batch_update_layout", (long long)update_bytes);
    char* host = (char*)update_block;
    const int64_t* L = (const int64_t*)(host + off[3]);
    const int64_t* rows = (const int64_t*)(host + off[4]);
    const int32_t* second = (const int32_t*)(host + off[7]);
    const int32_t* band_mode = (const int32_t*)(host + off[9]);
    const int64_t* U = (const int64_t*)(host + off[11]);
    const int64_t* user_rows = (const int64_t*)(host + off[12]);
    std::lock_guard<std::mutex> lk(db->mu);
    BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    FitBatchArgs fa;
    UpdateBatchArgs ua;
    fa.lstart[0] = ua.ustart[0] = 0;
    uint32_t mask = 0;
    int64_t max_m = 0;
    for (int q = 0; q < kBatchSlots; ++q) {
        const int64_t lq = q < Q ? L[q] : 0, uq = q < Q ? U[q] : 0;
        VQ_REQUIRE(lq >= 0 && uq >= 0 && uq <= n_user_rows, "query %d: L = %lld, U = %lld (n_user_rows = %lld)", q, (long long)lq, (long long)uq,
                   (long long)n_user_rows);
        VQ_REQUIRE(given || lq <= n_labels, "query %d: L = %lld outside [0, n_labels = %lld]", q, (long long)lq, (long long)n_labels);
        if (lq > 0 && q >= r.q) return fail(VQ_E_STATE, "the last batched round had %d queries (labels for query %d)", r.q, q);
        fa.lstart[q + 1] = fa.lstart[q] + (given ? 0 : lq);
        ua.ustart[q + 1] = ua.ustart[q] + uq;
        ua.qoff[q] = r.start[q];
        fa.qoff[q] = tables ? fa.lstart[q] : r.start[q];      // a given table holds query q's labelled rows from its first label on
        if (lq > 0) {
            mask |= 1u << q;
            max_m = std::max(max_m, r.m(q));
        }
    }
    VQ_REQUIRE(given || fa.lstart[kBatchSlots] == n_labels, "the L of the queries add up to %lld, n_labels is %lld", (long long)fa.lstart[kBatchSlots],
               (long long)n_labels);
    VQ_REQUIRE(ua.ustart[kBatchSlots] == n_user_rows, "the U of the queries add up to %lld, n_user_rows is %lld", (long long)ua.ustart[kBatchSlots],
               (long long)n_user_rows);
    for (int q = 0; q < Q; ++q) {
        if (!((mask >> q) & 1u)) continue;
        VQ_REQUIRE(second[q] >= 0 && second[q] < db->S, "query %d: second = %d outside [0,%d)", q, second[q], db->S);
        VQ_REQUIRE(band_mode[q] == 0 || band_mode[q] == 1, "query %d: band_mode %d (0 = a given reach, 1 = from the user's matches)", q, band_mode[q]);
        if (tables) continue;                         // no positions: the rows' avg came with the block
        for (int64_t l = fa.lstart[q]; l < fa.lstart[q + 1]; ++l)
            VQ_REQUIRE(rows[l] >= 0 && rows[l] < r.m(q), "query %d: row %lld (label %lld) outside [0,%lld)", q, (long long)rows[l],
                       (long long)(l - fa.lstart[q]), (long long)r.m(q));
        for (int64_t u = ua.ustart[q]; u < ua.ustart[q + 1]; ++u)
            VQ_REQUIRE(user_rows[u] >= 0 && user_rows[u] < r.m(q), "query %d: user row %lld (entry %lld) outside [0,%lld)", q, (long long)user_rows[u],
                       (long long)(u - ua.ustart[q]), (long long)r.m(q));
    }
    if (want_scores || do_select)
        VQ_REQUIRE(round_bytes >= r.off[9], "the block of the last batched round needs %lld bytes, got %lld", (long long)r.off[9], (long long)round_bytes);
    if (mask == 0) return VQ_OK;                      // every slot skipped: nothing to launch
    DeviceGuard g(db->device);
    const int64_t stage_w = off[15], stage_band = stage_w + kBatchSlots * 8 * 8;             // behind the block's image: weights | bands
    VQ_HIP(db->grid_buf.grow((size_t)(stage_band + kBatchSlots * 2 * 8)));
    char* base = db->grid_buf;
    // ONE upload: the fit's inputs, the surface piece (given, or about to be overwritten) and the update's inputs are adjacent
    VQ_HIP(hipMemcpyAsync(base, host, (size_t)off[13], hipMemcpyHostToDevice, db->stream));
    const bool have_rows = max_m > 0;                 // false: only empty views, which have neither labels nor scores nor lists
    if (!given && (tables || have_rows)) {            // a given table needs no row of this handle
        fa.avg = tables ? (const double*)(base + off[4]) : (const double*)(db->bround_dev + r.off[4]);
        fa.w_grid = (const double*)(base + off[0]);
        fa.th_grid = (const double*)(base + off[1]);
        fa.ballast = (const double*)(base + off[2]);
        fa.rows = tables ? nullptr : (const int64_t*)(base + off[4]);
        fa.labels = (const double*)(base + off[5]);
        fa.out = (double*)(base + off[6]);
        fa.G = G;
        fa.T = T;
        fa.S = db->S;
        loss_surface_batch_kernel<<<dim3(G, Q), kFitThreads, 0, db->stream>>>(fa);
        VQ_CHECK_LAUNCH();
    }
    ua.surface = (const double*)(base + off[6]);
    ua.w_grid = (const double*)(base + off[0]);
    ua.th_grid = (const double*)(base + off[1]);
    ua.L = (const int64_t*)(base + off[3]);
    ua.second = (const int32_t*)(base + off[7]);
    ua.eps = (const double*)(base + off[8]);
    ua.band_mode = (const int32_t*)(base + off[9]);
    ua.near = (const double*)(base + off[10]);
    ua.user_rows = tables ? nullptr : (const int64_t*)(base + off[12]);
    ua.user_avg = tables ? (const double*)(base + off[12]) : nullptr;
    ua.scores = have_rows ? (const double*)(db->bround_dev + r.off[5]) : nullptr;
    ua.pick = (double*)(base + off[13]);
    ua.pick_idx = (int32_t*)(base + off[14]);
    ua.w = (double*)(base + stage_w);
    ua.band = (double*)(base + stage_band);
    ua.G = G;
    ua.T = T;
    ua.S = db->S;
    pick_refine_batch_kernel<<<Q, kPickThreads, 0, db->stream>>>(ua);
    VQ_CHECK_LAUNCH();
    if (have_rows) {
        const int rc = launch_rescore(db, r, mask, max_m, ua.w);
        if (rc != VQ_OK) return rc;
    }
    review_band_batch_kernel<<<Q, kPickThreads, 0, db->stream>>>(ua);
    VQ_CHECK_LAUNCH();
    if (have_rows) {
        const int rc = partition_runs(db, r, mask, ua.band, (char*)round_block, want_scores, do_select);
        if (rc != VQ_OK) return rc;
    }
    VQ_HIP(hipMemcpyAsync(host + off[13], base + off[13], (size_t)(off[15] - off[13]), hipMemcpyDeviceToHost, db->stream));         // pick | pick_idx
    const int64_t cell = (int64_t)G * T * 8;
    for (int q = 0; want_surface && q < Q;) {         // the surfaces of the slots served, adjacent ones in one copy
        if (!((mask >> q) & 1u)) {
            ++q;
            continue;
        }
        int e = q;
        while (e + 1 < Q && ((mask >> (e + 1)) & 1u)) ++e;
        VQ_HIP(hipMemcpyAsync(host + off[6] + q * cell, base + off[6] + q * cell, (size_t)((e + 1 - q) * cell), hipMemcpyDeviceToHost, db->stream));
        q = e + 1;
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    if (do_select) {
        if (have_rows) adopt_counts(r, (const char*)round_block, mask);
        else empty_results(r, (char*)round_block, mask);
    }
    return VQ_OK;
}

int vq_db_batch_round_update(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                             void* update_block, int64_t update_bytes, void* round_block, int64_t round_bytes, int32_t flags) {
    return run_batch_update(db, false, n_queries, n_grid, n_thresholds, n_labels, n_user_rows, update_block, update_bytes, round_block, round_bytes, flags);
}

// ---- what a row-sharded database makes one operation of that update with (include/vq_amd_round_shard.h) ------------------------------
int vq_db_batch_avg_rows_layout(vq_db* db, int32_t n_queries, int64_t n_rows, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = batch_grid_shape(n_queries, 1, n_rows);
    if (rc != VQ_OK) return rc;
    batch_avg_rows_layout(n_queries, db->S, n_rows, off);
    return VQ_OK;
}

int vq_db_batch_round_avg_rows(vq_db* db, int32_t n_queries, int64_t n_rows, void* block, int64_t block_bytes) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = batch_grid_shape(n_queries, 1, n_rows);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries, S = db->S;
    int64_t off[4];
    batch_avg_rows_layout(Q, S, n_rows, off);
    VQ_REQUIRE(block_bytes >= off[3], "the block of these avg rows needs %lld bytes (vq_db_batch_avg_rows_layout), got %lld", (long long)off[3],
               (long long)block_bytes);
    char* host = (char*)block;
    const int64_t* L = (const int64_t*)(host + off[0]);
    const int64_t* rows = (const int64_t*)(host + off[1]);
    std::lock_guard<std::mutex> lk(db->mu);
    const BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    AvgRowsArgs a;
    int64_t max_l = 0;
    {
        const int rc = chosen_rows(r, Q, L, rows, n_rows, a.lstart, a.qoff, &max_l);
        if (rc != VQ_OK) return rc;
    }
    if (n_rows == 0) return VQ_OK;                    // every query skipped: nothing to launch
    DeviceGuard g(db->device);
    VQ_HIP(db->grid_buf.grow((size_t)off[3]));
    char* base = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(base, host, (size_t)off[2], hipMemcpyHostToDevice, db->stream));      // L | rows: adjacent
    a.avg = (const double*)(db->bround_dev + r.off[4]);
    a.rows = (const int64_t*)(base + off[1]);
    a.out = (double*)(base + off[2]);
    a.S = S;
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>((max_l * S + 255) / 256, (int64_t)db->cus * 8));
    avg_rows_batch_kernel<<<dim3(bx, Q), 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(host + off[2], base + off[2], (size_t)(n_rows * S * 8), hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_batch_update_given_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                                    int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = batch_fit_shape(n_queries, n_grid, n_thresholds, n_labels);
    if (rc != VQ_OK) return rc;
    VQ_REQUIRE(n_user_rows >= 0, "n_user_rows must not be negative");
    batch_update_layout(n_queries, n_grid, n_thresholds, n_labels, n_user_rows, off, (int64_t)db->S * 8);
    return VQ_OK;
}

int vq_db_batch_round_update_given(vq_db* db, int32_t n_queries, int32_t n_grid, int32_t n_thresholds, int64_t n_labels, int64_t n_user_rows,
                                   void* update_block, int64_t update_bytes, void* round_block, int64_t round_bytes, int32_t flags) {
    return run_batch_update(db, true, n_queries, n_grid, n_thresholds, n_labels, n_user_rows, update_block, update_bytes, round_block, round_bytes, flags);
}

// ---- the scores of chosen rows of a batched round's queries under a grid of weights (include/vq_amd_round_grid.h) --------------------
int vq_db_batch_grid_layout(vq_db* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = batch_grid_shape(n_queries, n_grid, n_rows);
    if (rc != VQ_OK) return rc;
    batch_grid_layout(n_queries, n_grid, n_rows, off);
    return VQ_OK;
}

int vq_db_batch_round_grid(vq_db* db, int32_t n_queries, int32_t n_grid, int64_t n_rows, void* block, int64_t block_bytes) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = batch_grid_shape(n_queries, n_grid, n_rows);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries, G = n_grid;
    int64_t off[5];
    batch_grid_layout(Q, G, n_rows, off);
    VQ_REQUIRE(block_bytes >= off[4], "the block of these grid scores needs %lld bytes (vq_db_batch_grid_layout), got %lld", (long long)off[4],
               (long long)block_bytes);
    char* host = (char*)block;
    const int64_t* L = (const int64_t*)(host + off[1]);
    const int64_t* rows = (const int64_t*)(host + off[2]);
    std::lock_guard<std::mutex> lk(db->mu);
    const BatchRound& r = db->round;
    if (r.q == 0) return fail(VQ_E_STATE, "no batched round has run on this handle");
    GridBatchArgs a;
    int64_t max_l = 0;
    {
        const int rc = chosen_rows(r, Q, L, rows, n_rows, a.lstart, a.qoff, &max_l);
        if (rc != VQ_OK) return rc;
    }
    if (n_rows == 0) return VQ_OK;                    // every query skipped: nothing to launch
    DeviceGuard g(db->device);
    VQ_HIP(db->grid_buf.grow((size_t)off[4]));
    char* base = db->grid_buf;
    VQ_HIP(hipMemcpyAsync(base, host, (size_t)off[3], hipMemcpyHostToDevice, db->stream));      // grid | L | rows: adjacent
    a.avg = (const double*)(db->bround_dev + r.off[4]);
    a.w_grid = (const double*)(base + off[0]);
    a.rows = (const int64_t*)(base + off[2]);
    a.out = (double*)(base + off[3]);
    a.G = G;
    a.S = db->S;
    grid_scores_batch_kernel<<<dim3(cdiv((int64_t)G * max_l, 256), Q), 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(host + off[3], base + off[3], (size_t)((int64_t)G * n_rows * 8), hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

}  // extern "C"
