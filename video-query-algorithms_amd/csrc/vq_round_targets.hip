// Batched query rounds on gfx950: the bootstrapped targets of up to 16 tickets in one call (include/vq_amd_round_targets.h).
//
// What it replaces (paths relative to the reference checkout):
//   src/models/target_clip.py:161-261  the two closed forms, per (draw, stream, split) -- csrc/vq_boot.hip has the algebra
//   src/models/target_clip.py:64-73    bagging: the mean of the draws' targets
//   src/models/target_clip.py:75-82    partial_update: keep * target + (1 - keep) * previous
//
// vq_db_bootstrap_target solves one draw per call: a gather, four allocations, three uploads, S*E workgroups, a synchronisation.
// A group of 16 revise tickets that bag three draws each makes 48 such calls in front of ONE shared pass.  Here the group is one
// call of four launches on the handle's own buffers:
//
//   gather   the rows of all pools, once (gather_rows_device, row numbers read from the uploaded block)
//   gram     G[q][slot] = pool x pool, one workgroup per (query, slot, row i): every entry is the 64-lane strided fp64 dot + the
//            shuffle tree of bootstrap_kernel, so a draw's Gram matrix is a SUB-MATRIX of its pool's with the bits bootstrap_kernel
//            computes on the draw's rows -- the draws of a bagging round share it
//   solve    one workgroup per (draw, slot): trace, scale and the two Gauss-Jordan solves of bootstrap_kernel (gauss_jordan itself,
//            csrc/vq_gauss_jordan.h) on the sub-matrix in draw order; the systems sit in local memory for draws of at most
//            kTargetsLdsRows rows and in a scratch area otherwise; the coefficients stay on the device
//   combine  per (query, slot, 256 dimensions): w_b[d] = sum_k coef_b[k] x_k[d] in draw order for draw after draw, the sequential
//            mean, the blend, the store -- w_b lives in a register
//
// Every floating-point operation of a draw is the one bootstrap_kernel performs, in its order (the library builds with
// -ffp-contract=off), which is what tests/test_batch_targets_gpu.py holds the call to: equal bits.
#include <algorithm>
#include <climits>

#include "vq_db.h"
#include "vq_gauss_jordan.h"

using namespace vq;

namespace {

constexpr int kTargetsSlots = 16;          // queries per call (the slots of a batched round)
constexpr int kTargetsMaxRows = 256;       // rows per pool and per draw (BOOT_MAX_ROWS of csrc/vq_boot.hip)
constexpr int kTargetsMaxDraws = 64;       // draws per query
// A draw of L rows needs at most L (L + 2) doubles for its two augmented systems (need_doubles below).  86 rows: 60 544 bytes, which
// with the 3 KB of static local memory of the solve kernel stays under the 64 KB a workgroup gets without a function attribute, and
// a typical draw (tens of rows, a few KB) leaves a CU room for many workgroups.  Longer draws take the scratch area.
constexpr int kTargetsLdsRows = 86;
constexpr int kTargetsWsGroups = 256;      // workgroups of the scratch-area launch (one per CU): each owns one scratch slot and walks problems

// off[11]: see include/vq_amd_round_targets.h
void targets_layout(int Q, int64_t n_rows, int n_draws, int64_t n_entries, int64_t nvd, int64_t* off) {
    off[0] = 0;
    off[1] = off[0] + up64((int64_t)Q * 8 * 4);
    off[2] = off[1] + up64((int64_t)Q * 4 * 8);
    off[3] = off[2] + up64(n_rows * 8);
    off[4] = off[3] + up64((int64_t)n_draws * 2 * 4);
    off[5] = off[4] + up64(n_entries * 4);
    off[6] = off[5] + up64((int64_t)n_draws * 5 * 4);          // work: [n_draws][4] (first entry | query | 2 unused) | list [n_draws]
    off[7] = off[6] + up64((int64_t)Q * nvd * 8);
    off[8] = off[7] + up64((int64_t)Q * 4 * 4);
    off[9] = off[8] + up64((int64_t)Q * nvd * 8);
    off[10] = kTargetsLdsRows;
}

int targets_shape(int Q, int64_t n_rows, int n_draws, int64_t n_entries) {
    VQ_REQUIRE(Q >= 1 && Q <= kTargetsSlots, "n_queries must be in [1,%d] (got %d)", kTargetsSlots, Q);
    VQ_REQUIRE(n_rows >= Q && n_rows <= (int64_t)Q * kTargetsMaxRows, "n_pool_rows: 1 to %d rows per query (got %lld for %d queries)", kTargetsMaxRows,
               (long long)n_rows, Q);
    VQ_REQUIRE(n_draws >= Q && n_draws <= Q * kTargetsMaxDraws, "n_draws: 1 to %d draws per query (got %d for %d queries)", kTargetsMaxDraws, n_draws, Q);
    VQ_REQUIRE(n_entries >= n_draws && n_entries <= (int64_t)n_draws * kTargetsMaxRows, "n_entries: 1 to %d positions per draw (got %lld for %d draws)",
               kTargetsMaxRows, (long long)n_entries, n_draws);
    return VQ_OK;
}

// doubles of the two augmented systems of a draw of m matches and n non-matches: A1 [n][n + m + 1] (only with non-matches and
// mu != 0) then B [m][m + 2]
__host__ __device__ inline int64_t first_system(int m, int n, double mu) { return (n > 0 && mu != 0.0) ? (int64_t)n * (n + m + 1) : 0; }
inline int64_t need_doubles(int m, int n, double mu) { return first_system(m, n, mu) + (int64_t)m * (m + 2); }

struct TargetsArgs {
    const void* dense;         // [n_pool_rows][NV][D]: the gathered pools, query after query
    int NV, D, Q;
    const int32_t* query;      // [Q][8]
    const double* param;       // [Q][4]
    const int32_t* draw;       // [n_draws][2]
    const int32_t* pos;        // [n_entries]
    const int32_t* work;       // [n_draws][4]
    const int32_t* list;       // [n_draws]: the draws solved in local memory, then the others
    const double* previous;    // [Q][NV][D]
    double* target;            // [Q][NV][D]
    int32_t* status;           // [Q][4]
    double* gram;              // query q, slot p: [R_q][R_q] at gram_off[q] + p R_q^2
    double* coef;              // slot p, draw b: [L_b] at p * n_entries + the draw's first entry
    int32_t* pstatus;          // [n_draws][NV]: 0 ok, 1 singular
    double* ws;                // the scratch area: ws_stride doubles per workgroup
    int64_t ws_stride, n_entries;
    int64_t gram_off[kTargetsSlots + 1];
    int32_t pool_start[kTargetsSlots + 1], draw_start[kTargetsSlots + 1], unit_start[kTargetsSlots + 1];
};

// G = pool x pool for every (query, slot): one workgroup per row i, its four waves take blocks of four columns j >= i.  Per entry the
// arithmetic of bootstrap_kernel: lane d-strided products summed in d order, the shuffle tree 32..1, lane 0's value to both
// triangles; x_i[d] is widened once for the four columns.
template <typename T>
__global__ __launch_bounds__(256) void targets_gram_kernel(TargetsArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int q = 0;
    while (q + 1 < a.Q && (int)blockIdx.x >= a.unit_start[q + 1]) ++q;
    const int R = a.query[8 * q], local = (int)blockIdx.x - a.unit_start[q];
    const int p = local / R, i = local - p * R, D = a.D;
    const T* rows = static_cast<const T*>(a.dense) + ((size_t)a.pool_start[q] * a.NV + p) * D;
    const size_t row_stride = (size_t)a.NV * D;
    double* G = a.gram + a.gram_off[q] + (size_t)p * R * R;
    const T* xi = rows + i * row_stride;
    for (int j0 = i + 4 * wave; j0 < R; j0 += 16) {
        const T* xj[4];
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) xj[u] = rows + (size_t)min(j0 + u, R - 1) * row_stride;
        for (int d = lane; d < D; d += 64) {
            const double v = widen(xi[d]);
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += v * widen(xj[u][d]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double t = s[u];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
            if (lane == 0 && j0 + u < R) {
                G[(size_t)i * R + j0 + u] = t;
                G[(size_t)(j0 + u) * R + i] = t;
            }
        }
    }
}

// One (draw, slot) problem per workgroup (local memory), or a walk over problems with one scratch slot per workgroup: bootstrap_kernel
// behind its Gram matrix, with G(i, j) read from the pool's matrix through the draw's positions.
template <bool kLds>
__global__ __launch_bounds__(256) void targets_solve_kernel(TargetsArgs a, int first, int count) {
    extern __shared__ double lds_sys[];
    __shared__ int piv;
    __shared__ double sh_scale;
    __shared__ double piv_floor[kTargetsMaxRows];
    __shared__ int at[kTargetsMaxRows];
    const int tid = threadIdx.x;
    for (int item = blockIdx.x; item < count * a.NV; item += gridDim.x) {
        const int b = a.list[first + item / a.NV], p = item % a.NV;
        const int es = a.work[4 * b], q = a.work[4 * b + 1];
        const int r = a.draw[2 * b], m = a.draw[2 * b + 1], n = r - m, R = a.query[8 * q];
        const double mu = a.param[4 * q];
        const double* G = a.gram + a.gram_off[q] + (size_t)p * R * R;
        __syncthreads();                                        // the previous problem of this workgroup is done with at[]
        for (int k = tid; k < r; k += 256) at[k] = a.pos[es + k];
        __syncthreads();
#define GS(i, j) G[(size_t)at[i] * R + at[j]]
        double* sys = kLds ? lds_sys : a.ws + (size_t)blockIdx.x * a.ws_stride;
        double* A1 = sys;                                       // [n][n + m + 1]
        double* Bm = sys + first_system(m, n, mu);              // [m][m + 2]
        double* coef = a.coef + (size_t)p * a.n_entries + es;   // [r]: a (m), b (n)
        if (tid == 0) {
            double tr = 0.0;
            for (int j = 0; j < n; ++j) tr += GS(m + j, m + j);
            sh_scale = (n > 0 && mu != 0.0) ? (tr < 1.0e300 ? mu / tr : __builtin_nan("")) : 0.0;       // as bootstrap_kernel
        }
        __syncthreads();
        const double scale = sh_scale;
        const bool with_y = n > 0 && scale != 0.0;
        bool ok = true;
        if (with_y) {
            const int w1 = n + m + 1;
            for (int idx = tid; idx < n * w1; idx += 256) {
                const int i = idx / w1, c = idx - i * w1;
                double v;
                if (c < n)
                    v = (i == c ? 1.0 : 0.0) + scale * GS(m + i, m + c);
                else if (c < n + m)
                    v = GS(m + i, c - n);
                else
                    v = 1.0;
                A1[idx] = v;
            }
            __syncthreads();
            ok = gauss_jordan(A1, n, m + 1, w1, &piv, piv_floor);
            if (ok) {
                for (int idx = tid; idx < m * (m + 2); idx += 256) {
                    const int i = idx / (m + 2), c = idx - i * (m + 2);
                    double v;
                    if (c < m) {
                        double s = 0.0;
                        for (int j = 0; j < n; ++j) s += GS(i, m + j) * (scale * A1[(size_t)j * w1 + n + c]);
                        v = GS(i, c) - s;
                    } else if (c == m) {
                        v = 1.0;
                    } else {
                        double s = 0.0;
                        for (int j = 0; j < n; ++j) s += GS(i, m + j) * (scale * A1[(size_t)j * w1 + n + m]);
                        v = s;
                    }
                    Bm[idx] = v;
                }
                __syncthreads();
                ok = gauss_jordan(Bm, m, 2, m + 2, &piv, piv_floor);
            }
            if (ok) {
                for (int i = tid; i < m; i += 256) coef[i] = Bm[(size_t)i * (m + 2) + m] - Bm[(size_t)i * (m + 2) + m + 1];
                __syncthreads();
                for (int j = tid; j < n; j += 256) {
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s += (scale * A1[(size_t)j * w1 + n + i]) * coef[i];
                    coef[m + j] = scale * A1[(size_t)j * w1 + n + m] - s;
                }
            }
        } else {
            for (int idx = tid; idx < m * (m + 2); idx += 256) {
                const int i = idx / (m + 2), c = idx - i * (m + 2);
                Bm[idx] = c < m ? GS(i, c) : (c == m ? 1.0 : 0.0);
            }
            __syncthreads();
            ok = gauss_jordan(Bm, m, 2, m + 2, &piv, piv_floor);
            if (ok) {
                for (int i = tid; i < m; i += 256) coef[i] = Bm[(size_t)i * (m + 2) + m];
                for (int j = tid; j < n; j += 256) coef[m + j] = 0.0;
            }
        }
#undef GS
        if (tid == 0) a.pstatus[(size_t)b * a.NV + p] = ok ? 0 : 1;
    }
}

// Per (query, slot, 256 dimensions): the rows of draw after draw combined under its coefficients in draw order (the last loop of
// bootstrap_kernel), the draws summed in order and divided by their number (numpy's mean over axis 0), the blend.  A query with a
// singular (draw, slot) gets its status and no target.
template <typename T>
__global__ __launch_bounds__(256) void targets_combine_kernel(TargetsArgs a) {
    __shared__ int fail;
    const int tid = threadIdx.x, p = blockIdx.x, q = blockIdx.y, d = blockIdx.z * 256 + tid;
    const int B = a.query[8 * q + 2], b0 = a.draw_start[q];
    if (tid == 0) fail = INT_MAX;
    __syncthreads();
    for (int idx = tid; idx < B * a.NV; idx += 256)
        if (a.pstatus[(size_t)b0 * a.NV + idx] != 0) atomicMin(&fail, idx);
    __syncthreads();
    const int bad = fail;
    if (p == 0 && blockIdx.z == 0 && tid == 0) {
        a.status[4 * q] = bad == INT_MAX ? 0 : 1;
        a.status[4 * q + 1] = bad == INT_MAX ? 0 : bad / a.NV;
        a.status[4 * q + 2] = bad == INT_MAX ? 0 : bad % a.NV;
        a.status[4 * q + 3] = 0;
    }
    if (bad != INT_MAX || d >= a.D) return;
    const T* rows = static_cast<const T*>(a.dense) + ((size_t)a.pool_start[q] * a.NV + p) * a.D + d;
    const size_t row_stride = (size_t)a.NV * a.D;
    double acc = 0.0;
    for (int bl = 0; bl < B; ++bl) {
        const int b = b0 + bl, es = a.work[4 * b], r = a.draw[2 * b];
        const double* coef = a.coef + (size_t)p * a.n_entries + es;
        double s = 0.0;
        for (int k = 0; k < r; ++k) s += coef[k] * widen(rows[a.pos[es + k] * row_stride]);
        acc = bl == 0 ? s : acc + s;
    }
    double t = B == 1 ? acc : acc / (double)B;
    const size_t o = ((size_t)q * a.NV + p) * a.D + d;
    if (a.query[8 * q + 3] == 1) t = a.param[4 * q + 1] * t + a.param[4 * q + 2] * a.previous[o];
    a.target[o] = t;
}

}  // namespace

extern "C" {

int vq_db_batch_targets_layout(vq_db* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, int64_t* off) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int rc = targets_shape(n_queries, n_pool_rows, n_draws, n_entries);
    if (rc != VQ_OK) return rc;
    targets_layout(n_queries, n_pool_rows, n_draws, n_entries, (int64_t)db->S * db->E * db->D, off);
    return VQ_OK;
}

int vq_db_batch_targets(vq_db* db, int32_t n_queries, int64_t n_pool_rows, int32_t n_draws, int64_t n_entries, void* block, int64_t block_bytes) {
    VQ_REQUIRE(db && block, "NULL argument");
    {
        const int rc = targets_shape(n_queries, n_pool_rows, n_draws, n_entries);
        if (rc != VQ_OK) return rc;
    }
    const int Q = n_queries, NV = db->S * db->E, D = db->D;
    const int64_t nvd = (int64_t)NV * D;
    int64_t off[11];
    targets_layout(Q, n_pool_rows, n_draws, n_entries, nvd, off);
    VQ_REQUIRE(block_bytes >= off[9], "the block of these batched targets needs %lld bytes (vq_db_batch_targets_layout), got %lld", (long long)off[9],
               (long long)block_bytes);
    char* host = (char*)block;
    const int32_t* query = (const int32_t*)(host + off[0]);
    const double* param = (const double*)(host + off[1]);
    const int64_t* rows = (const int64_t*)(host + off[2]);
    const int32_t* draw = (const int32_t*)(host + off[3]);
    const int32_t* pos = (const int32_t*)(host + off[4]);
    int32_t* work = (int32_t*)(host + off[5]);
    int32_t* list = work + 4 * (int64_t)n_draws;

    // ---- every check, and the plan of the launches, on the host
    TargetsArgs a;
    a.pool_start[0] = a.draw_start[0] = a.unit_start[0] = 0;
    a.gram_off[0] = 0;
    bool any_previous = false;
    int64_t entry = 0;
    for (int q = 0; q < Q; ++q) {
        const int R = query[8 * q], mq = query[8 * q + 1], B = query[8 * q + 2], mode = query[8 * q + 3];
        VQ_REQUIRE(R >= 1 && R <= kTargetsMaxRows, "query %d: a pool holds 1 to %d rows (got %d)", q, kTargetsMaxRows, R);
        VQ_REQUIRE(mq >= 1 && mq <= R, "query %d: bootstrapping needs at least one validated match (%d of the pool's %d rows)", q, mq, R);
        VQ_REQUIRE(B >= 1 && B <= kTargetsMaxDraws, "query %d: 1 to %d draws (got %d)", q, kTargetsMaxDraws, B);
        VQ_REQUIRE(mode == 0 || mode == 1, "query %d: mode 0 (the mean of the draws) or 1 (blended with the previous target), got %d", q, mode);
        VQ_REQUIRE(a.pool_start[q] + R <= n_pool_rows && a.draw_start[q] + B <= n_draws, "query %d: the pools or draws of the queries exceed n_pool_rows = %lld / n_draws = %d",
                   q, (long long)n_pool_rows, n_draws);
        any_previous |= mode == 1;
        for (int k = 0; k < R; ++k) {
            const int64_t row = rows[a.pool_start[q] + k];
            VQ_REQUIRE(row >= 0 && row < db->n, "query %d: pool row %lld outside [0,%lld)", q, (long long)row, (long long)db->n);
        }
        for (int bl = 0; bl < B; ++bl) {
            const int b = a.draw_start[q] + bl, L = draw[2 * b], mb = draw[2 * b + 1];
            VQ_REQUIRE(L >= 1 && L <= R && mb >= 1 && mb <= L, "query %d, draw %d: %d positions, %d of them matches (a draw needs a match and fits its pool of %d)", q,
                       bl, L, mb, R);
            VQ_REQUIRE(entry + L <= n_entries, "query %d, draw %d: the draws hold more than n_entries = %lld positions", q, bl, (long long)n_entries);
            uint64_t seen[kTargetsMaxRows / 64] = {0, 0, 0, 0};
            for (int k = 0; k < L; ++k) {
                const int at = pos[entry + k];
                VQ_REQUIRE(at >= 0 && at < R, "query %d, draw %d: position %d outside its pool of %d rows", q, bl, at, R);
                VQ_REQUIRE((k < mb) == (at < mq), "query %d, draw %d: position %d is %s of the pool, listed among the draw's %s", q, bl, at,
                           at < mq ? "a match" : "a non-match", k < mb ? "matches" : "non-matches");
                VQ_REQUIRE(!((seen[at >> 6] >> (at & 63)) & 1), "query %d, draw %d: position %d twice", q, bl, at);
                seen[at >> 6] |= 1ull << (at & 63);
            }
            entry += L;
        }
        a.pool_start[q + 1] = a.pool_start[q] + R;
        a.draw_start[q + 1] = a.draw_start[q] + B;
        a.unit_start[q + 1] = a.unit_start[q] + NV * R;
        a.gram_off[q + 1] = a.gram_off[q] + (int64_t)NV * R * R;
    }
    VQ_REQUIRE(a.pool_start[Q] == n_pool_rows && a.draw_start[Q] == n_draws && entry == n_entries,
               "the pools, draws and positions of the queries add up to %d / %d / %lld; n_pool_rows, n_draws, n_entries are %lld / %d / %lld", a.pool_start[Q],
               a.draw_start[Q], (long long)entry, (long long)n_pool_rows, n_draws, (long long)n_entries);
    for (int q = Q; q < kTargetsSlots; ++q) {
        a.pool_start[q + 1] = a.pool_start[q];
        a.draw_start[q + 1] = a.draw_start[q];
        a.unit_start[q + 1] = a.unit_start[q];
        a.gram_off[q + 1] = a.gram_off[q];
    }

    std::lock_guard<std::mutex> lk(db->mu);
    // the work piece: where each draw's positions start and whose it is; the draws solved in local memory first, then the others
    int n_lds = 0, n_ws = 0;
    int64_t lds_need = 0, ws_need = 0;
    entry = 0;
    for (int q = 0; q < Q; ++q)
        for (int b = a.draw_start[q]; b < a.draw_start[q + 1]; ++b) {
            work[4 * b] = (int32_t)entry;
            work[4 * b + 1] = q;
            work[4 * b + 2] = work[4 * b + 3] = 0;
            entry += draw[2 * b];
            if (draw[2 * b] <= kTargetsLdsRows) ++n_lds;
        }
    for (int b = 0, il = 0, iw = n_lds; b < n_draws; ++b) {
        const int L = draw[2 * b], mb = draw[2 * b + 1];
        const int64_t need = need_doubles(mb, L - mb, param[4 * work[4 * b + 1]]);
        if (L <= kTargetsLdsRows) {
            list[il++] = b;
            lds_need = std::max(lds_need, need);
        } else {
            list[iw++] = b;
            ws_need = std::max(ws_need, need);
            ++n_ws;
        }
    }
    const int ws_groups = std::min(n_ws * NV, kTargetsWsGroups);

    DeviceGuard g(db->device);
    const int64_t gram_at = off[9], coef_at = gram_at + up64(a.gram_off[Q] * 8), pstat_at = coef_at + up64((int64_t)NV * n_entries * 8);
    VQ_HIP(db->targets_buf.grow((size_t)(pstat_at + up64((int64_t)n_draws * NV * 4))));
    if (n_ws) VQ_HIP(db->targets_ws.grow((size_t)ws_groups * ws_need * 8));
    char* base = db->targets_buf;
    VQ_HIP(hipMemcpyAsync(base, host, (size_t)(any_previous ? off[7] : off[6]), hipMemcpyHostToDevice, db->stream));      // adjacent: one copy
    int rc = gather_rows_device(db, nullptr, (int)n_pool_rows, &a.dense, (const int64_t*)(base + off[2]));
    if (rc != VQ_OK) return rc;
    a.NV = NV;
    a.D = D;
    a.Q = Q;
    a.query = (const int32_t*)(base + off[0]);
    a.param = (const double*)(base + off[1]);
    a.draw = (const int32_t*)(base + off[3]);
    a.pos = (const int32_t*)(base + off[4]);
    a.work = (const int32_t*)(base + off[5]);
    a.list = a.work + 4 * (int64_t)n_draws;
    a.previous = (const double*)(base + off[6]);
    a.status = (int32_t*)(base + off[7]);
    a.target = (double*)(base + off[8]);
    a.gram = (double*)(base + gram_at);
    a.coef = (double*)(base + coef_at);
    a.pstatus = (int32_t*)(base + pstat_at);
    a.ws = db->targets_ws;
    a.ws_stride = ws_need;
    a.n_entries = n_entries;
    const dim3 cgrid(NV, Q, cdiv(D, 256));
    if (db->dtype == VQ_F16)
        targets_gram_kernel<__half><<<a.unit_start[Q], 256, 0, db->stream>>>(a);
    else if (db->dtype == VQ_F32)
        targets_gram_kernel<float><<<a.unit_start[Q], 256, 0, db->stream>>>(a);
    else
        targets_gram_kernel<double><<<a.unit_start[Q], 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    if (n_lds) {
        targets_solve_kernel<true><<<n_lds * NV, 256, (size_t)lds_need * 8, db->stream>>>(a, 0, n_lds);
        VQ_CHECK_LAUNCH();
    }
    if (n_ws) {
        targets_solve_kernel<false><<<ws_groups, 256, 0, db->stream>>>(a, n_lds, n_ws);
        VQ_CHECK_LAUNCH();
    }
    if (db->dtype == VQ_F16)
        targets_combine_kernel<__half><<<cgrid, 256, 0, db->stream>>>(a);
    else if (db->dtype == VQ_F32)
        targets_combine_kernel<float><<<cgrid, 256, 0, db->stream>>>(a);
    else
        targets_combine_kernel<double><<<cgrid, 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipMemcpyAsync(host + off[7], base + off[7], (size_t)(off[9] - off[7]), hipMemcpyDeviceToHost, db->stream));   // status | target: one copy
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

}  // extern "C"
