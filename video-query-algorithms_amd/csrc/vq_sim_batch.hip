// ------------------------------------------------------------------------------------------------
// batched scan: Q queries per pass over the database, on the fp64 matrix cores
// ------------------------------------------------------------------------------------------------
// The single-query scan keeps the whole fp64 query (S*E*D*8 = 80 KB at cfg 4) in LDS; Q of them do not fit.  The
// batched scan therefore walks the database one (stream, split) slice at a time: the slice's query vectors (16 slots x
// D x 8 bytes = 128 KB, unused slots zero) sit in LDS and a wave multiplies a tile of 16 clips against all 16 slots with
// v_mfma_f64_16x16x4_f64: D[clip][query] += A[clip][k] B[k][query], 256 MFMAs per tile and slice.  Operand layouts
// (tools/ubench/mfma_f64_layout.hip): A lane l = (clip l % 16, k l / 16), B lane l = (k l / 16, query l % 16), D lane l
// register r = (clip l / 16 + 4 r, query l % 16).  Per 64-element chunk a lane loads four 16-byte pieces such that one load
// instruction covers 64 contiguous bytes of each of the 16 clips, converts to fp64 and feeds 16 MFMAs; the matching query
// values come from LDS with one ds_read_b64 per MFMA (rows swizzled: conflict-free).
// The fp64 matrix rate (64 cycles per MFMA and SIMD = 78.6 TFLOP/s) puts 16 queries x 41 GB at 4.2 ms of matrix time,
// under the 6.6 ms the HBM stream takes: the pass is HBM-bound, i.e. 16 queries cost what one does.
// The k order of a dot differs from scan_kernel's (matrix-core accumulation), so batched and single-query scores agree to rounding
// (<= 1e-12, tested), not bit for bit.  (Round 2 ran this as ten slice launches into a [slice][query][clip] matrix plus a finalising
// launch -- 2.6 GB written and read back per pass at cfg 4; batch_fused_kernel below replaced it in round 3 and was checked against
// it bit for bit until the two-kernel form was removed in round 5.)
#include <algorithm>

#include "vq_db.h"

using namespace vq;

typedef double doublex4 __attribute__((ext_vector_type(4)));

// One chunk of a clip's vector as a lane sees it, P pieces of 16 elements: piece m holds elements 16 m + 4 kk .. + 3 of the chunk (kk =
// the lane's k quarter), so that ONE load instruction covers 64 contiguous bytes per clip across the four k-lanes and a refill is 64 P
// contiguous bytes of each clip.
template <typename T, int P>
struct ChunkP;
template <int P>
struct ChunkP<float, P> {
    float4 v[P];
    __device__ __forceinline__ void load(const float* p) {      // plain loads: two pieces share a 128-byte line (with the non-temporal
#pragma unroll                                                  // hint of the one-query scan the 16-query pass took 8.3 ms instead of 7.5)
        for (int m = 0; m < P; ++m) v[m] = *reinterpret_cast<const float4*>(p + 16 * m);
    }
    __device__ __forceinline__ void load_tiled(const float* p) {   // the tiled mirror: a piece is 1 KB of contiguous memory for the wave,
#pragma unroll                                                     // pieces 256 floats apart; whole lines, read once: non-temporal
        for (int m = 0; m < P; ++m) v[m] = stream_load4(p + 256 * m);
    }
    __device__ __forceinline__ double at(int m, int e) const {
        return (double)(e == 0 ? v[m].x : e == 1 ? v[m].y : e == 2 ? v[m].z : v[m].w);
    }
};
template <int P>
struct ChunkP<double, P> {
    double2 v[P][2];
    __device__ __forceinline__ void load(const double* p) {
#pragma unroll
        for (int m = 0; m < P; ++m) {
            v[m][0] = *reinterpret_cast<const double2*>(p + 16 * m);
            v[m][1] = *reinterpret_cast<const double2*>(p + 16 * m + 2);
        }
    }
    // VQ_LAYOUT_TILED64: piece m = units 8 m + 2 kk and 8 m + 2 kk + 1 of the slice, 32 doubles apart (p = slice + 64 kk + 2 col); per
    // instruction four runs (one per kk) of 256 contiguous bytes -- whole lines, read once: non-temporal.  Pieces 256 doubles apart.
    __device__ __forceinline__ void load_tiled(const double* p) {
#pragma unroll
        for (int m = 0; m < P; ++m) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const vq_d2 r = __builtin_nontemporal_load(reinterpret_cast<const vq_d2*>(p + 256 * m + 32 * h));
                v[m][h] = make_double2(r.x, r.y);
            }
        }
    }
    __device__ __forceinline__ double at(int m, int e) const { return (e & 1) ? v[m][e >> 1].y : v[m][e >> 1].x; }
};

// fp16 rows: a lane's 16-byte load is 8 consecutive halves, so across the four k-lanes a load instruction still covers 64 contiguous bytes of
// each clip -- 32 elements, two 16-element pieces: piece m holds elements 32 (m / 2) + 8 kk + 4 (m % 2) + e of the chunk.  The query rows
// in LDS are stored in that order (batch_query_pos), so the MFMA loop reads them exactly as it does for fp32.
template <int P>
struct ChunkP<__half, P> {
    static_assert(P % 2 == 0, "a 16-byte load of halves is two pieces");
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 v[P / 2];
    __device__ __forceinline__ void load(const __half* p) {     // p = chunk start + 8 kk; plain loads, as for fp32
#pragma unroll
        for (int m = 0; m < P / 2; ++m) v[m] = *reinterpret_cast<const h8*>(p + 32 * m);
    }
    // VQ_LAYOUT_TILED16: load m' holds the same elements 32 m' + 8 kk + 0..7 of the chunk -- ONE unit of the slice, unit 4 m' + kk, at
    // 128 (4 m' + kk) + 8 col halves (p = chunk + 128 kk + 8 col): 1 KB of contiguous memory per wave instruction, whole lines read once:
    // non-temporal.  at() and batch_query_pos stay, so the MFMA sequence per (clip, query) is that of fp16 rows: the same bits.
    __device__ __forceinline__ void load_tiled(const __half* p) {
#pragma unroll
        for (int m = 0; m < P / 2; ++m) v[m] = __builtin_nontemporal_load(reinterpret_cast<const h8*>(p + 512 * m));
    }
    __device__ __forceinline__ double at(int m, int e) const { return half_to_double(v[m >> 1][4 * (m & 1) + e]); }
};

// Where element k of a query row sits inside the row in LDS.  The MFMA loop reads position 16 m + 4 kk + e for piece m, k-lane kk, step e;
// for fp32 / fp64 rows that IS element k.  For fp16 rows the lane holds element 32 (m / 2) + 8 kk + 4 (m % 2) + e there.
template <typename T>
__device__ __forceinline__ int batch_query_pos(int k) {
    if constexpr (sizeof(T) == 2) return (k & ~31) + ((k & 4) << 2) + ((k & 24) >> 1) + (k & 3);
    return k;
}

// Where query slot q starts in LDS (in doubles): rows of D doubles plus a swizzle that makes the 32 lanes of a
// ds_read_b64 group (16 queries x 2 k quarters, 4 doubles apart) hit 32 distinct 8-byte bank slots: D is a multiple
// of 32, so slot = (q % 4) + 8 (q / 4) + 4 kk + const is a bijection onto 0..31.
__device__ __forceinline__ int query_row(int q, int D) { return q * D + (q & 3) + 8 * (q >> 2); }

// ---- the pass as ONE launch: no dot matrix in memory ----------------------------------------------------------------
// A workgroup (16 waves, one per CU) owns TW tiles of 16 clips per wave and "round" and walks the (stream, split) slices
// itself: barrier, the slice's sixteen query rows into LDS (128 KB; from L2 after the first workgroup), barrier, then every
// wave multiplies its tiles against them.  What a tile carries from slice to slice lives in registers: the running sum
// over the splits of the stream being walked (ticket.py:155-160) and the running sum of the weighted squared misses over the
// streams already closed (ticket.py:172-180) -- 16 VGPRs per tile -- so no [slice][query][clip] matrix (2.6 GB per pass at cfg 4)
// and no per-slice launch ramps exist.  Per (clip, query): the dots of the splits present, their mean per stream in split order, the
// weighted squared misses in stream order (clip_add / clip_close_stream / score_from_avg, shared with scan_kernel's epilogue).
// The feature stream never stops at a slice change: the ring of chunk buffers is refilled from the NEXT (slice, tile) of
// the wave while the last chunks of the current one are multiplied, so the loads are in flight across the two barriers (a
// plain __syncthreads() does not wait for vector memory) and HBM stays busy while the matrix pipe waits for the new rows.
// Tiles are dealt so that a short last round spreads over ALL workgroups (tile = base + slot * gridDim + block).
// BatchFusedArgs and BatchViewArgs (the pass over the union of a round's views): csrc/vq_db.h


// Loads whose address is wave-uniform and whose memory no launch in flight writes (the plan of a view round): through the constant
// address space they are scalar loads for certain, so they never enter the in-order vector-memory queue between the feature loads
// (the trap of scan_kernel's VIEW form, see the comment above it).
typedef int vq_i16 __attribute__((ext_vector_type(16)));
template <typename U>
__device__ __forceinline__ U uniform_load(const U* p) {
    return *(const __attribute__((address_space(4))) U*)(p);
}
// element i (per lane) of 16 wave-uniform values: selects, no memory
__device__ __forceinline__ int pick16(const vq_i16& r, int i) {
    int v = r[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) v = i == k ? r[k] : v;
    return v;
}
struct ViewTile {                // a work item of the VIEW form: its 16 database rows (row-major) or the tile behind it (tiled)
    vq_i16 rows;
    int64_t tile, pt;
};

// What batch_view_kernel asks of the plan, per lane (col = its clip of a tile and its query slot, kk = its k quarter):
// the work items, this lane's pointer into a (work item, slice) and where a (query, clip) reports.  Every index comes from wave-uniform
// scalar loads.
template <typename T, bool TILED, int KL>
struct ViewWalk {
    const BatchViewArgs& a;
    const T* feats;
    int64_t clip_elems, ntiles, n_union;
    int NV, D, col, kk;
    __device__ __forceinline__ ViewWalk(const BatchViewArgs& a_, const T* feats_, int NV_, int D_, int col_, int kk_)
        : a(a_), feats(feats_), clip_elems((int64_t)NV_ * D_), ntiles((a_.n + 15) / 16), n_union(a_.n), NV(NV_), D(D_), col(col_), kk(kk_) {
        if (a.items) {                                             // else the whole database: its tiles, addressed as ever
            if (TILED) ntiles = uniform_load(a.counts + 1);
            else {
                n_union = uniform_load(a.counts);
                ntiles = (n_union + 15) / 16;
            }
        }
    }
    // the database rows of the 16 clips of virtual tile `tile`: rows past the union repeat its last row and are never stored
    __device__ __forceinline__ vq_i16 rows_of(int64_t tile) const {
        if (a.items) return uniform_load(reinterpret_cast<const vq_i16*>(a.items + tile * 16));
        vq_i16 rw = {};
#pragma unroll
        for (int i = 0; i < 16; ++i) rw[i] = (int)min(tile * 16 + i, a.n - 1);
        return rw;
    }
    // the tile of the tiled layout behind work item `tile`
    __device__ __forceinline__ int64_t phys_tile(int64_t tile) const { return a.items ? (int64_t)uniform_load(a.items + tile) : tile; }
    // this lane's pointer into slice v of work item `tile`: 64-bit, sixteen arbitrary rows can lie more than 2^32 elements apart
    __device__ __forceinline__ const T* ptr(int64_t tile, int v) const {
        // tiled: units of U = 16 / sizeof(T) elements, 16 U apart along k; a k-lane's KL elements are KL / U units: kk * 16 KL + col * U
        if constexpr (TILED) return feats + (phys_tile(tile) * NV + v) * 16 * D + (kk * 16 * KL + col * vq::tile_unit_of((int)sizeof(T)));
        else return feats + (int64_t)pick16(rows_of(tile), col) * clip_elems + ((int64_t)v * D + KL * kk);
    }
    __device__ __forceinline__ ViewTile tile(int64_t tile) const {
        ViewTile vt = {};
        vt.tile = tile;
        if constexpr (TILED) vt.pt = phys_tile(tile);
        else vt.rows = rows_of(tile);
        return vt;
    }
    // the database row of clip idx of a work item, clamped to one that exists (the presence mask is read by database row)
    __device__ __forceinline__ int64_t mask_row(const ViewTile& vt, int idx) const {
        if constexpr (TILED) return min(vt.pt * 16 + idx, a.n - 1);
        else return pick16(vt.rows, idx);
    }
    // where (this lane's query, clip idx of the work item) reports in the compact outputs: start[q] + the clip's position in the query's
    // view, or -1 -- a row past the union, an unused query slot, a clip outside the query's view
    __device__ __forceinline__ int64_t entry(const ViewTile& vt, int idx) const {
        int64_t row;
        bool ok;
        if constexpr (TILED) {
            row = vt.pt * 16 + idx;
            ok = row < a.n;
        } else {
            row = pick16(vt.rows, idx);
            ok = vt.tile * 16 + idx < n_union;
        }
        if (!ok || !(((a.whole | a.members) >> col) & 1u)) return -1;         // also the slots past Q
        const int64_t pos = ((a.whole >> col) & 1u) ? row : (int64_t)a.inv[(int64_t)col * a.inv_stride + row];
        return pos < 0 ? -1 : a.start[col] + pos;
    }
};

// ROUND (vq_db_query_round_batch, include/vq_amd_rounds.h): the weights come as the round block holds them ([Q][8]) and every stream's
// mean also goes to avg[q][clip][s] where the stream closes.  Stores only: a score is the same operands in the same order, so the
// same bits as the plain pass.
template <typename T, int CH, int TW, bool PRES, int P, bool TILED = false, bool ROUND = false>
__global__ __launch_bounds__(1024) void batch_fused_kernel(BatchFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tq[];      // 16 swizzled rows of D doubles (+ 32 of slack)
    constexpr int D = CH * 256, CE = 16 * P, NCHUNK = D / CE;       // a chunk = P pieces of 16 elements
    // the ring holds 64 VGPRs of features per lane (fp16 rows: 64 where the vector divides into four 128-element buffers, else 32)
    constexpr int NBUF = sizeof(T) == 2 ? (NCHUNK % (32 / P) == 0 ? 32 / P : 16 / P) : (sizeof(T) == 4 ? 16 : 8) / P;
    constexpr int KL = sizeof(T) == 2 ? 8 : 4;                       // consecutive elements a k-lane holds per load
    static_assert(NCHUNK % NBUF == 0, "chunk ring must divide the vector");
    const int lane = threadIdx.x & 63, col = lane & 15, kk = lane >> 4;
    // everything that indexes tiles is wave-uniform: kept on the scalar unit (the register budget of 4 waves per SIMD is
    // the ring of chunk buffers + the per-tile sums)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int NV = a.S * a.E;
    const int64_t ntiles = (a.n + 15) / 16;
    const int64_t per_round = (int64_t)gridDim.x * 16 * TW;
    const int rounds = (int)((ntiles + per_round - 1) / per_round);
    const int64_t clip_elems = (int64_t)NV * D;
    const T* feats = static_cast<const T*>(a.feats);
    const double* tb = tq + query_row(col, D) + 4 * kk;               // this lane's query (B operand column), its k quarter
    for (int i = threadIdx.x; i < kBatchSlots * D; i += blockDim.x) {  // slots beyond Q stay zero for the whole pass
        const int q = i / D, k = i - q * D;
        if (q >= a.Q) tq[query_row(q, D) + k] = 0.0;
    }
    // tile j of this wave in round r (scalar), and how many of its TW tiles exist (a prefix: the tiles grow with j)
    auto tile_of = [&](int r, int j) -> int64_t { return (int64_t)r * per_round + (int64_t)(wv * TW + j) * gridDim.x + blockIdx.x; };
    auto valid_in = [&](int r) -> int {
        int nv = 0;
        for (int j = 0; j < TW; ++j) nv += (r < rounds && tile_of(r, j) < ntiles) ? 1 : 0;
        return nv;
    };
    // a tile's slice = a scalar base + this lane's 32-bit element offset (its clip row, its k quarter); rows past n re-read the
    // last clip and are never stored
    // TILED: a.feats is the tile-interleaved mirror [tile][slice][k / 4][16 clips][4] (mirror_build_kernel): element (clip, k) of a
    // (tile, slice) block sits at (k / 4) * 64 + clip * 4 + k % 4, so the lane that owns (clip col, k quarter kk) reads piece m of chunk c
    // at ((c P + m) * 4 + kk) * 64 + col * 4 -- the same k = 16 (c P + m) + 4 kk + e as in the row-major form: same operands, same bits.
    constexpr int CSTEP = TILED ? 256 * P : CE;
    auto base_of = [&](int64_t tile, int v) -> const T* {
        return TILED ? feats + (tile * NV + v) * 16 * D : feats + tile * 16 * clip_elems + (int64_t)v * D;
    };
    auto lane_off = [&](int64_t tile) -> uint32_t {
        // units of U = 16 / sizeof(T) elements (4 floats, 2 doubles, 8 halves), 16 U apart along k; a k-lane's KL elements are KL / U units
        if (TILED) return (uint32_t)(kk * 16 * KL + col * vq::tile_unit_of((int)sizeof(T)));
        const int last = (int)min((int64_t)15, a.n - 1 - tile * 16);
        return (uint32_t)(min(col, last) * (int)clip_elems + KL * kk);
    };
    ChunkP<T, P> buf[NBUF];
    if (valid_in(0) > 0) {
        const T* x0 = base_of(tile_of(0, 0), 0) + lane_off(tile_of(0, 0));
#pragma unroll
        for (int bq = 0; bq < NBUF; ++bq) {
            if (TILED) buf[bq].load_tiled(x0 + CSTEP * bq);
            else buf[bq].load(x0 + CSTEP * bq);
        }
    }
    for (int r = 0; r < rounds; ++r) {
        const int nval = valid_in(r), nval_next = valid_in(r + 1);
        doublex4 miss[TW];                                            // sum over closed streams of (w_s (1 - avg_s))^2
#pragma unroll
        for (int j = 0; j < TW; ++j) miss[j] = {0.0, 0.0, 0.0, 0.0};
        double denom = 0.0;
        for (int s = 0; s < a.S; ++s) {
            doublex4 ssum[TW];
            int cnt[TW][4];
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                ssum[j] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) cnt[j][rr] = 0;
            }
            for (int e = 0; e < a.E; ++e) {
                const int v = s * a.E + e;
                __syncthreads();                                      // every wave is done with the previous slice's rows
                for (int i = threadIdx.x; i < a.Q * D; i += blockDim.x) {
                    const int q = i / D, k = i - q * D;
                    tq[query_row(q, D) + batch_query_pos<T>(k)] = a.t[((size_t)q * NV + v) * D + k];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    if (j >= nval) continue;                          // wave-uniform
                    const int64_t tile = tile_of(r, j);
                    const T* x = base_of(tile, v) + lane_off(tile);
                    // the wave's next (tile, slice): next tile of this slice, first tile of the next slice, first of the next round
                    // (after the wave's very last one the ring is refilled from the lines just read: the refill stays
                    // unconditional -- a branch around it makes the compiler drain the whole ring at every loop head)
                    int64_t tn = tile;
                    int vn = v;
                    if (j + 1 < nval) tn = tile_of(r, j + 1);
                    else if (v + 1 < NV) { tn = tile_of(r, 0); vn = v + 1; }
                    else if (nval_next > 0) { tn = tile_of(r + 1, 0); vn = 0; }
                    const T* xn = base_of(tn, vn) + lane_off(tn);
                    doublex4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
                    for (int ch0 = 0; ch0 < NCHUNK; ch0 += NBUF) {
                        const T* src = ch0 + NBUF < NCHUNK ? x + CSTEP * (ch0 + NBUF) : xn;
#pragma unroll
                        for (int bq = 0; bq < NBUF; ++bq) {
                            int off = CE * (ch0 + bq);
                            // the query rows of a slice do not change while a wave walks its tiles: the compiler would hoist all the LDS
                            // reads of a tile out of the tile loop (512 registers: spilled); an opaque offset keeps every read next to its MFMA
                            asm volatile("" : "+v"(off));
                            const double* tbc = tb + off;
#pragma unroll
                            for (int m = 0; m < P; ++m)
#pragma unroll
                                for (int ee = 0; ee < 4; ++ee)
                                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(buf[bq].at(m, ee), tbc[16 * m + ee], acc, 0, 0, 0);
                            if (TILED) buf[bq].load_tiled(src + CSTEP * bq);
                            else buf[bq].load(src + CSTEP * bq);
                        }
                    }
                    // ticket.py:155-160: the mean runs over the splits PRESENT for the clip
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        bool here = true;
                        if (PRES) {
                            const int64_t cc = min(tile * 16 + kk + 4 * rr, a.n - 1);
                            here = a.present[(cc * a.S + s) * a.E + e] != 0;
                        }
                        if (here) {
                            ssum[j][rr] = ssum[j][rr] + acc[rr];
                            if (PRES) ++cnt[j][rr];
                        }
                    }
                }
            }
            // the stream closes: avg = sum / count, then the terms of ticket.py:172-180 in stream order
            const double ws = col < a.Q ? a.w[col * (ROUND ? 8 : a.S) + s] : 0.0;
            denom = denom + ws * ws;
            // ROUND: the addresses of the avg stores do not depend on the stream, so the compiler would compute them once per round and keep
            // them (16 VGPRs) alive through the MFMA loop; an opaque lane offset makes it compute them here, where the stream closes
            [[maybe_unused]] int kko = kk;
            if constexpr (ROUND) asm volatile("" : "+v"(kko));
#pragma unroll
            for (int j = 0; j < TW; ++j)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const double av = ssum[j][rr] / (double)(PRES ? cnt[j][rr] : a.E);
                    if (ROUND) {                                      // the tile exists (wave-uniform), the query is in use, the row is inside n
                        const int64_t cc = tile_of(r, j) * 16 + kko + 4 * rr;
                        if (j < nval && col < a.Q && cc < a.n) a.avg[((int64_t)col * a.n + cc) * a.S + s] = av;
                    }
                    const double term = ws * (1.0 - av);
                    miss[j][rr] = miss[j][rr] + term * term;
                }
        }
        if (col < a.Q) {
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                if (j >= nval) continue;
                const int64_t tile = tile_of(r, j);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int64_t cc = tile * 16 + kk + 4 * rr;
                    if (cc < a.n) a.scores[(int64_t)col * a.n + cc] = 1.0 - sqrt(miss[j][rr] / denom);
                }
            }
        }
    }
}

// batch_fused_kernel<..., ROUND = true> over the UNION of the round's row views (BatchViewArgs).  It is a kernel of its own, the walk of
// batch_fused_kernel restated line for line, so that every existing instantiation keeps its code unchanged (the register allocation of
// those kernels, which spill at 4 waves per SIMD, moves with any edit of their source); what differs is marked VIEW below.
// The tiles are VIRTUAL -- 16 consecutive rows of the union, gathered (a lane's address is 64-bit: sixteen arbitrary rows can lie more
// than 2^32 elements apart) -- or, TILED, the touched tiles read whole.  The rows of a tile come in with ONE scalar load (the list is
// padded to whole tiles) and a lane picks its own with selects; the lane's pointer for the wave's NEXT (tile, slice) is made while the
// current one is multiplied and carried over, so no index load ever waits between feature loads.  The mask is read by database row; a
// store for (query, clip) goes to start[q] + the clip's position in that query's view and is skipped for a clip outside it.  The MFMA
// sequence per (clip, query) is batch_fused_kernel's: which tile, or which row of a tile, a clip occupies does not enter an output element
// of v_mfma_f64_16x16x4, so avg and scores have the bits of vq_db_query_round_batch.
template <typename T, int CH, int TW, bool PRES, int P, bool TILED = false>
__global__ __launch_bounds__(1024) void batch_view_kernel(BatchViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tq[];      // 16 swizzled rows of D doubles (+ 32 of slack)
    constexpr int D = CH * 256, CE = 16 * P, NCHUNK = D / CE;
    constexpr int NBUF = sizeof(T) == 2 ? (NCHUNK % (32 / P) == 0 ? 32 / P : 16 / P) : (sizeof(T) == 4 ? 16 : 8) / P;
    constexpr int KL = sizeof(T) == 2 ? 8 : 4;
    static_assert(NCHUNK % NBUF == 0, "chunk ring must divide the vector");
    const int lane = threadIdx.x & 63, col = lane & 15, kk = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int NV = a.S * a.E;
    const ViewWalk<T, TILED, KL> vw(a, static_cast<const T*>(a.feats), NV, D, col, kk);       // VIEW
    const int64_t ntiles = vw.ntiles;                                 // VIEW: the work items of the plan
    const int64_t per_round = (int64_t)gridDim.x * 16 * TW;
    const int rounds = (int)((ntiles + per_round - 1) / per_round);
    const double* tb = tq + query_row(col, D) + 4 * kk;
    for (int i = threadIdx.x; i < kBatchSlots * D; i += blockDim.x) {
        const int q = i / D, k = i - q * D;
        if (q >= a.Q) tq[query_row(q, D) + k] = 0.0;
    }
    auto tile_of = [&](int r, int j) -> int64_t { return (int64_t)r * per_round + (int64_t)(wv * TW + j) * gridDim.x + blockIdx.x; };
    auto valid_in = [&](int r) -> int {
        int nv = 0;
        for (int j = 0; j < TW; ++j) nv += (r < rounds && tile_of(r, j) < ntiles) ? 1 : 0;
        return nv;
    };
    constexpr int CSTEP = TILED ? 256 * P : CE;
    ChunkP<T, P> buf[NBUF];
    const T* xcur = vw.feats;                                         // VIEW: this lane's pointer for the wave's current (tile, slice)
    if (valid_in(0) > 0) {
        xcur = vw.ptr(tile_of(0, 0), 0);
#pragma unroll
        for (int bq = 0; bq < NBUF; ++bq) {
            if (TILED) buf[bq].load_tiled(xcur + CSTEP * bq);
            else buf[bq].load(xcur + CSTEP * bq);
        }
    }
    for (int r = 0; r < rounds; ++r) {
        const int nval = valid_in(r), nval_next = valid_in(r + 1);
        doublex4 miss[TW];
#pragma unroll
        for (int j = 0; j < TW; ++j) miss[j] = {0.0, 0.0, 0.0, 0.0};
        double denom = 0.0;
        for (int s = 0; s < a.S; ++s) {
            doublex4 ssum[TW];
            int cnt[TW][4];
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                ssum[j] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) cnt[j][rr] = 0;
            }
            for (int e = 0; e < a.E; ++e) {
                const int v = s * a.E + e;
                __syncthreads();
                for (int i = threadIdx.x; i < a.Q * D; i += blockDim.x) {
                    const int q = i / D, k = i - q * D;
                    tq[query_row(q, D) + batch_query_pos<T>(k)] = a.t[((size_t)q * NV + v) * D + k];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    if (j >= nval) continue;
                    const int64_t tile = tile_of(r, j);
                    const T* x = xcur;                                // VIEW: made one step ago
                    int64_t tn = tile;
                    int vn = v;
                    if (j + 1 < nval) tn = tile_of(r, j + 1);
                    else if (v + 1 < NV) { tn = tile_of(r, 0); vn = v + 1; }
                    else if (nval_next > 0) { tn = tile_of(r + 1, 0); vn = 0; }
                    const T* xn = xcur = vw.ptr(tn, vn);              // VIEW: what the next step of this wave walks
                    doublex4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
                    for (int ch0 = 0; ch0 < NCHUNK; ch0 += NBUF) {
                        const T* src = ch0 + NBUF < NCHUNK ? x + CSTEP * (ch0 + NBUF) : xn;
#pragma unroll
                        for (int bq = 0; bq < NBUF; ++bq) {
                            int off = CE * (ch0 + bq);
                            asm volatile("" : "+v"(off));             // keeps every LDS read next to its MFMA (batch_fused_kernel)
                            const double* tbc = tb + off;
#pragma unroll
                            for (int m = 0; m < P; ++m)
#pragma unroll
                                for (int ee = 0; ee < 4; ++ee)
                                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(buf[bq].at(m, ee), tbc[16 * m + ee], acc, 0, 0, 0);
                            if (TILED) buf[bq].load_tiled(src + CSTEP * bq);
                            else buf[bq].load(src + CSTEP * bq);
                        }
                    }
                    [[maybe_unused]] ViewTile pvt;
                    if constexpr (PRES) pvt = vw.tile(tile);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        bool here = true;
                        if (PRES) here = a.present[(vw.mask_row(pvt, kk + 4 * rr) * a.S + s) * a.E + e] != 0;      // VIEW: by database row
                        if (here) {
                            ssum[j][rr] = ssum[j][rr] + acc[rr];
                            if (PRES) ++cnt[j][rr];
                        }
                    }
                }
            }
            const double ws = col < a.Q ? a.w[col * 8 + s] : 0.0;
            denom = denom + ws * ws;
            int kko = kk;
            asm volatile("" : "+v"(kko));                             // the store addresses are made here, where the stream closes (batch_fused_kernel)
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                ViewTile vt = {};
                if (j < nval) vt = vw.tile(tile_of(r, j));
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const double av = ssum[j][rr] / (double)(PRES ? cnt[j][rr] : a.E);
                    if (j < nval) {                                   // VIEW: to the clip's position in this lane's query's view, if it has one
                        const int64_t o = vw.entry(vt, kko + 4 * rr);
                        if (o >= 0) a.avg[o * a.S + s] = av;
                    }
                    const double term = ws * (1.0 - av);
                    miss[j][rr] = miss[j][rr] + term * term;
                }
            }
        }
        if (col < a.Q) {
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                if (j >= nval) continue;
                const ViewTile vt = vw.tile(tile_of(r, j));
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int64_t o = vw.entry(vt, kk + 4 * rr);      // VIEW
                    if (o >= 0) a.scores[o] = 1.0 - sqrt(miss[j][rr] / denom);
                }
            }
        }
    }
}

// the instantiation of the 16-query pass for a database (fp16: the tiled branch exists at D = 1024 only, the one shape that can be tiled)
template <typename T, int CH, int TW, bool ROUND = false>
static auto fused_kernel_for(bool pres, bool tiled) -> void (*)(BatchFusedArgs) {
    if constexpr (sizeof(T) != 2 || CH == 4) {
        if (tiled) return pres ? batch_fused_kernel<T, CH, TW, true, 8, true, ROUND> : batch_fused_kernel<T, CH, TW, false, 8, true, ROUND>;
    }
    return pres ? batch_fused_kernel<T, CH, TW, true, 8, false, ROUND> : batch_fused_kernel<T, CH, TW, false, 8, false, ROUND>;
}

// One 16-query pass over the whole database on the handle's stream: d_t [Q][NV][D], d_w [Q][S] -> d_scores [Q][n].  ROUND: d_w is
// [Q][8] and the stream means also go to d_avg [Q][n][S] (vq_db_query_round_batch).  Caller holds the lock and has checked the shape.
template <bool ROUND>
static int launch_fused_pass(vq_db* db, int Q, const double* d_t, const double* d_w, double* d_scores, double* d_avg) {
    const size_t lds = ((size_t)kBatchSlots * db->D + 32) * 8;   // sixteen swizzled query rows
    const bool tiled = db->tiled();                        // whole 128-byte lines per load instruction, non-temporal: 0.75 of the HBM peak against 0.71
    BatchFusedArgs f;
    f.feats = db->feats;
    f.t = d_t;
    f.w = d_w;
    f.present = db->present;
    f.scores = d_scores;
    f.n = db->n;
    f.Q = Q;
    f.S = db->S;
    f.E = db->E;
    f.D = db->D;
    f.avg = d_avg;
    constexpr int TW = 2;                                     // tiles of 16 clips per wave and round
    // chunks of 8 pieces = 128 elements: a refill reads 512 contiguous bytes of each of the 16 clips (two ring buffers).  With 64-
    // element chunks and four buffers the pass took 7.60 ms instead of 7.45 at cfg 4 (65 k slow streams of 256-byte reads)
    const int64_t ntiles = (db->n + 15) / 16;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + 16 * TW - 1) / (16 * TW), (int64_t)db->cus));
    // every (T, CH, mask) is launched by CASES of tests/test_batch_round_gpu.py (the table above it): a new one gets a new case there
    const int rc = with_dtype(db, [&](auto x) {
        return with_chunks(db, [&](auto ch) -> int {
            constexpr int CH = decltype(ch)::value;
            auto kern = fused_kernel_for<decltype(x), CH, TW, ROUND>((bool)db->present, tiled);
            VQ_DYN_LDS(kern, (kBatchSlots * CH * 256 + 32) * 8);
            kern<<<blocks, 1024, lds, db->stream>>>(f);
            return VQ_OK;
        });
    });
    if (rc != VQ_OK) return rc;
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_round_pass(vq_db* db, int Q, const double* d_t, const double* d_w, double* d_scores, double* d_avg) {
    return launch_fused_pass<true>(db, Q, d_t, d_w, d_scores, d_avg);
}

extern "C" {

int vq_db_scan_batch(vq_db* db, int32_t n_queries, const double* t_host, const double* w_host, double* scores_host) {
    VQ_REQUIRE(db && t_host && w_host, "NULL argument");
    VQ_REQUIRE(n_queries >= 1 && n_queries <= kBatchSlots, "n_queries must be in [1,%d] (got %d)", kBatchSlots, n_queries);
    VQ_REQUIRE(db->D % 256 == 0 && db->D <= 1024, "batched scan needs D in {256,512,768,1024} (got %d)", db->D);
    VQ_REQUIRE(db->S <= 8, "at most 8 streams");
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->active >= 0) return fail(VQ_E_UNSUPPORTED, "vq_db_scan_batch runs over the whole database: row view %d is in use (vq_db_rows_use(db, -1) first)", db->active);
    DeviceGuard g(db->device);
    const int Q = n_queries, NV = db->S * db->E;
    const int64_t n_t = (int64_t)Q * NV * db->D, n_w = (int64_t)Q * db->S, n_sc = (int64_t)Q * db->n;
    VQ_HIP(db->batch_buf.grow((size_t)(n_t + n_w + n_sc) * 8));
    double* d_t = db->batch_buf;
    double* d_w = d_t + n_t;
    double* d_scores = d_w + n_w;
    db->batch_scores = d_scores;
    VQ_HIP(hipMemcpyAsync(d_t, t_host, (size_t)n_t * 8, hipMemcpyHostToDevice, db->stream));
    VQ_HIP(hipMemcpyAsync(d_w, w_host, (size_t)n_w * 8, hipMemcpyHostToDevice, db->stream));
    {
        const int rc = launch_fused_pass<false>(db, Q, d_t, d_w, d_scores, nullptr);
        if (rc != VQ_OK) return rc;
    }
    db->batch_q = Q;
    if (scores_host) {
        VQ_HIP(hipMemcpyAsync(scores_host, d_scores, (size_t)n_sc * 8, hipMemcpyDeviceToHost, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    return VQ_OK;
}

int vq_db_batch_scores_devptr(vq_db* db, void** dev_ptr, int32_t* n_queries) {
    VQ_REQUIRE(db && dev_ptr, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->batch_q == 0) return fail(VQ_E_STATE, "no batched scan has run");
    *dev_ptr = db->batch_scores;
    if (n_queries) *n_queries = db->batch_q;
    return VQ_OK;
}

}  // extern "C"

// ---- the pass of a batched round over a row view per query (csrc/vq_rounds.hip, include/vq_amd_round_views.h) -------------------------
// the VIEW instantiation of the 16-query pass for a database: the tiled layouts exist for rows of 1024 elements only (vq_db_set_layout)
template <typename T, int CH, int TW>
static auto view_kernel_for(bool pres, bool tiled) -> void (*)(BatchViewArgs) {
    if constexpr (CH == 4) {
        if (tiled) return pres ? batch_view_kernel<T, CH, TW, true, 8, true> : batch_view_kernel<T, CH, TW, false, 8, true>;
    }
    return pres ? batch_view_kernel<T, CH, TW, true, 8, false> : batch_view_kernel<T, CH, TW, false, 8, false>;
}

// One pass over the union of the round's views.  max_tiles bounds the tiles the plan can hold (the kernel reads their number from the
// device): it only sizes the grid.  Caller holds the lock and has checked the shape.
int vq::launch_view_pass(vq_db* db, BatchViewArgs f, int64_t max_tiles) {
    const size_t lds = ((size_t)kBatchSlots * db->D + 32) * 8;
    const bool tiled = db->tiled();
    if (tiled && db->D != 1024) return fail(VQ_E_UNSUPPORTED, "a tiled database holds rows of 1024 elements (float32, float64 or float16)");
    constexpr int TW = 2;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((max_tiles + 16 * TW - 1) / (16 * TW), (int64_t)db->cus));
    // every (T, CH, mask, layout) is launched by a case of tests/test_view_round_gpu.py (the table above VIEW_KERNELS there): a new one
    // gets a new case there (the tiled forms of fp64 and fp16: tests/test_tiled64_gpu.py, tests/test_tiled16_gpu.py)
    const int rc = with_dtype(db, [&](auto x) {
        return with_chunks(db, [&](auto ch) -> int {
            constexpr int CH = decltype(ch)::value;
            auto kern = view_kernel_for<decltype(x), CH, TW>((bool)db->present, tiled);
            VQ_DYN_LDS(kern, (kBatchSlots * CH * 256 + 32) * 8);
            kern<<<blocks, 1024, lds, db->stream>>>(f);
            return VQ_OK;
        });
    });
    if (rc != VQ_OK) return rc;
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}
