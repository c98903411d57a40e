// Hot path B on gfx950: the one-query similarity scan over a resident feature DB (the handle: csrc/vq_db.hip; the 16-query passes:
// csrc/vq_sim_batch.hip; scoring again, selection, top-k: csrc/vq_rank.hip).
//
// Reference semantics restated here (paths relative to the reference checkout):
//   src/models/ticket.py:120-163   compute_similarities  -> scan_kernel
//   src/models/ticket.py:165-180   compute_scores        -> score_from_avg (scan epilogue)
//
// The scan is an HBM-bound stream (2 FLOP per 4 bytes): every clip's S*E vectors are read exactly
// once with 16-byte coalesced loads, multiplied against the fp64 query held in LDS, accumulated in
// fp64 per lane and reduced across the 64-lane wavefront.  This file is compiled with
// -ffp-contract=off: the score arithmetic must round exactly like the reference's numpy scalars;
// fused multiply-adds are written explicitly where they are wanted (the dot products).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "vq_db.h"
#include "vq_score.h"

using namespace vq;

// LDS image of the query: element k of vector v lives at lds_index(v, k).  Inside each 256-element
// chunk the two 16-byte halves of a lane's 4 doubles are stored in separate lane-linear planes, so
// both ds_read_b128 of a wave are 64 x 16 contiguous bytes (bank-conflict free).
__device__ __forceinline__ int t_lds_index(int D, int v, int k) {
    const int j = k >> 8, r = k & 255, lane = r >> 2, q = r & 3;
    return v * D + (j << 8) + ((q >> 1) << 7) + (lane << 1) + (q & 1);
}

// The same image for a lane that holds 8 consecutive elements of a 512-element chunk (fp16 rows: 16 bytes per lane, 1 KB per wave
// instruction): four lane-linear planes of 128 doubles per chunk, plane q / 2 holds elements q = 2 (q / 2), 2 (q / 2) + 1 of every lane.
__device__ __forceinline__ int t_lds_index8(int D, int v, int k) {
    const int j = k >> 9, r = k & 511, lane = r >> 3, q = r & 7;
    return v * D + (j << 9) + ((q >> 1) << 7) + (lane << 1) + (q & 1);
}

template <typename T>
struct Quad;
template <>
struct Quad<__half> {                  // scan_generic_kernel: 8-byte loads
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 v;
    __device__ __forceinline__ void load(const __half* p) { v = __builtin_nontemporal_load(reinterpret_cast<const h4*>(p)); }
    __device__ __forceinline__ double x0() const { return half_to_double(v.x); }
    __device__ __forceinline__ double x1() const { return half_to_double(v.y); }
    __device__ __forceinline__ double x2() const { return half_to_double(v.z); }
    __device__ __forceinline__ double x3() const { return half_to_double(v.w); }
};
template <>
struct Quad<float> {
    float4 v;
    __device__ __forceinline__ void load(const float* p) { v = stream_load4(p); }
    __device__ __forceinline__ double x0() const { return (double)v.x; }
    __device__ __forceinline__ double x1() const { return (double)v.y; }
    __device__ __forceinline__ double x2() const { return (double)v.z; }
    __device__ __forceinline__ double x3() const { return (double)v.w; }
};
template <>
struct Quad<double> {
    double2 a, b;
    __device__ __forceinline__ void load(const double* p) {
        const vq_d2 lo = __builtin_nontemporal_load(reinterpret_cast<const vq_d2*>(p));
        const vq_d2 hi = __builtin_nontemporal_load(reinterpret_cast<const vq_d2*>(p + 2));
        a = make_double2(lo.x, lo.y);
        b = make_double2(hi.x, hi.y);
    }
    __device__ __forceinline__ double x0() const { return a.x; }
    __device__ __forceinline__ double x1() const { return a.y; }
    __device__ __forceinline__ double x2() const { return b.x; }
    __device__ __forceinline__ double x3() const { return b.y; }
};

// What a lane of scan_kernel holds of one wave instruction (1 KB of contiguous memory) and its share of the dot: N consecutive elements of
// a chunk of 64 N, against the planes of the LDS image of that chunk (tc = the chunk's image + 2 lane: every read is 64 x 16 contiguous bytes).
template <typename T>
struct LaneVec : Quad<T> {             // fp32: one 16-byte load, fp64: two; 4 elements of a 256-chunk
    static constexpr int N = 4;
    static __device__ __forceinline__ int lds_index(int D, int v, int k) { return t_lds_index(D, v, k); }
    __device__ __forceinline__ double dot(const double* tc, double p) const {
        const double2 ta = *reinterpret_cast<const double2*>(tc);
        const double2 tb = *reinterpret_cast<const double2*>(tc + 128);
        p = fma(this->x0(), ta.x, p);
        p = fma(this->x1(), ta.y, p);
        p = fma(this->x2(), tb.x, p);
        p = fma(this->x3(), tb.y, p);
        return p;
    }
};
template <>
struct LaneVec<__half> {               // fp16: one 16-byte load = 8 elements of a 512-chunk; per element cvt f16->f32, cvt f32->f64, fp64 FMA
    static constexpr int N = 8;
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 v;
    static __device__ __forceinline__ int lds_index(int D, int v, int k) { return t_lds_index8(D, v, k); }
    __device__ __forceinline__ void load(const __half* p) { v = __builtin_nontemporal_load(reinterpret_cast<const h8*>(p)); }
    __device__ __forceinline__ double dot(const double* tc, double p) const {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double2 tg = *reinterpret_cast<const double2*>(tc + 128 * g);
            p = fma(half_to_double(v[2 * g]), tg.x, p);
            p = fma(half_to_double(v[2 * g + 1]), tg.y, p);
        }
        return p;
    }
};

struct ScanArgs {
    const void* feats;
    const double* t;          // [NV][D] natural order, global
    const uint8_t* present;   // [N][S][E] or null
    const double* w;          // [S] or null
    double* sims;             // [N][S][E] or null
    double* avg;              // [N][S]
    int32_t* ne;              // [N][S]
    double* scores;           // [N] (written only if w)
    int64_t n;
    int32_t S, E, D;
};

// A row view (vq_db_rows_define / vq_db_rows_use): the one-query scan over M chosen rows of the database, in database order, as if it
// held only those.  Work item i of the row-major kernels reads clip items[i] and writes avg / ne / sims / scores at POSITION i (n = M: the
// result arrays are compact); the presence mask stays indexed by database row.  A tiled database cannot gather rows (a clip is 16-byte
// pieces of its tile): there work item i is the touched tile items[i], read whole as ever, and lane (clip j of the tile) stores only if
// pos[16 i + j] >= 0 -- its clip's position in the view (n stays the database's N there, n_items = touched tiles).  The arithmetic per clip
// is the full scan's, operation for operation: a clip scores the same bits under a view.
struct ScanViewArgs : ScanArgs {
    const int64_t* items;     // [M] rows, strictly ascending | tiled: [n_items] touched tiles, ascending
    const int64_t* pos;       // tiled: [n_items][16] position in the view, or -1
    int64_t n_items;          // M | touched tiles
};

// Per-clip bookkeeping, carried by every lane (wave-uniform values): ensemble mean
// (ticket.py:155-160: sequential sum over the splits present, divided by their count) and the
// weighted score (ticket.py:172-180).
struct ClipAcc {
    double acc = 0.0;
    int cnt = 0;
    double av[8];
};

__device__ __forceinline__ void clip_add(const ScanArgs& a, ClipAcc& st, int64_t c, int s, int e, double sim, int lane) {
    const int64_t idx = (c * a.S + s) * a.E + e;
    const bool p = a.present ? a.present[idx] != 0 : true;
    if (p) {
        st.acc = st.acc + sim;
        ++st.cnt;
    }
    if (a.sims && lane == 0) a.sims[idx] = sim;
}

// the same under a row view: the presence bits are the database row's, the result goes to the position in the view
__device__ __forceinline__ void clip_add_view(const ScanArgs& a, ClipAcc& st, int64_t pos, int64_t row, int s, int e, double sim, int lane) {
    const bool p = a.present ? a.present[(row * a.S + s) * a.E + e] != 0 : true;
    if (p) {
        st.acc = st.acc + sim;
        ++st.cnt;
    }
    if (a.sims && lane == 0) a.sims[(pos * a.S + s) * a.E + e] = sim;
}

__device__ __forceinline__ double clip_close_stream(const ScanArgs& a, ClipAcc& st, int64_t c, int s, int lane) {
    const double m = st.acc / (double)st.cnt;
    if (lane == 0) {
        a.avg[c * a.S + s] = m;
        a.ne[c * a.S + s] = st.cnt;
    }
    st.acc = 0.0;
    st.cnt = 0;
    return m;
}

// One wavefront per clip, grid-strided.  S streams x E splits per clip and CH = D/256 (fp16 rows: D/512 wave instructions per
// vector, LaneVec) are compile-time, so every index is static and everything stays in registers.  The next
// vector (possibly of the wave's next clip) is in flight while the current one is multiplied, so
// every wave keeps 2 x CH x 1 KiB of HBM reads outstanding.
// LEAN (round 6): left alone, the compiler keeps the WHOLE query slice of a lane in registers across clips (the LDS reads do not depend on
// the clip: 192-320 VGPRs, one wave per SIMD) -- right for a database of a million clips, where every wave streams for milliseconds, and wrong
// for one of ten thousand (configs[0]: three clips per wave), whose scan then runs at 4.3 TB/s with 4 waves per compute unit in flight.  The
// LEAN instantiation re-reads the query from LDS for every clip and fits three waves per SIMD (what the 48 KB LDS image allows per unit).
// VIEW: c walks the positions of a row view and r is the database row read (ScanViewArgs).  The position is kept wave-uniform on the
// scalar unit, so the row list is read with scalar loads: they do not enter the in-order vector-memory queue, whose waits stay those of the
// plain scan (a vector index load between the feature loads made the compiler drain the queue once per clip: 4-5 % of the scan).  The
// row of the item after the next is fetched a whole clip before its address is needed (index clamped, no branch), so the prefetch of
// the next clip never waits on an index load.
template <typename T, int S, int E, int CH, bool LEAN = false, bool VIEW = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LEAN ? 3 : 1, LEAN ? 3 : 8))) void scan_kernel(
    std::conditional_t<VIEW, ScanViewArgs, ScanArgs> a) {
    extern __shared__ __attribute__((aligned(16))) double t_lds[];
    constexpr int NV = S * E;
    constexpr int D = CH * 256;
    using V = LaneVec<T>;
    constexpr int CW = 64 * V::N, NCH = D / CW;                        // elements of a wave instruction, instructions per vector
    for (int i = threadIdx.x; i < NV * D; i += blockDim.x) t_lds[V::lds_index(D, i / D, i % D)] = a.t[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const T* feats = static_cast<const T*>(a.feats);
    constexpr int64_t clip_elems = (int64_t)NV * D;
    double w[S];
    if (a.w) {
#pragma unroll
        for (int s = 0; s < S; ++s) w[s] = a.w[s];
    }

    V cur[NCH], nxt[NCH];
    int64_t c = wave;
    int64_t r = 0, rn = 0;                                             // VIEW: the rows of item c and of item c + nwaves
    if constexpr (VIEW) {
        c = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (c < a.n) {
            r = a.items[c];
            rn = a.items[min(c + nwaves, a.n - 1)];
        }
    }
    if (c < a.n) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) cur[j].load(feats + (VIEW ? r : c) * clip_elems + j * CW + lane * V::N);
    }
    while (c < a.n) {
        if constexpr (LEAN) asm volatile("" ::: "memory");             // the query fragments are read again, not carried over
        const int64_t cn = c + nwaves;
        int64_t rnn = 0;
        if constexpr (VIEW) rnn = a.items[min(cn + nwaves, a.n - 1)];  // needed one clip from now
        ClipAcc st;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const T* nb = (v + 1 < NV) ? feats + (VIEW ? r : c) * clip_elems + (int64_t)(v + 1) * D
                                       : (cn < a.n ? feats + (VIEW ? rn : cn) * clip_elems : nullptr);
            if (nb) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) nxt[j].load(nb + j * CW + lane * V::N);
            }
            double p = 0.0;
#pragma unroll
            for (int j = 0; j < NCH; ++j) p = cur[j].dot(&t_lds[v * D + j * CW + lane * 2], p);
            if constexpr (VIEW) clip_add_view(a, st, c, r, v / E, v % E, wave_sum(p), lane);
            else clip_add(a, st, c, v / E, v % E, wave_sum(p), lane);
            if (v % E == E - 1) st.av[v / E] = clip_close_stream(a, st, c, v / E, lane);
#pragma unroll
            for (int j = 0; j < NCH; ++j) cur[j] = nxt[j];
        }
        if (a.w && lane == 0) a.scores[c] = score_from_avg(st.av, w, S);
        c = cn;
        if constexpr (VIEW) {
            r = rn;
            rn = rnn;
        }
    }
}

// Any shape with D % 4 == 0: runtime loops, query read from global memory (L2-resident).
template <typename T, bool VIEW = false>
__global__ __launch_bounds__(256) void scan_generic_kernel(std::conditional_t<VIEW, ScanViewArgs, ScanArgs> a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const T* feats = static_cast<const T*>(a.feats);
    const int NV = a.S * a.E, D = a.D;
    double w[8];
    if (a.w)
        for (int s = 0; s < a.S; ++s) w[s] = a.w[s];
    int64_t c0 = wave;
    if constexpr (VIEW) c0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t c = c0; c < a.n; c += nwaves) {
        int64_t r = c;                                                 // the row read; c stays where the results go
        if constexpr (VIEW) r = a.items[c];
        ClipAcc st;
        for (int s = 0; s < a.S; ++s) {
            for (int e = 0; e < a.E; ++e) {
                const int v = s * a.E + e;
                const T* x = feats + (r * NV + v) * (int64_t)D;
                const double* t = a.t + (int64_t)v * D;
                double p = 0.0;
                for (int k = lane * 4; k < D; k += 256) {
                    Quad<T> q;
                    q.load(x + k);
                    p = fma(q.x0(), t[k + 0], p);
                    p = fma(q.x1(), t[k + 1], p);
                    p = fma(q.x2(), t[k + 2], p);
                    p = fma(q.x3(), t[k + 3], p);
                }
                if constexpr (VIEW) clip_add_view(a, st, c, r, s, e, wave_sum(p), lane);
                else clip_add(a, st, c, s, e, wave_sum(p), lane);
            }
            const double m = clip_close_stream(a, st, c, s, lane);
            // runtime-indexed store into a small per-lane array; the generic path is not the fast path
            st.av[s] = m;
        }
        if (a.w && lane == 0) a.scores[c] = score_from_avg(st.av, w, a.S);
    }
}

// score_from_avg with the stream count a constant of each call: the loop over av / w unrolls and both stay in registers (the same
// operations in the same order whichever the case)
__device__ __forceinline__ double score_from_avg_streams(const double* av, const double* w, int S) {
    switch (S) {
        case 1: return score_from_avg(av, w, 1);
        case 2: return score_from_avg(av, w, 2);
        case 3: return score_from_avg(av, w, 3);
        case 4: return score_from_avg(av, w, 4);
        case 5: return score_from_avg(av, w, 5);
        case 6: return score_from_avg(av, w, 6);
        case 7: return score_from_avg(av, w, 7);
    }
    return score_from_avg(av, w, 8);
}

// Short rows (include/vq_amd_dim.h: handles created with VQ_DIM_SHORT_ROWS, stored D <= 128, rows layout): scan_generic_kernel gives
// a whole wave to one vector -- at D = 104 only 26 of its 64 lanes load -- and reads the query from global memory.  Here a wave
// works on 64 / L clips at once, L = 1 << lg = the smallest power of two >= D / 4 (1 .. 32): lane group lane / L owns clip
// c0 + lane / L, lane j = lane % L holds elements 4 j .. 4 j + 3 of the current vector (nothing when 4 j >= D: its share of the dot
// is +0.0).  The query is an LDS image [NV][D] of doubles in natural order (at most 64 x 128 x 8 = 64 KB: the launch raises the
// limit); lane j reads its four values with two 16-byte reads, every group the same addresses (broadcast).  The next vector
// (possibly of the group's next clip) is in flight while the current one is multiplied and reduced, as in scan_kernel.  A dot is
// summed over the group by __shfl_xor over L / 2 .. 1, which stays inside the group and leaves the sum in every lane of it, so the
// bookkeeping per clip (ClipAcc) is group-uniform and lane j == 0 stores.  A group whose clip is >= n neither loads nor stores.
// VIEW: c walks the positions of a row view, r is the database row read; results go to positions, presence bits are the row's.
template <typename T, bool VIEW = false>
__global__ __launch_bounds__(256) void scan_short_kernel(std::conditional_t<VIEW, ScanViewArgs, ScanArgs> a, int lg) {
    extern __shared__ __attribute__((aligned(16))) double t_lds[];    // [NV][D], natural order
    const int NV = a.S * a.E, D = a.D;
    for (int i = threadIdx.x; i < NV * D; i += blockDim.x) t_lds[i] = a.t[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, L = 1 << lg, G = 64 >> lg;
    const int grp = lane >> lg, j = lane & (L - 1);
    const bool act = 4 * j < D;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * (blockDim.x >> 6) * G;  // clips between two rounds of the grid
    const T* feats = static_cast<const T*>(a.feats) + 4 * j;
    const double* tq = t_lds + 4 * j;
    const int64_t clip_elems = (int64_t)NV * D;
    double w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) w[s] = (a.w && s < a.S) ? a.w[s] : 0.0;

    Quad<T> cur{}, nxt{};
    int64_t c = wave * G + grp;
    bool live = c < a.n;
    int64_t r = c;                                                     // the row read; c stays where the results go
    if constexpr (VIEW) r = live ? a.items[c] : 0;
    if (live && act) cur.load(feats + r * clip_elems);
    for (int64_t c0 = wave * G; c0 < a.n; c0 += step) {                // wave-uniform: every lane takes part in the shuffles
        const int64_t cn = c + step;
        const bool live_n = cn < a.n;
        int64_t rn = cn;
        if constexpr (VIEW) rn = live_n ? a.items[cn] : 0;
        ClipAcc st;
#pragma unroll
        for (int s = 0; s < 8; ++s) st.av[s] = 0.0;
        int s = 0, e = 0;
        for (int v = 0; v < NV; ++v) {
            const bool more = v + 1 < NV;
            const T* nb = more ? feats + r * clip_elems + (int64_t)(v + 1) * D : feats + rn * clip_elems;
            if ((more ? live : live_n) && act) nxt.load(nb);
            double p = 0.0;
            if (act) {
                const double2 ta = *reinterpret_cast<const double2*>(tq + v * D);
                const double2 tb = *reinterpret_cast<const double2*>(tq + v * D + 2);
                p = fma(cur.x0(), ta.x, p);
                p = fma(cur.x1(), ta.y, p);
                p = fma(cur.x2(), tb.x, p);
                p = fma(cur.x3(), tb.y, p);
            }
            if (lg > 4) p += __shfl_xor(p, 16, 64);
            if (lg > 3) p += __shfl_xor(p, 8, 64);
            if (lg > 2) p += __shfl_xor(p, 4, 64);
            if (lg > 1) p += __shfl_xor(p, 2, 64);
            if (lg > 0) p += __shfl_xor(p, 1, 64);
            if (live) {
                if constexpr (VIEW) clip_add_view(a, st, c, r, s, e, p, j);
                else clip_add(a, st, c, s, e, p, j);
            }
            if (++e == a.E) {
                if (live) {
                    const double m = clip_close_stream(a, st, c, s, j);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k == s) st.av[k] = m;
                }
                e = 0;
                ++s;
            }
            cur = nxt;
        }
        if (a.w && live && j == 0) a.scores[c] = score_from_avg_streams(st.av, w, a.S);
        c = cn;
        r = rn;
        live = live_n;
    }
}

// The one-query scan over a TILED database (vq_db_set_layout): [tile of 16 clips][slice][k / 4][clip][4], fp32.  A wave owns a tile:
// lane l = (clip l % 16, k quarter l / 16), and because piece g = 4 i + l / 16 of the slice sits at g * 64 + (l % 16) * 4 floats, load i
// of a lane is at i * 256 + l * 4 -- a wave instruction still takes 1 KB of contiguous memory and a whole tile (all its slices) is ONE
// contiguous run of NV * 64 KB.  A lane multiplies 256 of its clip's 1024 elements per slice (k = 16 i + 4 (l / 16) + 0..3; the
// matching query values are four 32-byte groups per instruction in LDS: broadcast, conflict-free) and the clip's dot is the sum
// over its four lanes: two butterfly steps per 16 clips and slice where the row-major kernel pays six per clip.  G loads of 1 KB
// per wave are in flight behind the G being multiplied.  Same bookkeeping per clip as scan_kernel (ensemble mean over the splits
// present, weighted score); the k order of a dot differs, so the two layouts agree to rounding (<= 1e-12, tested), not bit for bit.
// VIEW: the wave walks the TOUCHED tiles of a row view (item it -> tile items[it]: wave-uniform, scalar loads, the index two items on
// fetched a tile ahead) and a lane stores its clip's results at pos[16 it + col] when that is not -1 (ScanViewArgs; the entry of the
// wave's next tile is fetched while this one is multiplied); loads and arithmetic are the full scan's.
// fp64 (VQ_LAYOUT_TILED64, [tile][slice][k / 2][clip][2]): the same walk with the unit of doubles (TileVec).  Load i of a lane is at
// i * 128 + l * 2 doubles -- again 1 KB of contiguous memory per wave instruction -- and holds k = 8 i + 2 (l / 16) + 0..1: 128 loads per
// slice, each two fp64 FMAs against ONE 16-byte query read (fp32: four conversions, four FMAs, two reads per 16 bytes of features).
// The loop over the groups stays rolled and its query offset is the loop counter's: unrolled, the query reads (which do not depend on
// the tile) would be hoisted into registers across tiles -- scan_kernel's LEAN trap.  72-110 VGPRs, no scratch (profiles/README.md).
// fp16 (VQ_LAYOUT_TILED16, [tile][slice][k / 8][clip][8]): the unit of halves.  Load i of a lane is at i * 512 + l * 8 halves and holds
// k = 32 i + 8 (l / 16) + 0..7: 32 loads of 1 KB per wave and slice, each eight conversions and eight fp64 FMAs against four 16-byte query
// reads (the four k-groups read addresses 64 bytes apart, broadcast within a group).  Per element the query reads are fp32's while the
// HBM time halves.  Its group size is VQ_TILED_GROUP16.
template <typename T>
struct TileVec;                        // the 16 bytes a lane of scan_tiled_kernel loads: U elements, and their share of the dot
template <>
struct TileVec<float> {
    static constexpr int U = 4;
    float4 v;
    __device__ __forceinline__ void load(const float* p) { v = stream_load4(p); }
    __device__ __forceinline__ double dot(const double* tq, double p) const {
        const double2 ta = *reinterpret_cast<const double2*>(tq);
        const double2 tb = *reinterpret_cast<const double2*>(tq + 2);
        p = fma((double)v.x, ta.x, p);
        p = fma((double)v.y, ta.y, p);
        p = fma((double)v.z, tb.x, p);
        p = fma((double)v.w, tb.y, p);
        return p;
    }
};
template <>
struct TileVec<double> {
    static constexpr int U = 2;
    vq_d2 v;
    __device__ __forceinline__ void load(const double* p) { v = __builtin_nontemporal_load(reinterpret_cast<const vq_d2*>(p)); }
    __device__ __forceinline__ double dot(const double* tq, double p) const {
        const double2 ta = *reinterpret_cast<const double2*>(tq);
        p = fma(v.x, ta.x, p);
        p = fma(v.y, ta.y, p);
        return p;
    }
};
template <>
struct TileVec<__half> {
    static constexpr int U = 8;
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    h8 v;
    __device__ __forceinline__ void load(const __half* p) { v = __builtin_nontemporal_load(reinterpret_cast<const h8*>(p)); }
    __device__ __forceinline__ double dot(const double* tq, double p) const {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double2 tg = *reinterpret_cast<const double2*>(tq + 2 * g);
            p = fma(half_to_double(v[2 * g]), tg.x, p);
            p = fma(half_to_double(v[2 * g + 1]), tg.y, p);
        }
        return p;
    }
};

template <typename T, int S, int E, int CH, int G, bool VIEW = false>
__global__ __launch_bounds__(256) void scan_tiled_kernel(std::conditional_t<VIEW, ScanViewArgs, ScanArgs> a) {
    extern __shared__ __attribute__((aligned(16))) double t_lds[];    // [NV][D], natural order
    constexpr int NV = S * E;
    constexpr int D = CH * 256;
    constexpr int U = TileVec<T>::U, WL = 64 * U;                     // elements of a lane's load, of a wave's (1 KB)
    constexpr int LOADS = D * 16 / WL;                                // 1 KB loads of a wave per slice: D / 16 (fp32), D / 8 (fp64), D / 32 (fp16)
    constexpr int GROUPS = LOADS / G;
    static_assert(LOADS % G == 0, "group size must divide the slice");
    for (int i = threadIdx.x; i < NV * D; i += blockDim.x) t_lds[i] = a.t[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, col = lane & 15, kk = lane >> 4;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    int64_t ntiles = (a.n + 15) / 16;
    if constexpr (VIEW) ntiles = a.n_items;                          // work items: the touched tiles
    constexpr int64_t tile_elems = (int64_t)NV * 16 * D;
    const T* feats = static_cast<const T*>(a.feats) + lane * U;
    double w[S];
    if (a.w) {
#pragma unroll
        for (int s = 0; s < S; ++s) w[s] = a.w[s];
    }
    TileVec<T> cur[G], nxt[G];
    int64_t tile = wave;
    int64_t tr = 0, trn = 0, on = -1;                                  // VIEW: the tiles of item `tile` and of the wave's next item; this lane's position
    if constexpr (VIEW) {
        tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (tile < ntiles) {
            tr = a.items[tile];
            trn = a.items[min(tile + nwaves, ntiles - 1)];
            on = a.pos[tile * 16 + col];
        }
    }
    if (tile < ntiles) {
#pragma unroll
        for (int j = 0; j < G; ++j) cur[j].load(feats + (VIEW ? tr : tile) * tile_elems + j * WL);
    }
    while (tile < ntiles) {
        const int64_t tn = tile + nwaves;
        int64_t trnn = 0, onn = -1;
        if constexpr (VIEW) {
            trnn = a.items[min(tn + nwaves, ntiles - 1)];
            onn = a.pos[min(tn, ntiles - 1) * 16 + col];
        }
        const T* x = feats + (VIEW ? tr : tile) * tile_elems;
        // after the wave's last tile the ring is refilled from the tile just read: the refill stays unconditional
        const T* xn = tn < ntiles ? feats + (VIEW ? trn : tn) * tile_elems : x;
        const int64_t c = (VIEW ? tr : tile) * 16 + col;
        const int64_t o = VIEW ? on : c;                               // where this lane's clip reports
        const bool mine = kk == 0 && (VIEW ? o >= 0 : c < a.n);
        const int64_t cc = min(c, a.n - 1);                            // the clip whose presence bits this lane follows
        double acc = 0.0, av[S];
        int cnt = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const double* tq = t_lds + v * D + U * kk;
            double p = 0.0;
#pragma unroll 1
            for (int g = 0; g < GROUPS; ++g) {
                const T* src = (v + 1 < NV || g + 1 < GROUPS) ? x + ((int64_t)v * GROUPS + g + 1) * (G * WL) : xn;
#pragma unroll
                for (int j = 0; j < G; ++j) nxt[j].load(src + j * WL);
#pragma unroll
                for (int j = 0; j < G; ++j) p = cur[j].dot(tq + 4 * U * (g * G + j), p);
#pragma unroll
                for (int j = 0; j < G; ++j) cur[j] = nxt[j];
            }
            p += __shfl_xor(p, 16, 64);
            p += __shfl_xor(p, 32, 64);
            const int s = v / E, e = v % E;
            const int64_t idx = (cc * S + s) * E + e;
            const bool here = a.present ? a.present[idx] != 0 : true;
            if (here) {
                acc = acc + p;
                ++cnt;
            }
            if (a.sims && mine) a.sims[VIEW ? (o * S + s) * E + e : idx] = p;
            if (e == E - 1) {
                const double m = acc / (double)cnt;
                if (mine) {
                    a.avg[o * S + s] = m;
                    a.ne[o * S + s] = cnt;
                }
                av[s] = m;
                acc = 0.0;
                cnt = 0;
            }
        }
        if (a.w && mine) a.scores[o] = score_from_avg(av, w, S);
        tile = tn;
        if constexpr (VIEW) {
            tr = trn;
            trn = trnn;
            on = onn;
        }
    }
}

#ifndef VQ_TILED_GROUP
#define VQ_TILED_GROUP 4
#endif
constexpr int kTiledGroup = VQ_TILED_GROUP;     // 1 KB loads a wave of scan_tiled_kernel keeps in flight behind the ones it multiplies
#ifndef VQ_TILED_GROUP64
#define VQ_TILED_GROUP64 4
#endif
constexpr int kTiledGroup64 = VQ_TILED_GROUP64; // the same for fp64 (VQ_LAYOUT_TILED64)
#ifndef VQ_TILED_GROUP16
#define VQ_TILED_GROUP16 8
#endif
// the same for fp16 (VQ_LAYOUT_TILED16), 32 loads per slice.  8 from an A/B of 2 / 4 / 8 on one MI355X (profiles/README.md, "fp16 storage
// tiled in place"): 0.85 / 0.83 / 0.78 of the HBM peak at 1 M x 2 x 5 and 0.79 / 0.75 / 0.79 at 1 M x 2 x 3 -- at 8 the kernel holds 256
// VGPRs + 60-70 AGPRs (no scratch) and runs one wave per SIMD, 8 KB in flight each; 4 is the better value at 50 000 x 2 x 5 (0.73 / 0.64)
constexpr int kTiledGroup16 = VQ_TILED_GROUP16;
template <typename T>
constexpr int kTiledGroupOf = sizeof(T) == 8 ? kTiledGroup64 : sizeof(T) == 2 ? kTiledGroup16 : kTiledGroup;

// A = ScanArgs, or ScanViewArgs: the VIEW instantiations of the same kernels, under the same launch rules with the view's M for n
template <typename T, int S, int E, int CH, typename A>
static int launch_scan_t(vq_db* db, const A& a) {
    constexpr bool VIEW = std::is_same_v<A, ScanViewArgs>;
    const size_t lds = (size_t)S * E * CH * 256 * 8;
    int per_cu = (int)std::min<size_t>(8, (160 * 1024) / lds);
    if (per_cu < 1) per_cu = 1;
    // a database whose clips are a few per wave: the lean instantiation, three waves per SIMD (VQ_SCAN_LEAN=0|1 forces one or the other)
    static const int force_lean = getenv("VQ_SCAN_LEAN") ? atoi(getenv("VQ_SCAN_LEAN")) : -1;
    // (measured, MI355X, fp32 rows, lean against not: 10 000 clips x 2 x 3: 49 against 59 us; 50 000: 0.77 against 0.72 of the HBM peak; 1 M x 2 x 3:
    // 0.81 against 0.76; 1 M x 2 x 5: 0.81 against 0.82; fp64 rows 200 000 x 2 x 3: 0.75 against 0.76)
    // fp16 rows: always lean.  The streaming instantiation holds the same 256-380 VGPRs of query (one wave per SIMD) but has half the bytes per
    // vector in flight and three instructions per element to hide: 1 M x 2 x 5: 3.54 against 5.67 ms (0.72 against 0.45 of the HBM peak);
    // 1 M x 2 x 3: 1.95 against 2.57 ms; 50 000 x 2 x 5: 0.18 against 0.30 ms; 10 000 x 2 x 3: 31 against 43 us
    const bool lean = force_lean >= 0 ? force_lean != 0
                                      : (sizeof(T) == 2 || a.n < (int64_t)db->cus * per_cu * 4 * 16 || (sizeof(T) == 4 && S * E <= 6));
    // the dynamic LDS limit is raised per kernel: once per instantiation chosen
    void (*kern)(A) = nullptr;
    int64_t want = (a.n + 3) / 4;   // 4 waves (clips in flight) per block
    if (db->tiled()) {
        kern = scan_tiled_kernel<T, S, E, CH, kTiledGroupOf<T>, VIEW>;
        VQ_DYN_LDS(kern, lds);
        want = ((a.n + 15) / 16 + 3) / 4;   // 4 waves (tiles in flight) per block
        if constexpr (VIEW) want = (a.n_items + 3) / 4;
    } else if (lean) {
        kern = scan_kernel<T, S, E, CH, true, VIEW>;
        VQ_DYN_LDS(kern, lds);
    } else {
        kern = scan_kernel<T, S, E, CH, false, VIEW>;
        VQ_DYN_LDS(kern, lds);
    }
    // (as many waves as fit the chip.  Fewer waves that each walk the same number of clips -- 2 500 waves of exactly four clips for a
    // 10 000-clip database instead of 3 072 of three or four -- were measured in round 6: 62.9 against 56.8 us per scan; the streams in
    // flight matter more than the ragged last round.)
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)db->cus * per_cu));
    kern<<<grid, 256, lds, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

template <typename T, typename A>
static int launch_scan_shape(vq_db* db, const A& a) {
    if (db->D == 1024) {
        // every entry is launched by tests/test_scan_matrix_gpu.py (SHAPES in tests/_scan_matrix_cases.py): a new entry gets a new row there
#define C_(s_, e_) \
    if (db->S == s_ && db->E == e_) return launch_scan_t<T, s_, e_, 4, A>(db, a);
        C_(1, 1) C_(1, 2) C_(1, 3) C_(1, 4) C_(1, 5)
        C_(2, 1) C_(2, 2) C_(2, 3) C_(2, 4) C_(2, 5)
#undef C_
    }
    if (db->layout != VQ_LAYOUT_ROWS) return fail(VQ_E_STATE, "internal: tiled layout on a shape without a tiled scan kernel");
    // a handle created with VQ_DIM_SHORT_ROWS (include/vq_amd_dim.h), stored D <= 128: the short-row kernel, unless the environment
    // (VQ_SCAN_SHORT=0) forces the generic one; every other handle runs what it ever ran
    static const int env_short = getenv("VQ_SCAN_SHORT") ? atoi(getenv("VQ_SCAN_SHORT")) : -1;
    if (db->short_rows && db->D <= 128 && env_short != 0) {
        int lg = 0;
        while ((4 << lg) < db->D) ++lg;                                // L = 1 << lg lanes per clip, 64 >> lg clips per wave
        const size_t lds = (size_t)db->S * db->E * db->D * 8;           // <= 64 x 128 x 8 = 64 KB
        void (*kern)(A, int) = scan_short_kernel<T, std::is_same_v<A, ScanViewArgs>>;
        VQ_DYN_LDS(kern, 65536);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
        const int64_t per_block = 4 * (int64_t)(64 >> lg);             // 4 waves of 64 / L clips
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.n + per_block - 1) / per_block, (int64_t)db->cus * per_cu));
        kern<<<grid, 256, lds, db->stream>>>(a, lg);
        VQ_CHECK_LAUNCH();
        return VQ_OK;
    }
    const int64_t want = (a.n + 3) / 4;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)db->cus * 8));
    scan_generic_kernel<T, std::is_same_v<A, ScanViewArgs>><<<grid, 256, 0, db->stream>>>(a);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

// the storage type's kernels (vq_db_scan and vq_db_query_round: the same kernels, the same bits)
template <typename A>
static int launch_scan_args(vq_db* db, const A& a) {
    return with_dtype(db, [&](auto x) { return launch_scan_shape<decltype(x), A>(db, a); });
}

// ... over the row view in use: none -> the kernels, the arguments and the launch of ever; M = 0 -> nothing to launch
int vq::launch_scan(vq_db* db, bool with_scores, bool keep_sims) {
    ScanArgs a;
    a.feats = db->feats;
    a.t = db->t;
    a.present = db->present;
    a.w = with_scores ? db->w : nullptr;
    a.sims = keep_sims ? db->sims.get() : nullptr;
    a.avg = db->avg;
    a.ne = db->ne;
    a.scores = db->scores;
    a.n = db->n;
    a.S = db->S;
    a.E = db->E;
    a.D = db->D;
    if (db->active < 0) return launch_scan_args<ScanArgs>(db, a);
    const vq_db::RowView& v = db->views[db->active];
    if (v.m == 0) return VQ_OK;
    ScanViewArgs va;
    static_cast<ScanArgs&>(va) = a;
    va.pos = nullptr;
    if (db->tiled()) {
        if (!v.tiles) return fail(VQ_E_STATE, "internal: a row view without tile tables on a tiled database");
        va.items = v.tiles;
        va.pos = v.pos;
        va.n_items = v.ntiles;            // va.n stays N: the ragged last tile's bound
    } else {
        va.items = v.rows;
        va.n_items = va.n = v.m;
    }
    return launch_scan_args<ScanViewArgs>(db, va);
}

extern "C" {

int vq_db_scan(vq_db* db, const double* w_host, int32_t keep_sims) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_query) return fail(VQ_E_STATE, "vq_db_scan: no query set (call vq_db_set_query first)");
    DeviceGuard g(db->device);
    if (keep_sims) VQ_HIP(db->sims.grow((size_t)db->n * db->S * db->E * 8));
    if (w_host) VQ_HIP(hipMemcpyAsync(db->w, w_host, db->S * 8, hipMemcpyHostToDevice, db->stream));
    const int rc = launch_scan(db, w_host != nullptr, keep_sims != 0);          // over the row view in use, if any
    if (rc != VQ_OK) return rc;
    db->have_avg = true;
    db->have_sims = keep_sims != 0;
    db->have_scores = w_host != nullptr;
    return VQ_OK;
}

}  // extern "C"
