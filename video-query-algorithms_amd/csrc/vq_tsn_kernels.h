// What the TSN executor (vq_tsn.hip) and its separately compiled kernel files (vq_tsn_conv.hip, vq_tsn_ops.hip, vq_wino.hip) share:
// device helpers, the pooling path, the Winograd launch, and the host launches of the small kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "host/vq_tsn_plan.h"   // KPAD, FC_COLS, kMaxFusedT, kWinoMaxJobs, kWinoMaxPools
#include "vq_div9.h"

namespace vq {

// XCD-aware tile order: workgroups b and b+8 share an XCD (and its L2); give each XCD a contiguous run of
// tiles, with the N tiles of one M tile adjacent, so the gathered activation tile is re-read from L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// x / d as one multiply-high: m = floor(2^32 / d) + 1 is exact while x * (m d - 2^32) < 2^32, i.e. certainly for
// x < 2^32 / d (the host checks that bound where it builds the constants: magic_u32 in vq_wino.hip).  d = 1 has no such
// constant; it is encoded as m = 0.  On uniform values the compiler keeps all of it on the scalar unit (s_mul_hi_u32),
// which costs the matrix pipe nothing.
__device__ __forceinline__ unsigned magic_div(unsigned x, unsigned m) { return m ? __umulhi(x, m) : x; }

// x / d for EVERY 32-bit x (Granlund & Montgomery): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1,
// t = mulhi(m, x), q = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0).  Five scalar instructions on a uniform x.
struct FullDiv {
    unsigned m, sh1, sh2;
};
__device__ __forceinline__ unsigned full_div(unsigned x, const FullDiv& d) {
    const unsigned t = __umulhi(d.m, x);
    return (t + ((x - t) >> d.sh1)) >> d.sh2;
}
static inline FullDiv full_div_for(unsigned d) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    FullDiv f;
    f.m = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 1 ? l - 1 : 0;
    return f;
}
// x / d = (x * s) >> 22 with s = 2^22 / d + 1 on 24-bit multiplies (v_mul_u32_u24: full rate; v_mul_lo / v_mul_hi_u32 run at a quarter
// of it): exact while x (s d - 2^22) < 2^22, i.e. certainly for x d < 2^22, and x s < 2^32 (recip22_ok).
constexpr int kRecipShift = 22;
// 24-bit multiplies as inline asm: through __umul24 / __mul24 the compiler reasons about the operand masks, finds them dead where only the
// low bits of a product are used further on, and is back at a plain 32-bit multiply (v_mul_lo_u32, v_mad_u64_u32).
// The second factor is UNIFORM (a kernel argument or scalar arithmetic on some): it stays in a scalar register.
__device__ __forceinline__ unsigned umul24(unsigned x, unsigned y_uniform) {
    unsigned r;
    asm("v_mul_u32_u24 %0, %2, %1" : "=v"(r) : "v"(x), "s"(y_uniform));
    return r;
}
__device__ __forceinline__ int imul24(int x, int y_uniform) {
    int r;
    asm("v_mul_i32_i24 %0, %2, %1" : "=v"(r) : "v"(x), "s"(y_uniform));
    return r;
}
static inline unsigned recip22(unsigned d) { return (1u << kRecipShift) / d + 1u; }
static inline bool recip22_ok(unsigned d, unsigned xmax) {
    return d >= 1 && (unsigned long long)xmax * d < (1ull << kRecipShift) && (unsigned long long)xmax * recip22(d) < (1ull << 32);
}

// ------------------------------------------------------------------------------------------------
// pooling (Caffe semantics: ceil-mode output size; MAX ignores padding; AVE divides by the window
// clipped to the padded extent and accumulates h-major in fp32)
// ------------------------------------------------------------------------------------------------
struct PoolArgs {
    const float* in;
    float* out;
    int H, W, Cs_in, coff_in, C;
    int Ho, Wo, Cs_out, coff_out;
    int k, stride, pad;
    int is_max;
    int64_t total;   // n * Ho * Wo * C/4
    const float* bias;   // AVE only: added after the division (finishes a commuted 1x1 projection), may be null
    int relu;
    int unit0, n_units;  // grouped launch: workgroups [unit0, unit0 + n_units), kPoolPerWG outputs each
    // The window-specialised path (pool_unit below); pool_plan() fills all of it from the fields above and the two extents.
    int mode;            // 0: generic pool_one per output; kPool311: (k, stride, pad) = (3, 1, 1); kPool320: (3, 2, 0)
    unsigned in_bytes, out_bytes;   // extents of the two slots for the buffer descriptors (the caller sets them before pool_plan)
    FullDiv d_c4n, d_wo, d_ho;      // a workgroup's first output -> (image, row, column, channel quad): scalar unit, any 32-bit index
    unsigned s_c4n, s_wo, s_ho;     // recip22 constants for the per-lane walk (at most kPoolPerWG outputs further)
};
constexpr int kPoolPerWG = 1024;   // float4 outputs per pooling workgroup (grouped launch, and pool_fast_kernel)
constexpr int kPool311 = 1, kPool320 = 2;

// Chooses PoolArgs::mode and builds the division constants.  The specialised path needs one of the two window shapes with the output
// size Caffe's ceil rule gives them, slots within signed 32-bit byte offsets, and every factor of its 24-bit multiplies below 2^23;
// anything else keeps mode 0, which has no such limits.
static inline void pool_plan(PoolArgs& a, int n_crops) {
    a.mode = 0;
    const bool w311 = a.k == 3 && a.stride == 1 && a.pad == 1 && a.Ho == a.H && a.Wo == a.W;
    // (3, 2, 0): the last window starts inside the map (so a clamped row or column is one of the window's own)
    const bool w320 = a.k == 3 && a.stride == 2 && a.pad == 0 && a.Ho >= 1 && a.Wo >= 1 && 2 * (a.Ho - 1) < a.H && 2 * (a.Wo - 1) < a.W;
    if (!w311 && !w320) return;
    const unsigned c4n = (unsigned)(a.C >> 2);
    if (a.C < 4 || a.C % 4 || a.Cs_in % 4 || a.coff_in % 4 || a.Cs_out % 4 || a.coff_out % 4) return;
    if (a.in_bytes > 0x7FFFFFF0u || a.out_bytes > 0x7FFFFFF0u || a.in_bytes == 0 || a.out_bytes == 0) return;
    if (a.total <= 0 || a.total + kPoolPerWG >= (1ll << 31)) return;
    if ((long long)n_crops * a.H * a.W + a.W + 2 >= (1 << 23) || (long long)n_crops * a.Ho * a.Wo + kPoolPerWG >= (1 << 23) ||
        a.Cs_in >= (1 << 21) || a.Cs_out >= (1 << 21))
        return;
    if (!recip22_ok(c4n, c4n + kPoolPerWG) || !recip22_ok((unsigned)a.Wo, (unsigned)a.Wo + kPoolPerWG) ||
        !recip22_ok((unsigned)a.Ho, (unsigned)a.Ho + kPoolPerWG))
        return;
    a.d_c4n = full_div_for(c4n);
    a.d_wo = full_div_for((unsigned)a.Wo);
    a.d_ho = full_div_for((unsigned)a.Ho);
    a.s_c4n = recip22(c4n);
    a.s_wo = recip22((unsigned)a.Wo);
    a.s_ho = recip22((unsigned)a.Ho);
    a.mode = w311 ? kPool311 : kPool320;
}

typedef float poolx4 __attribute__((ext_vector_type(4)));
typedef float poolx2 __attribute__((ext_vector_type(2)));
typedef unsigned pooluintx4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

// One-instruction arithmetic on loaded values (results go to memory only).  v_max3_f32 and v_max_f32 as inline asm: the compiler
// puts a canonicalising v_max(x, x) in front of every fmaxf() on a value it cannot prove quiet.
__device__ __forceinline__ float max3(float x, float y, float z) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
    return r;
}
__device__ __forceinline__ float max0(float x) {
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ poolx4 pool_add(poolx4 x, poolx4 y) {     // two v_pk_add_f32: the same fp32 add per element
    poolx2 lo, hi;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(x.xy), "v"(y.xy));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(x.zw), "v"(y.zw));
    return (poolx4){lo.x, lo.y, hi.x, hi.y};
}

// The nine taps of one output in flight, and where the result goes.
struct PoolTaps {
    poolx4 v[9];         // h-major
    poolx4 b;            // AVE with a bias
    unsigned ooff;       // byte offset of the output quad; 0xFFFFFFFF: past the end, the store is dropped
    float size;          // AVE, (3, 2, 0): Caffe's divisor (the window clipped to the padded extent)
};

// kPoolPerWG consecutive outputs (index = ((image * Ho + row) * Wo + column) * C/4 + channel quad), kPoolPerWG / 256 per thread, for the
// window shapes (3, 1, 1) and (3, 2, 0).  The workgroup's first output is decoded on the scalar unit; a lane walks from there with
// recip22 multiplies; every address is a 32-bit byte offset into a buffer descriptor (out-of-range offsets read as zero / are dropped).
// All nine taps of an output are requested before the first is used, and the taps of the thread's next output are requested before
// the arithmetic of the current one.
//   MAX: rows and columns past the edge are clamped to the map -- a clamped tap re-reads a pixel of the same window, which cannot
//        change a maximum (no reliance on zero fill: right for negative inputs).
//   AVE: taps past the edge get an out-of-range offset and read as +0; the chain 0 + t00 + t01 + ... (h-major, one fp32 add per tap)
//        can never hold -0, so adding +0 where pool_one skips the tap gives the same bits.  (3, 1, 1) divides by 9 everywhere
//        (div9); (3, 2, 0) by Caffe's clipped window size with '/'.
template <int MODE, bool IS_MAX>
__device__ __forceinline__ void pool_unit(const PoolArgs& a, unsigned unit) {
    constexpr int S = MODE == kPool311 ? 1 : 2, P = MODE == kPool311 ? 1 : 0, R = kPoolPerWG / 256;
    constexpr unsigned kRowOut = 0x80000000u, kColOut = 0x7FFFFFF0u;   // row + column: past in_bytes whenever either is out, and never wraps
    // ---- the workgroup's first output: scalar unit -------------------------------------------------------------------------------
    const unsigned c4n = (unsigned)a.C >> 2, H = (unsigned)a.H, W = (unsigned)a.W, Ho = (unsigned)a.Ho, Wo = (unsigned)a.Wo;
    const unsigned first = unit * (unsigned)kPoolPerWG;
    const unsigned pix0 = full_div(first, a.d_c4n), c40 = first - pix0 * c4n;
    const unsigned row0 = full_div(pix0, a.d_wo), pw0 = pix0 - row0 * Wo;
    const unsigned n0 = full_div(row0, a.d_ho), ph0 = row0 - n0 * Ho;
    const unsigned s_c4n = a.s_c4n, s_wo = a.s_wo, s_ho = a.s_ho;
    const unsigned left = (unsigned)a.total - first;                   // outputs from `first` to the end of the layer
    const int px = a.Cs_in * 4, opx = a.Cs_out * 4, cin0 = a.coff_in * 4, cout0 = a.coff_out * 4;
    const bool has_bias = !IS_MAX && a.bias != nullptr, relu = !IS_MAX && a.relu != 0;
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, a.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, a.out_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, has_bias ? (unsigned)a.C * 4u : 0u, 0x00020000);

    PoolTaps t[2];
    auto request = [&](int r, PoolTaps& q) {
        const unsigned e = (unsigned)(r * 256) + threadIdx.x;
        const unsigned x = c40 + e, dp = umul24(x, s_c4n) >> kRecipShift, c4 = x - umul24(dp, c4n);
        const unsigned y = pw0 + dp, dq = umul24(y, s_wo) >> kRecipShift, pw = y - umul24(dq, Wo);
        const unsigned z = ph0 + dq, dn = umul24(z, s_ho) >> kRecipShift, ph = z - umul24(dn, Ho);
        const int nH = imul24((int)(n0 + dn), (int)H);
        const int hs = (int)ph * S - P, ws = (int)pw * S - P;
        const int cb = cin0 + (int)c4 * 16;
        unsigned ro[3], co[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {            // (the multiplies are inline asm: computed first, selected after -- no branch around them)
            const int h = IS_MAX ? min(max(hs + d, 0), (int)H - 1) : hs + d, w = IS_MAX ? min(max(ws + d, 0), (int)W - 1) : ws + d;
            const unsigned rb = (unsigned)(imul24(imul24(nH + h, (int)W), px) + cb), cbyte = (unsigned)imul24(w, px);
            ro[d] = IS_MAX || (unsigned)h < H ? rb : kRowOut;
            co[d] = IS_MAX || (unsigned)w < W ? cbyte : kColOut;
        }
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
#pragma unroll
            for (int dw = 0; dw < 3; ++dw)
                q.v[dh * 3 + dw] = __builtin_bit_cast(poolx4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, ro[dh] + co[dw], 0, 0));
        if (has_bias) q.b = __builtin_bit_cast(poolx4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, c4 * 16u, 0, 0));
        const unsigned obyte = umul24(pix0 + dp, (unsigned)opx) + (unsigned)cout0 + c4 * 16u;
        q.ooff = e < left ? obyte : 0xFFFFFFFFu;
        if (!IS_MAX && MODE != kPool311)
            q.size = (float)(min(hs + 3, (int)H + P) - hs) * (float)(min(ws + 3, (int)W + P) - ws);   // small integers: the product is exact
    };
    auto finish = [&](const PoolTaps& q) {
        poolx4 acc;
        if (IS_MAX) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[c] = max3(max3(q.v[0][c], q.v[1][c], q.v[2][c]), max3(q.v[3][c], q.v[4][c], q.v[5][c]), max3(q.v[6][c], q.v[7][c], q.v[8][c]));
        } else {
            acc = pool_add((poolx4){0.f, 0.f, 0.f, 0.f}, q.v[0]);
#pragma unroll
            for (int k = 1; k < 9; ++k) acc = pool_add(acc, q.v[k]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = MODE == kPool311 ? div9(acc[c]) : acc[c] / q.size;
            if (has_bias) acc = pool_add(acc, q.b);
            if (relu) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = max0(acc[c]);
            }
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pooluintx4, acc), out_rsrc, q.ooff, 0, 0);
    };
    request(0, t[0]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r + 1 < R) request(r + 1, t[(r + 1) & 1]);
        finish(t[r & 1]);
    }
}

// The workgroup `unit` of a layer on the specialised path (a.mode != 0).
__device__ __forceinline__ void pool_unit_any(const PoolArgs& a, unsigned unit) {
    if (a.mode == kPool311) {
        if (a.is_max)
            pool_unit<kPool311, true>(a, unit);
        else
            pool_unit<kPool311, false>(a, unit);
    } else {
        if (a.is_max)
            pool_unit<kPool320, true>(a, unit);
        else
            pool_unit<kPool320, false>(a, unit);
    }
}

// Output i (4 consecutive channels of one pooled pixel): any window, any size.
template <bool IS_MAX>
__device__ __forceinline__ void pool_one(const PoolArgs& a, int64_t i) {
    const int c4n = a.C >> 2;
    const int c4 = (int)(i % c4n);
    int64_t pix = i / c4n;
    const int pw = (int)(pix % a.Wo);
    pix /= a.Wo;
    const int ph = (int)(pix % a.Ho);
    const int64_t n = pix / a.Ho;
    int hs = ph * a.stride - a.pad, ws = pw * a.stride - a.pad;
    int he = min(hs + a.k, a.H + a.pad), we = min(ws + a.k, a.W + a.pad);
    const float pool_size = (float)((he - hs) * (we - ws));
    hs = max(hs, 0);
    ws = max(ws, 0);
    he = min(he, a.H);
    we = min(we, a.W);
    const float* base = a.in + (size_t)n * a.H * a.W * a.Cs_in + a.coff_in + c4 * 4;
    float4 acc = IS_MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) {
            const float4 v = *reinterpret_cast<const float4*>(base + ((size_t)h * a.W + w) * a.Cs_in);
            if (IS_MAX) {
                acc.x = fmaxf(acc.x, v.x);
                acc.y = fmaxf(acc.y, v.y);
                acc.z = fmaxf(acc.z, v.z);
                acc.w = fmaxf(acc.w, v.w);
            } else {
                acc.x += v.x;
                acc.y += v.y;
                acc.z += v.z;
                acc.w += v.w;
            }
        }
    if (!IS_MAX) {
        acc.x /= pool_size;
        acc.y /= pool_size;
        acc.z /= pool_size;
        acc.w /= pool_size;
        if (a.bias) {
            const float4 b = *reinterpret_cast<const float4*>(a.bias + c4 * 4);
            acc.x += b.x;
            acc.y += b.y;
            acc.z += b.z;
            acc.w += b.w;
        }
        if (a.relu) {
            acc.x = fmaxf(acc.x, 0.f);
            acc.y = fmaxf(acc.y, 0.f);
            acc.z = fmaxf(acc.z, 0.f);
            acc.w = fmaxf(acc.w, 0.f);
        }
    }
    float* o = a.out + (((size_t)n * a.Ho + ph) * a.Wo + pw) * a.Cs_out + a.coff_out + c4 * 4;
    *reinterpret_cast<float4*>(o) = acc;
}

// One 3x3 / stride 1 / pad 1 convolution (+ folded BN + ReLU) in Winograd F(2x2, 3x3) form: see vq_wino.hip.
struct WinoJob {
    const float* in;     // NHWC slot (first crop of this launch)
    const float* u;      // transformed filters [Cin/8][16][Cout][8]: U = G g G^T, position xi = 4 i + j
    const float* bias;   // [Cout]
    float* out;          // NHWC slot, same H x W (first crop of this launch)
    int H, W, Cs_in, coff_in, Cin;
    int Cs_out, coff_out, Cout;
    int th, tw, P;       // 2x2 output tiles per image (rows, columns) and in the whole launch
    int relu;
    int t16;             // 1: u is the second layout of a VQ_OP_CONV_WINOGRAD16 layer -- [Cin/16][16][Cout][16 slots] -- and the units have 16 tiles
    int tiles_n;         // 32*NB-channel blocks of Cout
    int unit0, n_units;  // workgroups [unit0, unit0 + n_units) of the launch belong to this job (unit0 % 8 == 0)
    unsigned in_bytes, u_bytes, out_bytes;   // extents for the buffer descriptors (out-of-range offsets read as zero / are dropped)
    unsigned m_tiles_n, m_tpi, m_tw;         // magic_div constants for tiles_n, th * tw and tw
    unsigned s_tw, s_th;                     // recip22 constants for the per-lane tile walk (at most 31 tiles from the workgroup's first)
#ifdef VQ_WINO_PHASES
    long long* phases;   // tools/ubench/wino_phases.hip: [workgroup][6] s_memtime stamps
#endif
};

// kWinoMaxJobs convolutions and kWinoMaxPools pooling layers of one graph level as ONE launch (host/vq_tsn_plan.h)
struct WinoGroup {
    int n_jobs;
    int n_pools;         // pooling layers of the same graph level: their (few, short) workgroups come last and fill the tail
    int total_units;     // grid size (jobs padded to multiples of 8 workgroups so every job keeps its XCD mapping)
    int pool_unit0;      // first pooling workgroup
    WinoJob job[kWinoMaxJobs];
    PoolArgs pool[kWinoMaxPools];
};

constexpr int kWinoVariants = 2;   // output-channel blocks of 32 per workgroup: variant v -> (v & 1) + 1; v >= 2: units of 16 tiles (layers that carry both layouts)

// Fill the derived fields of the jobs (unit ranges, magic constants) for `variant` and launch on `stream`.
// ev_start / ev_stop (both or neither): events that receive the kernel's own begin / end timestamps
// (hipExtLaunchKernelGGL) for per-launch profiling.  Returns a VQ_* status.
int launch_wino_group(WinoGroup& g, int variant, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);

// vq_tsn_ops.hip: one host launch per small kernel; each returns a VQ_* status.  ev_start / ev_stop: as for launch_wino_group.
// n uint8 NHWC crops at src -> the fp32 input slot at dst (channels padded, or space-to-depth: vq_input_desc), minus mean
int launch_preprocess(const uint8_t* src, float* dst, int n, const vq_input_desc& in, const vq_tensor_desc& t0, const float* mean,
                      hipStream_t stream);
// one pooling layer (after pool_plan): the window-specialised path where a.mode says so, else one thread per output
int launch_pool(const PoolArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
int launch_gavgpool(const float* in, float* out, int n, int HW, int Cs_in, int coff_in, int C, int Cs_out, int coff_out, hipStream_t stream,
                    hipEvent_t ev_start, hipEvent_t ev_stop);
// global pool + segment consensus of B whole clips of T <= kMaxFusedT snippets
int launch_gavgpool_consensus(const float* in, float* out, double* feat, int B, int T, int HW, int Cs_in, int coff_in, int C, int Cs_out,
                              int coff_out, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
int launch_inner_product(const float* x, int x_stride, const float* W, const float* bias, float* y, int y_stride, int M, int K, int N,
                         hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
// the slices of a K-split convolution added in slice order, + bias, ReLU (M * Cout and M * Cs_out below 2^31: the caller checks)
int launch_splitk_combine(const float* part, int ksplit, size_t slice_stride, int M, int Cout, const float* bias, int relu, float* out,
                          int Cs_out, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
int launch_consensus(const float* per_snippet, double* feat, int B, int T, int D, int Cs, hipStream_t stream);

// A launch whose begin / end timestamps land in two events when they are given: the timestamps come from the
// dispatch packet itself, so the measured interval is the kernel alone (what rocprofv3 reports) and no extra
// marker packets sit between consecutive layers.
#define VQ_LAUNCH(KERN, GRID, BLOCK, LDS, STREAM, EV_START, EV_STOP, ...)                                     \
    do {                                                                                                      \
        if ((EV_START) || (EV_STOP))                                                                          \
            hipExtLaunchKernelGGL(KERN, dim3(GRID), dim3(BLOCK), (std::uint32_t)(LDS), STREAM, EV_START, EV_STOP, 0, __VA_ARGS__); \
        else                                                                                                  \
            KERN<<<GRID, BLOCK, LDS, STREAM>>>(__VA_ARGS__);                                                  \
    } while (0)

}  // namespace vq
