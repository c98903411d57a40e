// The direct convolution of the TSN forward pass on gfx950: convolution + frozen BN + ReLU as implicit GEMM, M = crops*Ho*Wo pixels,
// N = Cout, K = k*k*Cin, on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, 256 FLOP/clk/CU) from LDS-staged,
// register-prefetched tiles -- the 1x1, stride-2 and stem layers (the 3x3 / stride-1 layers: vq_wino.hip).  The kernels, one host
// launch per instantiation, the table of tilings, and the rule for which kernel serves a tiling; the executor (vq_tsn.hip) fills
// the arguments and picks the tiling (vq_tsn_conv.h).
#include <algorithm>

#include "vq_common.h"
#include "vq_tsn_conv.h"

using namespace vq;

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

// ------------------------------------------------------------------------------------------------
// convolution (+ folded BN + ReLU) as implicit GEMM on v_mfma_f32_32x32x2_f32
// ------------------------------------------------------------------------------------------------
// ConvSeg / ConvArgs: vq_tsn_conv.h
template <int BM, int BN, int BK>
struct ConvSmem {
    // padded rows (BK + 4 floats): the 16 rows one ds_read_b128 lane group touches land on 16 distinct
    // 16-byte bank slots for BK = 16 and BK = 32 alike
    float a[2][BM][BK + 4];
    float b[2][BN][BK + 4];
};

// Epilogue shared by both kernels: + bias (folded BN), ReLU, store at the channel offset of the destination slot.
// In the MFMA C/D layout a lane holds ONE channel of 16 pixels (column = lane & 31, row = (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5)), which would mean 16 four-byte stores per accumulator tile; the store tail of such a wave is
// issue-bound and cost ~20 % of a K = 576 tile.  Each wave therefore transposes its 32x32 tile through a private
// 4.5 KB LDS patch and writes 16 bytes per lane: 4 store instructions per tile, each 8 pixels x 128 bytes.
#define VQ_EPILOGUE()                                                                                             \
    {                                                                                                             \
        __syncthreads(); /* every wave is done with the K-loop image of the LDS */                               \
        float* patch = reinterpret_cast<float*>(smem_raw) + wave * (32 * 36);                                     \
        const int prow = lane >> 3, pc4 = lane & 7;                                                               \
        const bool full_m = m0 + BM <= a.M;                                                                       \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                          \
            const int nb = n0 + wn * (BN / WN) + 32 * j;                                                          \
            if (nb < a.Cout) {                                                                                    \
                const ConvSeg sg = seg_v[j];                                                                      \
                _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                  \
                    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                \
                        patch[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + l31] = acc[i][j][r];                     \
                    const int mb = m0 + wm * (BM / WM) + 32 * i;                                                  \
                    _Pragma("unroll") for (int ps = 0; ps < 4; ++ps) {                                            \
                        const int row = prow + 8 * ps;                                                            \
                        floatx4 v = *reinterpret_cast<const floatx4*>(&patch[row * 36 + pc4 * 4]);                \
                        v += bias_v[j];                                                                           \
                        if (sg.relu) {                                                                            \
                            v[0] = fmaxf(v[0], 0.f);                                                              \
                            v[1] = fmaxf(v[1], 0.f);                                                              \
                            v[2] = fmaxf(v[2], 0.f);                                                              \
                            v[3] = fmaxf(v[3], 0.f);                                                              \
                        }                                                                                         \
                        if ((full_m || mb + row < a.M) && nb + pc4 * 4 < a.Cout)                                  \
                            *reinterpret_cast<floatx4*>(sg.out_base + (size_t)(a.out_row0 + mb + row) * sg.Cs + nb + pc4 * 4) = v; \
                    }                                                                                             \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    }

// The same epilogue with 32-bit offsets into a buffer descriptor per destination segment (conv_igemm_pipe_kernel, whose wave index is a
// scalar): the row / segment part of an address is uniform and rides in the store's scalar offset, the lane part (row in the 8-row group,
// 16-byte column) is formed once per segment, a masked-off lane stores at 0xFFFFFFFF (dropped by the range check).  No 64-bit vector
// arithmetic, no multiply per store.  A launch never spans 2^31 bytes of a destination slot (LaunchItem::max_crops).
#define VQ_EPILOGUE_BUF()                                                                                         \
    {                                                                                                             \
        __syncthreads(); /* every wave is done with the K-loop image of the LDS */                               \
        float* patch = reinterpret_cast<float*>(smem_raw) + wave * (32 * 36);                                     \
        const int prow = lane >> 3, pc4 = lane & 7;                                                               \
        const bool full_m = m0 + BM <= a.M;                                                                       \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                          \
            const int nb = n0 + wn * (BN / WN) + 32 * j;                                                          \
            if (nb < a.Cout) {                                                                                    \
                const ConvSeg sg = seg_v[j];                                                                      \
                const __amdgpu_buffer_rsrc_t o_rsrc =                                                             \
                    __builtin_amdgcn_make_buffer_rsrc(sg.out_base + (size_t)a.out_row0 * sg.Cs, 0, 0x7FFFFFF0u, 0x00020000); \
                const unsigned lane_off = nb + pc4 * 4 < a.Cout ? (unsigned)((imul24(prow, sg.Cs) + pc4 * 4) * 4) : 0xFFFFFFFFu; \
                _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                  \
                    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                \
                        patch[((r & 3) + 8 * (r >> 2) + 4 * half) * 36 + l31] = acc[i][j][r];                     \
                    const int mb = m0 + wm * (BM / WM) + 32 * i;                                                  \
                    _Pragma("unroll") for (int ps = 0; ps < 4; ++ps) {                                            \
                        const int row = prow + 8 * ps;                                                            \
                        floatx4 v = *reinterpret_cast<const floatx4*>(&patch[row * 36 + pc4 * 4]);                \
                        v += bias_v[j];                                                                           \
                        if (sg.relu) {                                                                            \
                            v[0] = fmaxf(v[0], 0.f);                                                              \
                            v[1] = fmaxf(v[1], 0.f);                                                              \
                            v[2] = fmaxf(v[2], 0.f);                                                              \
                            v[3] = fmaxf(v[3], 0.f);                                                              \
                        }                                                                                         \
                        const unsigned off = (full_m || mb + row < a.M) ? lane_off : 0xFFFFFFFFu;                 \
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, v), o_rsrc, off,        \
                                                               ((mb + 8 * ps) * sg.Cs + nb) * 4, 0);              \
                    }                                                                                             \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    }

// One workgroup = 4 waves = one BM x BN output tile; K is walked in steps of BK through a double-buffered LDS
// image that is filled through registers (global -> VGPR under the MFMAs of the current step -> LDS).
template <int BM, int BN, int WM, int WN, int BK, bool SMALL_CIN, bool POOL = false>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(BK == 16 || BK == 32, "BK is 16 or 32");
    static_assert(!(POOL && SMALL_CIN), "the pooled loader walks whole channel chunks");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;   // 32x32 accumulator tiles per wave
    constexpr int CPR = BK / 4;                            // 16-byte chunks per staged row
    constexpr int NA = (BM * CPR + 255) / 256, NB = (BN * CPR + 255) / 256;   // chunks staged per thread
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    ConvSmem<BM, BN, BK>& sm = *reinterpret_cast<ConvSmem<BM, BN, BK>*>(smem_raw);

    const int tid = threadIdx.x;
    const int n_tiles = a.tiles_m * a.tiles_n;
    const int ks = a.ksplit > 1 ? (int)blockIdx.x / n_tiles : 0;            // K slice of this workgroup (uniform)
    const int kbeg = ks * a.k_per;
    const int tile = xcd_remap(blockIdx.x - ks * n_tiles, n_tiles);
    const int m0 = (tile / a.tiles_n) * BM;
    const int n0 = (tile % a.tiles_n) * BN;

    // ---- staging roles: chunk id = tid + 256 i -> (row, 16-byte column).
    // Rows past M get an input row far outside the image, so the ordinary bounds test routes them to the
    // zero page; every pointer below stays derived from a kernel argument (global address space -- a null
    // alternative would demote the loads to flat_load, which also counts against lgkmcnt).
    const float* a_img[NA];
    int a_ih0[NA], a_iw0[NA], a_row[NA], a_col[NA];
    const int HoWo = a.Ho * a.Wo;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int c = tid + 256 * i;
        a_row[i] = c / CPR;
        a_col[i] = c % CPR;
        const int m = m0 + a_row[i];
        const bool ok = m < a.M && a_row[i] < BM;
        const int mm = ok ? m : 0;
        const int n_img = mm / HoWo, rem = mm - n_img * HoWo;
        const int oh = rem / a.Wo, ow = rem - oh * a.Wo;
        a_img[i] = a.in + (size_t)n_img * a.H * a.W * a.Cs_in + a.coff_in;
        a_ih0[i] = ok ? oh * a.stride - a.pad : -(1 << 20);
        a_iw0[i] = ow * a.stride - a.pad;
        if (POOL) {   // first row / column of the pooling window (always inside the image: Caffe's ceil rule)
            a_ih0[i] = ok ? oh * a.pool_s : -(1 << 20);
            a_iw0[i] = ow * a.pool_s;
        }
    }
    const float* b_ptr[NB];
    bool b_ok[NB];
    int b_row[NB], b_col[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int c = tid + 256 * i;
        b_row[i] = c / CPR;
        b_col[i] = c % CPR;
        const int n = n0 + b_row[i];
        b_ok[i] = n < a.Cout && b_row[i] < BN;
        b_ptr[i] = a.w + (size_t)(b_ok[i] ? n : 0) * a.Kp + b_col[i] * 4 + kbeg;
    }

    floatx4 ra[NA], rb[NB];   // ext-vector values (a HIP float4 struct copy becomes a memcpy the optimiser leaves in scratch)
    constexpr int PT = POOL ? 8 : 1;
    floatx4 rp[NA][PT];       // POOL: the other window taps, in flight under the MFMAs; folded into ra when the tile is stored
    int kh = 0, kw = 0, c0 = 0;   // aligned mode: walk (tap, channel chunk) without divisions
    if (!SMALL_CIN && kbeg > 0) {  // a later K slice starts its walk in the middle
        const int tap0 = kbeg / a.Cin;
        c0 = kbeg - tap0 * a.Cin;
        kh = tap0 / a.kw;
        kw = tap0 - kh * a.kw;
    }
    // Every lane always issues its loads: lanes that fall into the zero padding (or past M / Cout) read the
    // zero page instead, so there is no branch and no exec-mask juggling around the global loads.
    // (Macros, not lambdas: by-reference captures of the staging arrays ended up in scratch memory.)
#define VQ_LOAD_TILES(KC)                                                                                          \
    {                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                           \
            const float* src = a.zeros;                                                                            \
            if (SMALL_CIN) {                                                                                       \
                const int kidx = ((KC) * CPR + a_col[i]) * 4;                                                      \
                const int tap = kidx / a.Cin, c = kidx - tap * a.Cin;                                              \
                const int th = tap / a.kw, tw = tap - th * a.kw;                                                   \
                const int ih = a_ih0[i] + th, iw = a_iw0[i] + tw;                                                  \
                if (tap < a.k * a.kw && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)              \
                    src = a_img[i] + ((size_t)ih * a.W + iw) * a.Cs_in + c;                                        \
            } else if (POOL) {                                                                                     \
                /* 3x3 window: taps outside the image re-read the window's first pixel (max is unchanged) */      \
                const bool ok = a_ih0[i] >= 0;                                                                     \
                if (ok) src = a_img[i] + ((size_t)a_ih0[i] * a.W + a_iw0[i]) * a.Cs_in + c0 + a_col[i] * a.col_off; \
                _Pragma("unroll") for (int t = 1; t < 9; ++t) {                                                    \
                    const int ih = a_ih0[i] + t / 3, iw = a_iw0[i] + t % 3;                                        \
                    const float* q = src;                                                                          \
                    if (ok && ih < a.H && iw < a.W) q = a_img[i] + ((size_t)ih * a.W + iw) * a.Cs_in + c0 + a_col[i] * a.col_off; \
                    rp[i][t - 1] = *reinterpret_cast<const floatx4*>(q);                                           \
                }                                                                                                  \
            } else {                                                                                               \
                const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;                                                  \
                if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)                                  \
                    src = a_img[i] + ((size_t)ih * a.W + iw) * a.Cs_in + c0 + a_col[i] * a.col_off;                \
            }                                                                                                      \
            ra[i] = *reinterpret_cast<const floatx4*>(src);                                                        \
        }                                                                                                          \
        _Pragma("unroll") for (int i = 0; i < NB; ++i)                                                             \
            rb[i] = *reinterpret_cast<const floatx4*>(b_ok[i] ? b_ptr[i] + (size_t)(KC) * BK : a.zeros);           \
        if (!SMALL_CIN) {                                                                                          \
            c0 += a.c_step ? a.c_step : BK;                                                                        \
            if (c0 >= a.Cin) {                                                                                     \
                c0 = 0;                                                                                            \
                if (++kw == a.kw) {                                                                                \
                    kw = 0;                                                                                        \
                    ++kh;                                                                                          \
                }                                                                                                  \
            }                                                                                                      \
        }                                                                                                          \
    }
#define VQ_STORE_TILES(BUF)                                                                                        \
    {                                                                                                              \
        if (POOL) {                                                                                                \
            _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                         \
                _Pragma("unroll") for (int t = 0; t < 8; ++t)                                                      \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) ra[i][e] = fmaxf(ra[i][e], rp[i][t][e]);         \
        }                                                                                                          \
        _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                             \
            if ((BM * CPR) % 256 == 0 || a_row[i] < BM)                                                            \
                *reinterpret_cast<floatx4*>(&sm.a[BUF][a_row[i]][a_col[i] * 4]) = ra[i];                           \
        _Pragma("unroll") for (int i = 0; i < NB; ++i)                                                             \
            if ((BN * CPR) % 256 == 0 || b_row[i] < BN)                                                            \
                *reinterpret_cast<floatx4*>(&sm.b[BUF][b_row[i]][b_col[i] * 4]) = rb[i];                           \
    }

    // ---- compute roles
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int arow0 = wm * (BM / WM) + l31, brow0 = wn * (BN / WN) + l31;
    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // folded-BN bias of this lane's output columns: fetched now so that its latency (and its vmcnt wait)
    // is long gone when the epilogue starts -- a load inside the store loop would serialise every store
    floatx4 bias_v[TN];   // this lane's 4 output channels in the transposed store (see VQ_EPILOGUE)
    ConvSeg seg_v[TN];    // where each 32-column group of this wave goes (wave-uniform)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb_ = n0 + wn * (BN / WN) + 32 * j;
        const int n = nb_ + (lane & 7) * 4;
        bias_v[j] = *reinterpret_cast<const floatx4*>(a.bias + (n < a.Cout ? n : 0));
        seg_v[j] = a.segs[ks * a.seg_stride + (nb_ < a.Cout ? nb_ >> 5 : 0)];
    }

    const int nk = (a.ksplit > 1 ? a.k_per : a.Kp) / BK;
    VQ_LOAD_TILES(0)
    VQ_STORE_TILES(0)
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nk) VQ_LOAD_TILES(kc + 1)   // global loads in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            // lane (row r, half h) holds k = 8 kk + 4 h + j for MFMA step j: the two halves of a step cover a
            // k pair {8kk + j, 8kk + 4 + j}; A and B use the same assignment, so every k is summed once.
            floatx4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const floatx4*>(&sm.a[buf][arow0 + 32 * i][kk * 8 + half * 4]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const floatx4*>(&sm.b[buf][brow0 + 32 * j][kk * 8 + half * 4]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        }
        if (kc + 1 < nk) VQ_STORE_TILES(buf ^ 1)
        __syncthreads();
    }

    VQ_EPILOGUE()
#undef VQ_LOAD_TILES
#undef VQ_STORE_TILES
}

// ------------------------------------------------------------------------------------------------
// Software-pipelined variant (aligned Cin only).  Same tiles, same k order (bit-identical results), but the
// instruction stream of a K-step is laid out by hand: every MFMA is followed by one small slice of the side
// work -- a fragment prefetch for the next 8-wide k group, one global load (with its address arithmetic) of the
// next tile, or one LDS store of it -- and a scheduling fence, so a wave keeps its SIMD's matrix pipe fed
// while it stages (an in-order wave cannot overlap a BLOCK of vector work with more than one MFMA).
// ------------------------------------------------------------------------------------------------
// (round 6: the 128 x 64 x 16 and 64 x 128 x 16 tilings need 134 registers left alone; held to 128 -- no spill -- they fit FOUR workgroups per
// compute unit instead of three: conv1 0.245 -> 0.239 ms, the cfg-2 step in product mode +2 % in alternating builds on one box.  The BK = 32
// tilings of the same area spill 140-232 bytes per lane under that limit and keep their 154-160 registers.)
#ifndef VQ_PIPE_WPE
#define VQ_PIPE_WPE 4
#endif
template <int BM, int BN, int WM, int WN, int BK, bool SMALL_CIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BM * BN == 128 * 64 && BK == 16 ? VQ_PIPE_WPE : 1, 8)))
void conv_igemm_pipe_kernel(ConvArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int NT = 256;                    // threads per workgroup
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int CPR = BK / 4;
    constexpr int NA = (BM * CPR + NT - 1) / NT, NB = (BN * CPR + NT - 1) / NT;
    constexpr int NKK = BK / 8;              // 8-wide k groups per K-step
    constexpr int MFK = 4 * TM * TN;         // MFMAs per k group
    constexpr int NMF = NKK * MFK;           // MFMAs per K-step
    constexpr int NFR = TM + TN;             // fragment reads per k group
    constexpr int NG = NA + NB;              // global loads (= LDS stores) per K-step
    constexpr int NFREE = NMF - (NKK - 1) * NFR;
    static_assert(NFREE >= 2 * NG, "not enough MFMA gaps for the staging slices");
    // EARLY: the LDS stores of tile kc+1 are all issued before the last k group of step kc, so a barrier right behind
    // them lets that last group's gaps prefetch the first fragments of step kc+1: no LDS latency is exposed at the
    // start of a step.
    constexpr bool EARLY = (NKK - 1) * (MFK - NFR) >= NG && NFREE - NFR >= 2 * NG;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    ConvSmem<BM, BN, BK>& sm = *reinterpret_cast<ConvSmem<BM, BN, BK>*>(smem_raw);

    const int tid = threadIdx.x;
    const int n_tiles = a.tiles_m * a.tiles_n;
    const int ks = a.ksplit > 1 ? (int)blockIdx.x / n_tiles : 0;            // K slice of this workgroup (uniform)
    const int kbeg = ks * a.k_per;
    const int tile = xcd_remap(blockIdx.x - ks * n_tiles, n_tiles);
    // Which pixels, which channels: on the scalar unit, with reciprocals from the host (launch_conv_t).  An integer division costs
    // ~30 vector instructions, a third of them at a quarter of the rate, and the vector unit's time is the matrix pipe's: the prologue
    // of a K = 256 tile used to be 11 % of its issue slots.
    const int tm = (int)magic_div((unsigned)tile, a.m_tiles_n);
    const int m0 = tm * BM;
    const int n0 = (tile - tm * a.tiles_n) * BN;
    const unsigned img0 = full_div((unsigned)m0, a.d_howo), rem0 = (unsigned)m0 - img0 * (unsigned)(a.Ho * a.Wo);
    const unsigned oh0 = full_div(rem0, a.d_wo), ow0 = rem0 - oh0 * (unsigned)a.Wo;

    // Staging addresses are 32-bit byte offsets into two buffer descriptors (activation slot, weights).  A lane
    // whose tap falls into the zero padding (or whose row is past M / Cout) uses offset 0xFFFFFFFF: the
    // hardware range check of buffer_load returns zeros, so a load costs one add and one select -- no 64-bit
    // address arithmetic, no branches, no zero page.  Which of the k*k taps are inside the image is a per-pixel
    // bit mask computed once per tile.
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, a.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.w_bytes, 0x00020000);
    int a_off[NA];            // byte offset of (pixel, tap (0,0), channel chunk) -- may be "negative" in the padding
    unsigned long long a_mask[NA];   // bit kh*k+kw set: that tap reads inside the image (k*k <= 64)
    int a_row[NA], a_col[NA];
    const unsigned HW = (unsigned)(a.H * a.W);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int c = tid + NT * i;
        a_row[i] = c / CPR;
        a_col[i] = c % CPR;
        const bool ok = m0 + a_row[i] < a.M && a_row[i] < BM;
        // the a_row-th pixel behind the tile's first one: a walk of < BM pixels (every factor below 2^24, launch_conv_t)
        const unsigned lin = ow0 + (unsigned)a_row[i];
        const unsigned q1 = umul24(lin, a.s_wo) >> kRecipShift;
        const unsigned ly = oh0 + q1;
        const unsigned q2 = umul24(ly, a.s_ho) >> kRecipShift;
        const int ow = (int)(lin - umul24(q1, (unsigned)a.Wo)), oh = (int)(ly - umul24(q2, (unsigned)a.Ho));
        const int ih0 = imul24(oh, a.stride) - a.pad, iw0 = imul24(ow, a.stride) - a.pad;
        // aligned mode: the chunk column is a channel offset inside the tap; small-Cin mode: it selects the tap itself
        a_off[i] = (imul24((int)umul24(img0 + q2, HW) + imul24(ih0, a.W) + iw0, a.Cs_in) + a.coff_in + (SMALL_CIN ? 0 : imul24(a_col[i], a.col_off))) * 4;
        unsigned long long mask = 0;
        for (int th = 0; th < a.k; ++th)
            for (int tw = 0; tw < a.kw; ++tw)
                if (ok && (unsigned)(ih0 + th) < (unsigned)a.H && (unsigned)(iw0 + tw) < (unsigned)a.W) mask |= 1ull << (th * a.kw + tw);
        a_mask[i] = mask;
    }
    unsigned b_off[NB];
    int b_row[NB], b_col[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int c = tid + NT * i;
        b_row[i] = c / CPR;
        b_col[i] = c % CPR;
        const int n = n0 + b_row[i];
        b_off[i] = (n < a.Cout && b_row[i] < BN) ? (unsigned)((imul24(n, a.Kp) + b_col[i] * 4 + kbeg) * 4) : 0xFFFFFFFFu;
    }

    floatx4 ra[2][NA], rb[2][NB];   // two staging sets: tile kc+1 waits in one while tile kc+2 is fetched into the other
    int kh = 0, kw = 0, c0 = 0, tap = 0;
    // Aligned mode: the address of a staged chunk is (pixel + tap) [per lane, changes only when the tap changes] +
    // c0 [uniform, changes every step].  The first part lives in a_voff (0xFFFFFFFF when the tap falls into the
    // padding) and is recomputed on tap changes only; the second rides in the scalar offset of the buffer load, which
    // the hardware range check accounts for.  The VALU and the matrix pipe share issue bandwidth
    // (tools/ubench/mfma_coissue.hip), so the steady state of the K loop carries no address arithmetic at all.
    unsigned a_voff[NA];
    if (!SMALL_CIN && kbeg > 0) {   // a later K slice starts its walk in the middle
        tap = kbeg / a.Cin;
        c0 = kbeg - tap * a.Cin;
        kh = tap / a.kw;
        kw = tap - kh * a.kw;
    }
    {
        const int tap_pix0 = ((kh * a.W + kw) * a.Cs_in) * 4;
#pragma unroll
        for (int i = 0; i < NA; ++i) a_voff[i] = ((a_mask[i] >> tap) & 1ull) ? (unsigned)(a_off[i] + tap_pix0) : 0xFFFFFFFFu;
    }
    const int c_step = a.c_step ? a.c_step : BK;
    const unsigned cpt = (unsigned)a.Cin >> 2, inv_cpt = 65536u / cpt + 1u, inv_k = 65536u / (unsigned)a.kw + 1u;   // small-Cin decode

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int arow0 = wm * (BM / WM) + l31, brow0 = wn * (BN / WN) + l31;
    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    floatx4 bias_v[TN];   // this lane's 4 output channels in the transposed store (see VQ_EPILOGUE_BUF)
    ConvSeg seg_v[TN];    // where each 32-column group of this wave goes (wave-uniform: scalar loads)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb_ = n0 + wn * (BN / WN) + 32 * j;
        const int n = nb_ + (lane & 7) * 4;
        bias_v[j] = *reinterpret_cast<const floatx4*>(a.bias + (n < a.Cout ? n : 0));
        seg_v[j] = a.segs[ks * a.seg_stride + (nb_ < a.Cout ? nb_ >> 5 : 0)];
    }

// Small-Cin mode (the 7x7 stem: Cin padded to 4 or 12): a 32-wide K-step spans several taps, so every staged
// 16-byte chunk decodes its own tap from its K index -- g = KC * CPR + column, tap = g / (Cin/4), (th, tw) = tap / k,
// tap % k -- with multiply-shift divisions (exact for the < 2^10 values that occur).
#define VQ_G_LOAD(IDX, KC, SET)                                                                                \
    {                                                                                                          \
        if ((IDX) < NA) {                                                                                      \
            const int ii = (IDX) < NA ? (IDX) : 0;                                                             \
            unsigned off;                                                                                      \
            if (SMALL_CIN) {                                                                                   \
                const unsigned g_ = (unsigned)(KC) * CPR + a_col[ii];                                          \
                const unsigned tap_ = (g_ * inv_cpt) >> 16, c4_ = g_ - tap_ * cpt;                             \
                const unsigned th_ = (tap_ * inv_k) >> 16, tw_ = tap_ - th_ * a.kw;                            \
                const unsigned ok_ = (unsigned)(a_mask[ii] >> (tap_ & 63u)) & (tap_ < 64u ? 1u : 0u);          \
                off = ok_ ? (unsigned)(a_off[ii] + (int)(((th_ * a.W + tw_) * a.Cs_in + c4_ * 4) * 4)) : 0xFFFFFFFFu; \
            } else {                                                                                           \
                off = a_voff[ii];                                                                              \
            }                                                                                                  \
            ra[SET][ii] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, off, SMALL_CIN ? 0 : c0 * 4, 0)); \
        } else {                                                                                               \
            const int ii = (IDX) >= NA ? (IDX) - NA : 0;                                                       \
            rb[SET][ii] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_off[ii], (KC) * (BK * 4), 0)); \
        }                                                                                                      \
    }
#define VQ_G_STORE(IDX, BUF, SET)                                                                              \
    {                                                                                                          \
        if ((IDX) < NA) {                                                                                      \
            const int ii = (IDX) < NA ? (IDX) : 0;                                                             \
            if ((BM * CPR) % NT == 0 || a_row[ii] < BM)                                                        \
                *reinterpret_cast<floatx4*>(&sm.a[BUF][a_row[ii]][a_col[ii] * 4]) = ra[SET][ii];               \
        } else {                                                                                               \
            const int ii = (IDX) >= NA ? (IDX) - NA : 0;                                                       \
            if ((BN * CPR) % NT == 0 || b_row[ii] < BN)                                                        \
                *reinterpret_cast<floatx4*>(&sm.b[BUF][b_row[ii]][b_col[ii] * 4]) = rb[SET][ii];               \
        }                                                                                                      \
    }
#define VQ_ADVANCE_TAP()                                                                     \
    if (!SMALL_CIN) {                                                                        \
        c0 += c_step;                                                                        \
        if (c0 >= a.Cin) {                                                                   \
            c0 = 0;                                                                          \
            ++tap;                                                                           \
            if (++kw == a.kw) {                                                              \
                kw = 0;                                                                      \
                ++kh;                                                                        \
            }                                                                                \
            asm volatile("" ::: "memory"); /* keep this a (rarely taken, uniform) branch: if-converted, the    \
                                              recomputation below would run on every step */                 \
            const int tap_pix = ((kh * a.W + kw) * a.Cs_in) * 4;                             \
            _Pragma("unroll") for (int i = 0; i < NA; ++i)                                   \
                a_voff[i] = ((a_mask[i] >> tap) & 1ull) ? (unsigned)(a_off[i] + tap_pix) : 0xFFFFFFFFu; \
        }                                                                                    \
    }
// One K-step on LDS buffer BUF (compute on tile KC); its first fragments are already in fa[0] / fb[0].
// DO_STORE: tile KC+1, fetched during the previous step into staging set SS, goes to LDS buffer BUF^1 behind the first
// MFMAs (a whole K-step after its loads were issued, so the vmcnt wait in front of the LDS store does not stall); with
// EARLY a barrier follows the last of these stores and the last k group prefetches the first fragments of step KC+1.
// DO_LOAD: tile KC+2 is fetched into staging set SL.
#define VQ_PIPE_STEP(BUF, KC, DO_STORE, DO_LOAD, SS, SL)                                                       \
    {                                                                                                          \
        if (!EARLY) {                                                                                          \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
                fa[0][i] = *reinterpret_cast<const floatx4*>(&sm.a[BUF][arow0 + 32 * i][half * 4]);            \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                fb[0][j] = *reinterpret_cast<const floatx4*>(&sm.b[BUF][brow0 + 32 * j][half * 4]);            \
        }                                                                                                      \
        _Pragma("unroll") for (int q = 0; q < NMF; ++q) {                                                      \
            const int kk = q / MFK, r = q % MFK, s_ = r / (TM * TN), i_ = (r / TN) % TM, j_ = r % TN;          \
            acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk & 1][i_][s_], fb[kk & 1][j_][s_], acc[i_][j_], 0, 0, 0); \
            if (kk + 1 < NKK && r < NFR) {                                                                     \
                if (r < TM)                                                                                    \
                    fa[(kk + 1) & 1][r < TM ? r : 0] = *reinterpret_cast<const floatx4*>(                      \
                        &sm.a[BUF][arow0 + 32 * (r < TM ? r : 0)][(kk + 1) * 8 + half * 4]);                   \
                else                                                                                           \
                    fb[(kk + 1) & 1][r >= TM ? r - TM : 0] = *reinterpret_cast<const floatx4*>(                \
                        &sm.b[BUF][brow0 + 32 * (r >= TM ? r - TM : 0)][(kk + 1) * 8 + half * 4]);             \
            } else if (EARLY && (DO_STORE) && kk + 1 == NKK && r < NFR) {                                      \
                if (r < TM)                                                                                    \
                    fa[0][r < TM ? r : 0] = *reinterpret_cast<const floatx4*>(                                 \
                        &sm.a[(BUF) ^ 1][arow0 + 32 * (r < TM ? r : 0)][half * 4]);                            \
                else                                                                                           \
                    fb[0][r >= TM ? r - TM : 0] = *reinterpret_cast<const floatx4*>(                           \
                        &sm.b[(BUF) ^ 1][brow0 + 32 * (r >= TM ? r - TM : 0)][half * 4]);                      \
            } else {                                                                                           \
                const int fidx = q - (kk + 1 < NKK ? (kk + 1) * NFR : (NKK - 1) * NFR + (EARLY && (DO_STORE) ? NFR : 0)); \
                if ((DO_STORE) && fidx < NG) {                                                                 \
                    VQ_G_STORE(fidx < NG ? fidx : 0, (BUF) ^ 1, SS)                                            \
                    if (EARLY && fidx == NG - 1) __syncthreads(); /* tile KC+1 is complete in LDS */           \
                } else if ((DO_LOAD) && fidx >= NG && fidx < 2 * NG)                                           \
                    VQ_G_LOAD(fidx - NG < NG ? fidx - NG : 0, (KC) + 2, SL)                                    \
            }                                                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                                 \
        }                                                                                                      \
    }

    const int nk = (a.ksplit > 1 ? a.k_per : a.Kp) / BK;
    _Pragma("unroll") for (int i = 0; i < NG; ++i) VQ_G_LOAD(i, 0, 0)
    _Pragma("unroll") for (int i = 0; i < NG; ++i) VQ_G_STORE(i, 0, 0)
    if (nk > 1) {
        VQ_ADVANCE_TAP()              // (tap, c0) now address tile 1
        _Pragma("unroll") for (int i = 0; i < NG; ++i) VQ_G_LOAD(i, 1, 1)
    }
    __syncthreads();
    floatx4 fa[2][TM], fb[2][TN];     // MFMA operand fragments, double-buffered over the 8-wide k groups
    if (EARLY) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[0][i] = *reinterpret_cast<const floatx4*>(&sm.a[0][arow0 + 32 * i][half * 4]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[0][j] = *reinterpret_cast<const floatx4*>(&sm.b[0][brow0 + 32 * j][half * 4]);
    }
    // Steady state (steps 0 .. nk-3: store tile kc+1, fetch tile kc+2), unrolled by two so that the staging sets have
    // static names, as a straight-line pair with no exit in the middle (a mid-loop exit made the register allocator
    // shuttle the accumulators between VGPRs and AGPRs on every trip).
    // End-of-step barrier: every wave is done READING buffer b before anybody stores tile kc+2 into it.  With EARLY
    // the only LDS operations still in flight are the NFR fragment prefetches of the next step (from the other
    // buffer), so the wait is counted and the barrier raw -- a full __syncthreads() would wait for those prefetches
    // and put the LDS latency right back in front of the next step's first MFMA.
#define VQ_END_BARRIER()                                                     \
    {                                                                        \
        if (EARLY) {                                                         \
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NFR) : "memory");     \
            __builtin_amdgcn_s_barrier();                                    \
            asm volatile("" ::: "memory");                                   \
        } else {                                                             \
            __syncthreads();                                                 \
        }                                                                    \
    }
    const int n_steady = nk > 2 ? nk - 2 : 0;
    int kc = 0;
    for (; kc + 1 < n_steady; kc += 2) {
        VQ_ADVANCE_TAP()              // tile kc + 2
        VQ_PIPE_STEP(0, kc, true, true, 1, 0)
        VQ_END_BARRIER()
        VQ_ADVANCE_TAP()              // tile kc + 3
        VQ_PIPE_STEP(1, kc + 1, true, true, 0, 1)
        VQ_END_BARRIER()
    }
    if (kc < n_steady) {              // odd number of steady steps: one more even-indexed step
        VQ_ADVANCE_TAP()
        VQ_PIPE_STEP(0, kc, true, true, 1, 0)
        VQ_END_BARRIER()
        ++kc;
    }
    // tail: the step that still has a successor to store (nothing left to fetch), then the last step
    if (kc + 1 < nk) {
        if (kc & 1) {
            VQ_PIPE_STEP(1, kc, true, false, 0, 0)
        } else {
            VQ_PIPE_STEP(0, kc, true, false, 1, 1)
        }
        VQ_END_BARRIER()
        ++kc;
    }
    if (kc & 1) {
        VQ_PIPE_STEP(1, kc, false, false, 0, 0)
    } else {
        VQ_PIPE_STEP(0, kc, false, false, 0, 0)
    }
    VQ_EPILOGUE_BUF()
#undef VQ_G_LOAD
#undef VQ_G_STORE
#undef VQ_ADVANCE_TAP
#undef VQ_PIPE_STEP
#undef VQ_END_BARRIER
}

// ------------------------------------------------------------------------------------------------
// max-pool + 1x1 convolution with the pooled activations of a workgroup resident in LDS (the stem pools: pool1 ->
// conv2/3x3_reduce, pool2 -> the sibling 1x1 group of inception_3a).  The POOL instantiation of conv_igemm_kernel above stages
// BOTH operands through a double-buffered LDS ring, K-step by K-step.  Here
//   * the pooled image of the workgroup's BM pixels is written ONCE, slab by slab (32 channels of BM = 64 pixels), into a
//     [BM][K] LDS image that is never overwritten -- so there is no ring and only one barrier per slab;
//   * the 18 tap loads of slab s + 1 are in flight under the MFMAs of slab s (64 per wave on the 64 x 256 tile), their maxima
//     (v_max3) and two ds_write_b128 follow those MFMAs;
//   * the weight fragments go straight from L2 into registers one k-group ahead: every wave owns its own BN / WN output
//     columns, nothing about the weights is shared inside a workgroup, so no LDS stage and no barrier exists for them.
// Measured on pool2 -> inception_3a (75 264 x 224 x 192 at 96 crops): the pooling stream alone takes 0.061 ms, the GEMM alone
// 0.069 ms; un-overlapped (all maxima first, then the GEMM; or the K-step ring of conv_igemm_kernel) 0.111 ms.
// Same k order per output element as every other direct kernel (k-groups of 8 ascending, pairs {s, 4 + s} inside): same bits.
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void pool_gemm_kernel(ConvArgs a) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(BM == 64 || BM == 128, "two staged chunks per thread and slab");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int SLAB = 2048 / BM;                              // channels per slab: 512 16-byte chunks = 2 per thread
    constexpr int CPS = SLAB / 4;                                // chunks per row and slab
    constexpr int GS = SLAB / 8;                                 // k-groups per slab (2 or 4)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* As = reinterpret_cast<float*>(smem_raw);               // [BM][K + 4]: rows 16 bytes longer than K -> conflict-free b128 reads
    const int K = a.Cin, pitch = K + 4;
    const int tid = threadIdx.x;
    const int tile = xcd_remap(blockIdx.x, a.tiles_m * a.tiles_n);
    const int m0 = (tile / a.tiles_n) * BM, n0 = (tile % a.tiles_n) * BN;
    const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, a.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.w_bytes, 0x00020000);

    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    floatx4 bias_v[TN];
    ConvSeg seg_v[TN];
    unsigned b_voff[TN];                                          // this lane's weight row, k = 4 half: + 32 bytes per k-group
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb_ = n0 + wn * (BN / WN) + 32 * j;
        const int n = nb_ + (lane & 7) * 4;
        bias_v[j] = *reinterpret_cast<const floatx4*>(a.bias + (n < a.Cout ? n : 0));
        seg_v[j] = a.segs[nb_ < a.Cout ? nb_ >> 5 : 0];
        b_voff[j] = nb_ + l31 < a.Cout ? (unsigned)(((nb_ + l31) * a.Kp + half * 4) * 4) : 0xFFFFFFFFu;
    }

    // ---- staging role: chunk u of a slab = row (tid + 256 u) / CPS, 16-byte column (tid + 256 u) % CPS -- the same two rows for
    // every slab, so the nine tap offsets of each are computed once (a tap outside the image re-reads the window's first pixel:
    // the maximum is unchanged; a row past M reads zeros through the range check) and a slab adds its scalar channel offset
    unsigned tap_base[2], tap_ok[2];                               // first window pixel (0xFFFFFFFF: row past M); bit t: tap t is inside the image
    int a_dst[2];
    const int px = a.Cs_in * 4, rowb = a.W * px;                   // bytes to the next pixel / next image row (uniform)
    {
        const int HoWo = a.Ho * a.Wo;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, row = idx / CPS, col = idx % CPS;
            const int m = m0 + row;
            const bool ok = m < a.M;
            const int mm = ok ? m : 0;
            const int n_img = mm / HoWo, rem = mm - n_img * HoWo;
            const int oh = rem / a.Wo, ow = rem - oh * a.Wo;
            const int ih0 = oh * a.pool_s, iw0 = ow * a.pool_s;
            tap_base[u] = ok ? (unsigned)((((n_img * a.H + ih0) * a.W + iw0) * a.Cs_in + a.coff_in + col * 4) * 4) : 0xFFFFFFFFu;
            const int nvy = min(3, a.H - ih0), nvx = min(3, a.W - iw0);
            unsigned mask = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t)
                if (ok && t / 3 < nvy && t % 3 < nvx) mask |= 1u << t;
            tap_ok[u] = mask;
            a_dst[u] = row * pitch + col * 4;
        }
    }
    floatx4 v[2][9];
#define VQ_PG_TAPS(S)                                                                                               \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                 \
        unsigned inside = tap_ok[u];                                                                                \
        asm volatile("" : "+v"(inside)); /* opaque: the 18 offsets must not be hoisted out of the slab loop into registers */ \
        _Pragma("unroll") for (int t = 0; t < 9; ++t)                                                               \
            v[u][t] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(                            \
                in_rsrc, tap_base[u] + (((inside >> t) & 1u) ? (unsigned)((t / 3) * rowb + (t % 3) * px) : 0u), (S) * (SLAB * 4), 0)); \
    }
#define VQ_PG_POOL(S)                                                                                               \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                 \
        floatx4 r;                                                                                                  \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                             \
            const float x = __builtin_fmaxf(__builtin_fmaxf(v[u][0][e], v[u][1][e]), v[u][2][e]);                  \
            const float y = __builtin_fmaxf(__builtin_fmaxf(v[u][3][e], v[u][4][e]), v[u][5][e]);                  \
            const float z = __builtin_fmaxf(__builtin_fmaxf(v[u][6][e], v[u][7][e]), v[u][8][e]);                  \
            r[e] = __builtin_fmaxf(__builtin_fmaxf(x, y), z);                                                       \
        }                                                                                                           \
        *reinterpret_cast<floatx4*>(As + a_dst[u] + (S) * SLAB) = r;                                                \
    }

    // ---- compute role.  Lane (row r, half h) holds k = 8 g + 4 h + s for MFMA step s of k-group g, as in conv_igemm_kernel.
    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const float* a_frag = As + (wm * (BM / WM) + l31) * pitch + half * 4;      // + 32 i rows, + 8 g floats
    // A wave's vector-memory loads return IN ORDER as far as s_waitcnt vmcnt can tell: a weight fragment fetched behind the 18 tap
    // loads of the next slab could not be consumed before every one of those (HBM) loads had landed -- the first form of this loop did
    // that, and the memory stream and the matrix pipe took turns (0.108 ms for 0.061 + 0.069).  So ALL weight fragments of slab s + 1 are
    // requested FIRST (8 loads, a second register set), the taps of slab s + 1 behind them; the MFMAs of slab s then touch only
    // registers that arrived before the previous slab's closing wait and LDS (lgkmcnt): no vmcnt wait inside a slab.
    floatx4 fa[2][TM], fbs[2][GS][TN];
#define VQ_PG_FETCH_B(SET, S)                                                                                       \
    _Pragma("unroll") for (int q = 0; q < GS; ++q)                                                                  \
        _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                              \
            fbs[SET][q][j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_voff[j], ((S) * GS + q) * 32, 0));
#define VQ_PG_FETCH_A(SET, G)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                  \
        fa[SET][i] = *reinterpret_cast<const floatx4*>(a_frag + 32 * i * pitch + (G) * 8);
#define VQ_PG_MFMA(SET, BSET, Q)                                                                                    \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_)                                                                \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                              \
            _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                          \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][i][s_], fbs[BSET][Q][j][s_], acc[i][j], 0, 0, 0);
// one slab: BSET = the register set its weight fragments are in (slab parity)
#define VQ_PG_SLAB(S, BSET)                                                                                         \
    {                                                                                                               \
        const bool more = (S) + 1 < ns;                                                                             \
        if (more) {                                                                                                 \
            VQ_PG_FETCH_B((BSET) ^ 1, (S) + 1)                                                                      \
            VQ_PG_TAPS((S) + 1)                              /* in flight under this slab's MFMAs */                \
        }                                                                                                           \
        VQ_PG_FETCH_A(0, (S) * GS)                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
        _Pragma("unroll") for (int q = 0; q < GS; ++q) {                                                            \
            if (q + 1 < GS) VQ_PG_FETCH_A((q + 1) & 1, (S) * GS + q + 1)                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                      \
            VQ_PG_MFMA(q & 1, BSET, q)                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                      \
        }                                                                                                           \
        if (more) {                                                                                                 \
            VQ_PG_POOL((S) + 1)                                                                                     \
            __syncthreads();                                 /* slab S + 1 is complete in LDS (nothing is ever overwritten) */ \
        }                                                                                                           \
    }

    const int ns = K / SLAB;
    VQ_PG_FETCH_B(0, 0)
    VQ_PG_TAPS(0)
    VQ_PG_POOL(0)
    __syncthreads();
    int s = 0;
    for (; s + 1 < ns; s += 2) {                                   // by two: the weight register sets have static names
        VQ_PG_SLAB(s, 0)
        VQ_PG_SLAB(s + 1, 1)
    }
    if (s < ns) VQ_PG_SLAB(s, 0)
#undef VQ_PG_SLAB
#undef VQ_PG_TAPS
#undef VQ_PG_POOL
#undef VQ_PG_FETCH_A
#undef VQ_PG_FETCH_B
#undef VQ_PG_MFMA
    VQ_EPILOGUE()
}

// ------------------------------------------------------------------------------------------------
// host side: one launch per instantiation, the table of tilings, which kernel serves a tiling
// ------------------------------------------------------------------------------------------------
// The kernels of a direct convolution: the plain kernel, the software-pipelined one, the plain kernel with the pooled-input
// loader, and the two-phase pool_gemm_kernel
enum : int { kConv = 1, kPipe = 2, kPool = 4, kGemm = 8 };

constexpr size_t kPoolGemmMaxLds = 64 * 1024;                  // pool_gemm_kernel: BM x (K + 4) floats, two or three workgroups per unit
size_t vq::pool_gemm_lds(int bm, int K) { return std::max((size_t)bm * (K + 4) * sizeof(float), (size_t)4 * 32 * 36 * sizeof(float)); }

// The pipelined kernel decodes pixels with host-made reciprocals on 24-bit multiplies: what the shapes must satisfy
static bool pixel_walk_ok(const ConvArgs& a) {
    const long long n_img = cdiv(a.M, a.Ho * a.Wo);
    return n_img * a.H * a.W < (1 << 23) && a.Cs_in < (1 << 23) && a.Kp < (1 << 23) && a.Cout < (1 << 23) && a.stride < (1 << 23) &&
           recip22_ok((unsigned)a.Wo, (unsigned)a.Wo + 128u) && recip22_ok((unsigned)a.Ho, (unsigned)a.Ho + 130u);
}

template <int BM, int BN, int WM, int WN, int BK, int KERNEL, bool SMALL>
static int launch_conv_t(ConvArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    a.tiles_m = cdiv(a.M, BM);
    a.tiles_n = cdiv(a.Cout, BN);
    void (*kern)(ConvArgs);
    size_t lds = sizeof(ConvSmem<BM, BN, BK>), lds_max = lds;
    if constexpr (KERNEL == kPipe) {
        VQ_REQUIRE(pixel_walk_ok(a) && (unsigned long long)a.tiles_m * a.tiles_n * a.tiles_n < 0x100000000ull,
                   "pipelined convolution: shape outside the range of its reciprocal divisions");
        a.m_tiles_n = a.tiles_n == 1 ? 0u : (unsigned)(0x100000000ull / (unsigned)a.tiles_n) + 1u;
        a.d_howo = full_div_for((unsigned)(a.Ho * a.Wo));
        a.d_wo = full_div_for((unsigned)a.Wo);
        a.s_wo = recip22((unsigned)a.Wo);
        a.s_ho = recip22((unsigned)a.Ho);
        kern = conv_igemm_pipe_kernel<BM, BN, WM, WN, BK, SMALL>;
    } else if constexpr (KERNEL == kGemm) {
        VQ_REQUIRE(a.pool_k == 3 && a.Cin % 32 == 0 && a.Kp == a.Cin, "pool_gemm_kernel: a 3x3 window over a multiple of 32 channels");
        kern = pool_gemm_kernel<BM, BN, WM, WN>;
        lds = pool_gemm_lds(BM, a.Cin);                     // a launch asks for what its K needs
        lds_max = kPoolGemmMaxLds;
    } else {
        kern = conv_igemm_kernel<BM, BN, WM, WN, BK, SMALL, KERNEL == kPool>;
    }
    VQ_DYN_LDS(kern, lds_max);            // per instantiation and device
    VQ_LAUNCH(kern, a.tiles_m * a.tiles_n * a.ksplit, 256, lds, stream, ev_start, ev_stop, a);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

// An entry of kTiles: the tiling and launches of the kernels HAS names (kPipe brings the plain kernel along)
template <int BM, int BN, int BK, int WM, int WN, int HAS>
constexpr ConvTile tiling() {
    ConvTile t{BM, BN, BK, (HAS & kGemm) ? 3 : (HAS & kPipe) ? 1 : 0, {}, {}, nullptr};
    if constexpr ((HAS & (kConv | kPipe)) != 0) {
        t.conv[0] = launch_conv_t<BM, BN, WM, WN, BK, kConv, false>;
        t.conv[1] = launch_conv_t<BM, BN, WM, WN, BK, kConv, true>;
    }
    if constexpr ((HAS & kPipe) != 0) {
        t.piped[0] = launch_conv_t<BM, BN, WM, WN, BK, kPipe, false>;
        t.piped[1] = launch_conv_t<BM, BN, WM, WN, BK, kPipe, true>;
    }
    if constexpr ((HAS & kPool) != 0) t.pooled = launch_conv_t<BM, BN, WM, WN, BK, kPool, false>;
    if constexpr ((HAS & kGemm) != 0) t.pooled = launch_conv_t<BM, BN, WM, WN, BK, kGemm, false>;
    return t;
}

// Candidate tilings: BM x BN x BK on four waves of WM x WN, and the kernels each has.  Every candidate sums each output element's
// K terms in the same order, so the choice never changes a result bit; it is made per layer and batch size by timing (autotune) or,
// with VQ_TSN_AUTOTUNE=0, by the occupancy heuristic (vq_tsn.hip).  Both take the first of equals in this order.
// The pooled loader keeps 8 extra window taps per staged chunk in registers: tilings that stage at most two chunks per thread have it.
static constexpr ConvTile kTable[] = {
    tiling<128, 128, 32, 2, 2, kConv>(), tiling<128, 128, 16, 2, 2, kConv | kPool>(),
    tiling<128, 96, 32, 4, 1, kConv>(),  tiling<128, 96, 16, 4, 1, kConv | kPool>(),
    tiling<128, 64, 32, 2, 2, kConv>(),  tiling<128, 64, 16, 2, 2, kConv | kPool>(),
    tiling<64, 128, 32, 2, 2, kConv | kPool>(), tiling<64, 128, 16, 2, 2, kConv | kPool>(),
    tiling<64, 64, 32, 2, 2, kConv | kPool>(),  tiling<64, 64, 16, 2, 2, kConv | kPool>(),
    tiling<128, 32, 32, 4, 1, kConv>(),  tiling<128, 32, 16, 4, 1, kConv | kPool>(),
    tiling<32, 128, 32, 1, 4, kConv>(),  tiling<32, 128, 16, 1, 4, kConv>(),
    tiling<128, 128, 32, 2, 2, kPipe>(), tiling<128, 128, 16, 2, 2, kPipe>(),
    tiling<128, 96, 32, 4, 1, kPipe>(),  tiling<128, 96, 16, 4, 1, kPipe>(),
    tiling<128, 64, 32, 2, 2, kPipe>(),  tiling<128, 64, 16, 2, 2, kPipe>(),
    tiling<64, 128, 32, 2, 2, kPipe>(),  tiling<64, 128, 16, 2, 2, kPipe>(),
    tiling<64, 64, 32, 2, 2, kPipe>(),   tiling<64, 64, 16, 2, 2, kPipe>(),
    tiling<128, 32, 32, 4, 1, kPipe>(),  tiling<128, 32, 16, 4, 1, kPipe>(),
    tiling<32, 128, 32, 1, 4, kPipe>(),  tiling<32, 128, 16, 1, 4, kPipe>(),
    // (round 6: 256 x 64 tilings -- four waves of 64 x 64 one above the other, for the 64-channel stem with its short K -- were built, tested
    // against the oracle and offered to the sweep: never chosen, conv1 stays at 0.233-0.238 ms on 128 x 64; removed again.)
    // pooled-input 1x1 layers only: ONE column tile for up to 256 output columns (every pooling window is read once), and the
    // two-phase kernel
    tiling<64, 256, 16, 1, 4, kPool>(), tiling<64, 256, 8, 1, 4, kGemm>(), tiling<64, 64, 8, 2, 2, kGemm>(), tiling<128, 64, 8, 2, 2, kGemm>()};
const int vq::kNumTiles = (int)(sizeof(kTable) / sizeof(kTable[0]));
#ifndef __HIP_DEVICE_COMPILE__   // host data: a device copy of the table would ask the device linker for the host launches it names
const ConvTile* const vq::kTiles = kTable;
#endif

// The entry of the external form [bm, bn, bk, pipe] of a tiling (vq_tsn_set_tiles, VQ_TSN_TILE); -1: none
int vq::tile_index(int bm, int bn, int bk, int pipe) {
    for (int i = 0; i < kNumTiles; ++i)
        if (kTiles[i].bm == bm && kTiles[i].bn == bn && kTiles[i].bk == bk && kTiles[i].pipe == pipe) return i;
    return -1;
}

// A pooled-input layer of K channels has a kernel under tiling t
bool vq::pooled_ok(const ConvTile& t, int K) { return t.pooled && (t.pipe != 3 || pool_gemm_lds(t.bm, K) <= kPoolGemmMaxLds); }

// The launch that runs tiling ti with arguments a; nullptr: none.  Every substitute gives the same bits.
static ConvLaunch conv_launch(const ConvArgs& a, int ti) {
    const ConvTile* t = &kTiles[ti];
    if (a.pool_k > 0) {
        // max-pool folded into the loader: any tiling gives the same bits, so an unsupported choice (heuristic, VQ_TSN_TILE)
        // is replaced by the BK = 16 tiling of the same shape
        if (!pooled_ok(*t, a.Cin)) ti = tile_index(std::min(t->bm, 128), std::min(t->bn, 128), 16, 0);
        return ti < 0 ? nullptr : kTiles[ti].pooled;
    }
    // the x-major stem (c_step != 0, launch_conv_layer): four chunk columns = four kernel rows: BK = 16 tilings only (same bits for all)
    if (a.c_step != 0) ti = tile_index(t->bm, t->bn, 16, t->pipe);
    if (ti < 0) return nullptr;
    t = &kTiles[ti];
    const bool small = (a.Cin % t->bk) != 0;
    // (shapes outside the pipelined kernel's reciprocal range run the plain kernel of the same tiling: same bits)
    return t->piped[small] && pixel_walk_ok(a) ? t->piped[small] : t->conv[small];
}

int vq::launch_conv(int ti, ConvArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    VQ_REQUIRE(ti >= 0 && ti < kNumTiles, "tiling %d outside the table of %d", ti, kNumTiles);
    const ConvLaunch run = conv_launch(a, ti);
    const ConvTile& t = kTiles[ti];
    if (!run) return fail(VQ_E_INVALID, "no kernel for tile %dx%dx%d pipe=%d", t.bm, t.bn, t.bk, t.pipe);
    return run(a, stream, ev_start, ev_stop);
}
