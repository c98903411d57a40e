// The small kernels of the TSN forward pass on gfx950 -- preprocessing, pooling, global pooling, the class-score layer, the combine
// pass of a K-split convolution, the segment consensus -- each with the host launch that knows its grid (declared in vq_tsn_kernels.h).
#include "vq_common.h"
#include "vq_tsn_kernels.h"

using namespace vq;

typedef float floatx4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// preprocess: uint8 NHWC crops -> fp32 NHWC (channels padded to a multiple of 4), minus mean
// ------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk of the output (4 consecutive channels of one pixel): coalesced float4 stores.
__global__ void preprocess_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t nchunk, int C, int Cpad,
                                  const float* __restrict__ mean) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunk) return;
    const int cpp = Cpad >> 2;                      // chunks per pixel
    const int64_t p = i / cpp;
    const int c0 = (int)(i - p * cpp) * 4;
    floatx4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c0 + e < C ? (float)src[p * C + c0 + e] - mean[c0 + e] : 0.0f;
    *reinterpret_cast<floatx4*>(dst + p * Cpad + c0) = v;
}

// Space-to-depth(2) variant (vq_input_desc.s2d_pad >= 0): slot0[n][Y][X][(p*2+q)*C + c] = crop[2Y+p-pad][2X+q-pad][c] -
// mean[c], zeros outside the crop (the first convolution's own zero padding, applied after the mean like Caffe does).
// One thread per 16-byte chunk of the 4*C output channels of a cell.
__global__ void preprocess_s2d_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t nchunk, int H, int W, int C,
                                      int Hs, int Ws, int pad, const float* __restrict__ mean, int xmajor) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunk) return;
    const int64_t cell = i / C;                     // 4*C channels = C chunks of 4 per cell
    const int j0 = (int)(i - cell * C) * 4;
    const int X = (int)(cell % Ws), Y = (int)((cell / Ws) % Hs);
    const int64_t n = cell / ((int64_t)Ws * Hs);
    floatx4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = j0 + e, pq = j / C, c = j - pq * C;
        const int p = xmajor ? pq & 1 : pq >> 1, q = xmajor ? pq >> 1 : pq & 1;       // s2d_order 1: cell channels (q*2+p)*C + c
        const int y = 2 * Y + p - pad, x = 2 * X + q - pad;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        v[e] = in ? (float)src[((n * H + y) * W + x) * C + c] - mean[c] : 0.0f;
    }
    *reinterpret_cast<floatx4*>(dst + cell * (4 * C) + j0) = v;
}

// The RGB stem's form (C = 3): one thread per CELL -- its 2 x 2 pixels are two runs of 6 bytes, its 12 floats three 16-byte
// stores; two divisions per thread instead of a dozen per chunk (32 us -> 17 us per 96-crop step).  Same values.
__global__ __launch_bounds__(256) void preprocess_s2d3_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t ncell, int H, int W,
                                                              int Hs, int Ws, int pad, const float* __restrict__ mean, int xmajor) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= ncell) return;
    const int X = (int)(cell % Ws);
    const int64_t ny = cell / Ws;
    const int Y = (int)(ny % Hs);
    const int64_t n = ny / Hs;
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
    float v[12];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int y = 2 * Y + p - pad;
        const bool row_in = (unsigned)y < (unsigned)H;
        const uint8_t* r = src + ((n * H + (row_in ? y : 0)) * W) * 3;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int x = 2 * X + q - pad;
            const bool in = row_in && (unsigned)x < (unsigned)W;
            const uint8_t* px = r + (in ? x : 0) * 3;
            const float a = (float)px[0] - m0, b = (float)px[1] - m1, c = (float)px[2] - m2;
            const int slot = xmajor ? q * 2 + p : p * 2 + q;        // s2d_order 1: (q, p, c) -- the x-taps of a kernel row side by side
            v[slot * 3 + 0] = in ? a : 0.0f;
            v[slot * 3 + 1] = in ? b : 0.0f;
            v[slot * 3 + 2] = in ? c : 0.0f;
        }
    }
    floatx4* o = reinterpret_cast<floatx4*>(dst + cell * 12);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        floatx4 t;
        t[0] = v[4 * k], t[1] = v[4 * k + 1], t[2] = v[4 * k + 2], t[3] = v[4 * k + 3];
        o[k] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// pooling (Caffe semantics: ceil-mode output size; MAX ignores padding; AVE divides by the window
// clipped to the padded extent and accumulates h-major in fp32)
// ------------------------------------------------------------------------------------------------
// PoolArgs / pool_one / pool_unit: vq_tsn_kernels.h (shared with the grouped Winograd launch, which also carries a level's pooling)
template <bool IS_MAX>
__global__ __launch_bounds__(256) void pool_kernel(PoolArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.total) pool_one<IS_MAX>(a, i);
}
// a.mode != 0 (pool_plan): the window-specialised path, kPoolPerWG outputs per workgroup -- the code a grouped launch runs
__global__ __launch_bounds__(256) void pool_fast_kernel(PoolArgs a) { pool_unit_any(a, blockIdx.x); }

// global average pool (Caffe AVE, kernel = whole map): sequential fp32 sum over h, w then / (H*W)
__global__ void gavgpool_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int HW, int Cs_in, int coff_in,
                                int C, int Cs_out, int coff_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const int c = i % C, img = i / C;
    const float* p = in + (size_t)img * HW * Cs_in + coff_in + c;
    float acc = 0.f;
    for (int q = 0; q < HW; ++q) acc += p[(size_t)q * Cs_in];
    out[(size_t)img * Cs_out + coff_out + c] = acc / (float)HW;
}

// InnerProduct on 1x1 tensors (fc-action: K = 1024 pooled features -> N = 101 class scores; M = the crops of the launch, 1 .. 960):
//   y[m][n] = b[n] + sum_k x[m][k] * W[n][k],  W [N][K] as Caffe stores it.
// A wave-per-rows VALU kernel, not the matrix pipe: the whole layer is 2 x 960 x 1024 x 101 = 0.2 GFLOP at the largest batch (0.02 at the
// product's 96 crops) against a forward of 200+ GFLOP, so it is bound by launch and load latency, not by arithmetic; the 414 KB of weights
// and <= 4 MB of inputs sit in L2, both operands are read along K -- the contiguous axis of x AND of W, 16 bytes per lane -- so neither
// needs LDS staging or a transposed copy, and N = 101 needs no zero-padded rows.  The fp32-input MFMA forms run at the vector fp32 rate on
// gfx950, and 32 x 32 tiles of v_mfma_f32_32x32x2_f32 would give 120 waves a serial chain of 512 dependent MFMAs each -- an ESTIMATE on
// paper (64 cycles apiece: ~14 us before any load latency, on 120 of the chip's 1024 SIMDs); that form was not built or timed.
// One wave computes FC_ROWS crops x FC_COLS outputs (W values reused FC_ROWS times, x values FC_COLS times from registers).
// SUMMATION ORDER of one output, a function of K alone: lane l owns k = 256 j + 4 l + e (j = 0 .. ceil(K / 256) - 1, e = 0 .. 3) and
// chains acc = fma(x[k], W[n][k], acc) from 0 over j ascending, e ascending (k >= K: skipped); the 64 lane sums then meet in a butterfly
// acc += acc[lane ^ s], s = 32, 16, 8, 4, 2, 1 (fp32 addition commutes, so every lane holds the same bits); last + b[n].
// No accumulator is shared between crops or outputs, rows past M / columns past N recompute the last valid one and store nothing: the
// bits of y[m][:] do not depend on the batch size, the crop's position, the sub-batch split or the crop range of the launch.
constexpr int FC_ROWS = 4;     // x FC_COLS (host/vq_tsn_plan.h)
__global__ __launch_bounds__(64) void inner_product_kernel(const float* __restrict__ x, int x_stride, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ y, int y_stride, int M,
                                                           int K, int N) {
    const int lane = threadIdx.x;
    const int m0 = blockIdx.x * FC_ROWS, n0 = blockIdx.y * FC_COLS;
    const float* xr[FC_ROWS];
    const float* wr[FC_COLS];
#pragma unroll
    for (int r = 0; r < FC_ROWS; ++r) xr[r] = x + (size_t)min(m0 + r, M - 1) * x_stride;
#pragma unroll
    for (int c = 0; c < FC_COLS; ++c) wr[c] = W + (size_t)min(n0 + c, N - 1) * K;
    float acc[FC_ROWS][FC_COLS];
#pragma unroll
    for (int r = 0; r < FC_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < FC_COLS; ++c) acc[r][c] = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {             // K % 4 == 0: a lane's four values are all inside or all outside
        floatx4 xv[FC_ROWS], wv[FC_COLS];
#pragma unroll
        for (int r = 0; r < FC_ROWS; ++r) xv[r] = *reinterpret_cast<const floatx4*>(xr[r] + k);
#pragma unroll
        for (int c = 0; c < FC_COLS; ++c) wv[c] = *reinterpret_cast<const floatx4*>(wr[c] + k);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < FC_ROWS; ++r)
#pragma unroll
                for (int c = 0; c < FC_COLS; ++c) acc[r][c] = __builtin_fmaf(xv[r][e], wv[c][e], acc[r][c]);
    }
    float mine = 0.f;                                     // lane r * FC_COLS + c stores output (r, c)
#pragma unroll
    for (int r = 0; r < FC_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < FC_COLS; ++c) {
            float v = acc[r][c];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
            if (lane == r * FC_COLS + c) mine = v;
        }
    const int m = m0 + lane / FC_COLS, n = n0 + lane % FC_COLS;
    if (lane < FC_ROWS * FC_COLS && m < M && n < N) y[(size_t)m * y_stride + n] = mine + bias[n];
}

// Second half of a convolution that was split over K (the 7x7-map layers with long K chains: at M = 49 x crops there
// are fewer output tiles than compute units, and one wave per SIMD cannot hide its own load latency): the slices' partial
// sums are added in slice order, then bias and ReLU -- a fixed order for every batch size and tiling, so the rule "which
// layers are split" (layer geometry only) keeps the features independent of how crops are batched.
// Workgroup (blockIdx.x, blockIdx.y) = 4 rows x 64 channel quads, one wave per row: no division, and 32-bit element offsets (the
// launch checks M * Cout and M * Cs_out against 2^31).
__global__ __launch_bounds__(256) void splitk_combine_kernel(const float* __restrict__ part, int ksplit, size_t slice_stride, int M, int Cout,
                                                             const float* __restrict__ bias, int relu, float* __restrict__ out, int Cs_out) {
    const unsigned m = blockIdx.x * 4u + (threadIdx.x >> 6), n = (blockIdx.y * 64u + (threadIdx.x & 63u)) * 4u;
    if (m >= (unsigned)M || n >= (unsigned)Cout) return;
    const unsigned at = m * (unsigned)Cout + n;
    floatx4 v = *reinterpret_cast<const floatx4*>(part + at);
    for (int q = 1; q < ksplit; ++q) {
        part += slice_stride;
        v += *reinterpret_cast<const floatx4*>(part + at);
    }
    v += *reinterpret_cast<const floatx4*>(bias + n);
    if (relu) {
        v[0] = fmaxf(v[0], 0.f);
        v[1] = fmaxf(v[1], 0.f);
        v[2] = fmaxf(v[2], 0.f);
        v[3] = fmaxf(v[3], 0.f);
    }
    *reinterpret_cast<floatx4*>(out + (m * (unsigned)Cs_out + n)) = v;
}

// global average pool + segment consensus in one pass: a snippet's global_pool value is formed exactly
// like gavgpool_kernel does (sequential fp32 sum over h, w, then / (H*W)) and stored as the per-snippet blob
// (calcSig_wOF.py:95,112); the T values of a clip meet in LDS and are summed in fp64 in numpy's axis-0 order
// (calcSig_wOF.py:82) -- the same bits as the two separate kernels.  Clips of up to kMaxFusedT snippets.
__global__ void gavgpool_consensus_kernel(const float* __restrict__ in, float* __restrict__ out, double* __restrict__ feat, int T,
                                          int HW, int Cs_in, int coff_in, int C, int Cs_out, int coff_out) {
    // block = 64 channels x T snippets of clip blockIdx.y; thread (c, t) pools snippet t, thread (c, 0) forms the consensus
    __shared__ float pooled[kMaxFusedT][64];
    const int c = blockIdx.x * 64 + threadIdx.x, t = threadIdx.y, b = blockIdx.y;
    float v = 0.f;
    if (c < C) {
        const int img = b * T + t;
        const float* p = in + (size_t)img * HW * Cs_in + coff_in + c;
        // the sum keeps Caffe's order (h, then w: one sequential fp32 chain); the LOADS of seven pixels are issued together
        float acc = 0.f;
        int q = 0;
        for (; q + 7 <= HW; q += 7) {
            float x[7];
#pragma unroll
            for (int u = 0; u < 7; ++u) x[u] = p[(size_t)(q + u) * Cs_in];
#pragma unroll
            for (int u = 0; u < 7; ++u) acc += x[u];
        }
        for (; q < HW; ++q) acc += p[(size_t)q * Cs_in];
        v = acc / (float)HW;
        out[(size_t)img * Cs_out + coff_out + c] = v;
    }
    pooled[t][threadIdx.x] = v;
    __syncthreads();
    if (t == 0 && c < C) {
        double cons = (double)pooled[0][threadIdx.x];
        for (int s = 1; s < T; ++s) cons = cons + (double)pooled[s][threadIdx.x];
        feat[(size_t)b * C + c] = cons / (double)T;
    }
}

// segment consensus (calcSig_wOF.py:82): fp64 mean over the T snippets of a clip, sequential like numpy's
// axis-0 reduction of the (T, 1, D) float64 array
__global__ void consensus_kernel(const float* __restrict__ per_snippet, double* __restrict__ feat, int B, int T, int D, int Cs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int d = i % D, b = i / D;
    double acc = (double)per_snippet[(size_t)(b * T) * Cs + d];
    for (int t = 1; t < T; ++t) acc = acc + (double)per_snippet[(size_t)(b * T + t) * Cs + d];
    feat[i] = acc / (double)T;
}

// ------------------------------------------------------------------------------------------------
// host launches
// ------------------------------------------------------------------------------------------------
int vq::launch_preprocess(const uint8_t* src, float* dst, int n, const vq_input_desc& in, const vq_tensor_desc& t0, const float* mean,
                          hipStream_t stream) {
    if (in.s2d_pad < 0) {
        const int64_t nchunk = (int64_t)n * in.h * in.w * (t0.c / 4);
        preprocess_kernel<<<cdiv(nchunk, 256), 256, 0, stream>>>(src, dst, nchunk, in.c, t0.c, mean);
    } else {
        const int64_t nchunk = (int64_t)n * t0.h * t0.w * in.c;
        if (in.c == 3 && t0.c == 12)
            preprocess_s2d3_kernel<<<cdiv(nchunk / 3, 256), 256, 0, stream>>>(src, dst, nchunk / 3, in.h, in.w, t0.h, t0.w, in.s2d_pad, mean, in.s2d_order);
        else
            preprocess_s2d_kernel<<<cdiv(nchunk, 256), 256, 0, stream>>>(src, dst, nchunk, in.h, in.w, in.c, t0.h, t0.w, in.s2d_pad, mean, in.s2d_order);
    }
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_pool(const PoolArgs& a, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int64_t blocks = (a.total + 255) / 256;
    if (a.mode)
        VQ_LAUNCH(pool_fast_kernel, (unsigned)((a.total + kPoolPerWG - 1) / kPoolPerWG), 256, 0, stream, ev_start, ev_stop, a);
    else if (a.is_max)
        VQ_LAUNCH(pool_kernel<true>, (unsigned)blocks, 256, 0, stream, ev_start, ev_stop, a);
    else
        VQ_LAUNCH(pool_kernel<false>, (unsigned)blocks, 256, 0, stream, ev_start, ev_stop, a);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_gavgpool(const float* in, float* out, int n, int HW, int Cs_in, int coff_in, int C, int Cs_out, int coff_out, hipStream_t stream,
                        hipEvent_t ev_start, hipEvent_t ev_stop) {
    VQ_LAUNCH(gavgpool_kernel, cdiv((int64_t)n * C, 256), 256, 0, stream, ev_start, ev_stop, in, out, n, HW, Cs_in, coff_in, C, Cs_out, coff_out);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_gavgpool_consensus(const float* in, float* out, double* feat, int B, int T, int HW, int Cs_in, int coff_in, int C, int Cs_out,
                                  int coff_out, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    VQ_LAUNCH(gavgpool_consensus_kernel, dim3(cdiv(C, 64), B), dim3(64, T), 0, stream, ev_start, ev_stop, in, out, feat, T, HW, Cs_in, coff_in, C,
              Cs_out, coff_out);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_inner_product(const float* x, int x_stride, const float* W, const float* bias, float* y, int y_stride, int M, int K, int N,
                             hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    VQ_LAUNCH(inner_product_kernel, dim3(cdiv(M, FC_ROWS), cdiv(N, FC_COLS)), 64, 0, stream, ev_start, ev_stop, x, x_stride, W, bias, y, y_stride, M,
              K, N);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_splitk_combine(const float* part, int ksplit, size_t slice_stride, int M, int Cout, const float* bias, int relu, float* out,
                              int Cs_out, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    VQ_LAUNCH(splitk_combine_kernel, dim3((unsigned)cdiv(M, 4), (unsigned)cdiv(Cout / 4, 64)), 256, 0, stream, ev_start, ev_stop, part, ksplit,
              slice_stride, M, Cout, bias, relu, out, Cs_out);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}

int vq::launch_consensus(const float* per_snippet, double* feat, int B, int T, int D, int Cs, hipStream_t stream) {
    consensus_kernel<<<cdiv((int64_t)B * D, 256), 256, 0, stream>>>(per_snippet, feat, B, T, D, Cs);
    VQ_CHECK_LAUNCH();
    return VQ_OK;
}
