// Frame ingest on gfx950: decoded frames -> the crops the TSN forward consumes.
//
// What it replaces (paths relative to the reference checkout): the resize + over-sample part of
//   src/features_GPU_compute/calcSig_wOF.py:94,111   CaffeNet.predict_single_frame / predict_single_flow_stack(...,
//                                                    frame_size=(340, 256))  ->  crop 0 (top-left 224 x 224, un-mirrored)
// i.e. per frame: cv2.resize(frame, (340, 256)) (INTER_LINEAR), then the top-left crop.  Only the crop x crop pixels that
// survive are computed.  Two rules (vq_amd.h):
//   VQ_RESIZE_CV2_FIXED (default of every caller)  OpenCV's own uint8 rule: float sample positions, 11-bit fixed-point weights,
//       int32 horizontal pass, ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2 vertical pass -- integer
//       arithmetic, so host (tsn/frames.py:resize_cv2_fixed), device and oracle (oracle/frames_oracle.py) agree bit for bit;
//   VQ_RESIZE_EXACT  the same sampling grid with exact fp64 weights, rounded half to even (tsn/frames.py:resize_exact,
//       operation for operation, contraction off).
// Both restate cv2 from memory of imgproc/resize.cpp: "parity unpinned" for lack of cv2 and of the reference's frames.
//
// VQ_RESIZE_OVERSAMPLE (a flag bit on `rule`, both entry points): all TEN crops of pyActionRecog's over-sample -- what predict_single_frame /
// predict_single_flow_stack feed the classifier head, and what the standard TSN test protocol averages -- from one pass over the frame:
// [n][10][crop][crop][C], crop k < 5 the window of the resized frame at tsn/frames.py:oversample_offsets()[k] (four corners, then the
// centre), crop 5 + k its mirror along x; VQ_RESIZE_MIRROR_INVERT stores 255 - v in the mirrored crops (the x planes of a flow stack; the
// planes form does it for its even channels itself).  A thread computes a pixel of one of the five windows ONCE and stores it twice, so a
// mirror pair is equal by construction; crop 0 has the bytes of the un-flagged call, whose kernels below are untouched.  Order and
// x-inversion restated from memory: parity unpinned.
#include "vq_common.h"

using namespace vq;

namespace {

struct ResizeArgs {
    const uint8_t* src;   // [n][h][w][c]
    uint8_t* dst;         // [n][crop][crop][dst_c], this plane at channel dst_c0
    int64_t total;        // n * crop * crop
    int h, w, c, rw, rh, crop, dst_c, dst_c0;
};

// cv::resize INTER_LINEAR, 8-bit: tap position and weights of output coordinate d (frames.py:_cv2_linear_taps)
__device__ inline void cv2_taps(int d, int n_in, int n_out, bool clamp_taps, int& s, int& w0, int& w1) {
    const double scale = 1.0 / ((double)n_out / (double)n_in);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (clamp_taps) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_in - 1) { f = 0.f; s = n_in - 1; }
    }
    w0 = (int)rintf((1.f - f) * 2048.f);          // cvRound: round half to even
    w1 = (int)rintf(f * 2048.f);
}

__global__ void resize_crop_cv2_kernel(ResizeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int x = (int)(i % a.crop), y = (int)((i / a.crop) % a.crop);
    const int64_t n = i / ((int64_t)a.crop * a.crop);
    int sx, a0, a1, sy, b0, b1;
    cv2_taps(x, a.w, a.rw, true, sx, a0, a1);
    cv2_taps(y, a.h, a.rh, false, sy, b0, b1);      // along y the weights stay, the ROWS are clipped
    const int x1 = min(sx + 1, a.w - 1);
    const int y0 = min(max(sy, 0), a.h - 1), y1 = min(max(sy + 1, 0), a.h - 1);
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w * a.c;
    uint8_t* out = a.dst + (n * a.crop * a.crop + (int64_t)y * a.crop + x) * a.dst_c + a.dst_c0;
    for (int ch = 0; ch < a.c; ++ch) {
        const int p00 = img[((int64_t)y0 * a.w + sx) * a.c + ch], p01 = img[((int64_t)y0 * a.w + x1) * a.c + ch];
        const int p10 = img[((int64_t)y1 * a.w + sx) * a.c + ch], p11 = img[((int64_t)y1 * a.w + x1) * a.c + ch];
        const int s0 = p00 * a0 + p01 * a1, s1 = p10 * a0 + p11 * a1;
        const int v = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;
        out[ch] = (uint8_t)min(max(v, 0), 255);
    }
}

__global__ void resize_crop_kernel(ResizeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int x = (int)(i % a.crop), y = (int)((i / a.crop) % a.crop);
    const int64_t n = i / ((int64_t)a.crop * a.crop);
    // frames.py: ys = clip((arange(h) + 0.5) * ih / h - 0.5, 0, ih - 1)
    double ys = ((double)y + 0.5) * (double)a.h / (double)a.rh - 0.5;
    double xs = ((double)x + 0.5) * (double)a.w / (double)a.rw - 0.5;
    ys = fmin(fmax(ys, 0.0), (double)(a.h - 1));
    xs = fmin(fmax(xs, 0.0), (double)(a.w - 1));
    const int y0 = (int)floor(ys), x0 = (int)floor(xs);
    const int y1 = min(y0 + 1, a.h - 1), x1 = min(x0 + 1, a.w - 1);
    const double wy = ys - (double)y0, wx = xs - (double)x0;
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w * a.c;
    uint8_t* out = a.dst + (n * a.crop * a.crop + (int64_t)y * a.crop + x) * a.dst_c + a.dst_c0;
    for (int ch = 0; ch < a.c; ++ch) {
        const double a00 = img[((int64_t)y0 * a.w + x0) * a.c + ch], a01 = img[((int64_t)y0 * a.w + x1) * a.c + ch];
        const double a10 = img[((int64_t)y1 * a.w + x0) * a.c + ch], a11 = img[((int64_t)y1 * a.w + x1) * a.c + ch];
        // a[y0][:, x0] * (1 - wy) * (1 - wx) + a[y0][:, x1] * (1 - wy) * wx + a[y1][:, x0] * wy * (1 - wx) + a[y1][:, x1] * wy * wx
        double v = a00 * (1.0 - wy) * (1.0 - wx);
        v = v + a01 * (1.0 - wy) * wx;
        v = v + a10 * wy * (1.0 - wx);
        v = v + a11 * wy * wx;
        v = fmin(fmax(rint(v), 0.0), 255.0);      // np.clip(np.rint(out), 0, 255)
        out[ch] = (uint8_t)v;
    }
}

// A frame that already has the size: the crop is a copy under either rule (weights 1 and 0)
__global__ void crop_copy_kernel(ResizeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int x = (int)(i % a.crop), y = (int)((i / a.crop) % a.crop);
    const int64_t n = i / ((int64_t)a.crop * a.crop);
    const uint8_t* px = a.src + ((n * a.h + y) * (int64_t)a.w + x) * a.c;
    uint8_t* out = a.dst + (n * a.crop * a.crop + (int64_t)y * a.crop + x) * a.dst_c + a.dst_c0;
    for (int ch = 0; ch < a.c; ++ch) out[ch] = px[ch];
}

// All C grey planes of a snippet stack in ONE launch (the flow net's ten): a thread owns two horizontally adjacent output pixels, computes
// their taps once, reads them from every plane and writes its 2 C bytes as whole 32-bit words of the interleaved crop.  The per-plane
// form above costs a launch per plane -- ten passes whose byte stores are C bytes apart (0.53 ms each for 800 crops: 5.3 ms of the GPU per
// command-line batch, beside the networks) -- and frames that already have the size went through the fp64 rule as a copy.
// MODE 0: the cv2 fixed-point rule, 1: exact fp64 weights, 2: the frame has the size already (the crop is a copy: weights 1, 0 under either rule).
struct PlanesArgs {
    const uint8_t* src;   // plane p of frame n at src + p * plane_stride + n * h * w
    uint8_t* dst;         // [n][crop][crop][C]
    int64_t plane_stride, total;   // total = n * crop * crop / 2
    int h, w, rw, rh, crop;
};

template <int C, int MODE>
__global__ void resize_crop_planes_kernel(PlanesArgs a) {
    static_assert((2 * C) % 4 == 0, "a thread's two pixels are whole 32-bit words");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int half = a.crop / 2;
    const int xp = (int)(i % half), y = (int)((i / half) % a.crop);
    const int64_t n = i / ((int64_t)half * a.crop);
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w;
    uint32_t words[2 * C / 4];
#pragma unroll
    for (int q = 0; q < 2 * C / 4; ++q) words[q] = 0u;
    int sy = y, b0 = 0, b1 = 0, y0 = y, y1 = y;
    double wy = 0.0;
    if (MODE == 0) {
        cv2_taps(y, a.h, a.rh, false, sy, b0, b1);
        y0 = min(max(sy, 0), a.h - 1);
        y1 = min(max(sy + 1, 0), a.h - 1);
    } else if (MODE == 1) {
        double ys = ((double)y + 0.5) * (double)a.h / (double)a.rh - 0.5;
        ys = fmin(fmax(ys, 0.0), (double)(a.h - 1));
        y0 = (int)floor(ys);
        y1 = min(y0 + 1, a.h - 1);
        wy = ys - (double)y0;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int x = 2 * xp + e;
        int x0 = x, x1 = x, a0 = 0, a1 = 0;
        double wx = 0.0;
        if (MODE == 0) {
            cv2_taps(x, a.w, a.rw, true, x0, a0, a1);
            x1 = min(x0 + 1, a.w - 1);
        } else if (MODE == 1) {
            double xs = ((double)x + 0.5) * (double)a.w / (double)a.rw - 0.5;
            xs = fmin(fmax(xs, 0.0), (double)(a.w - 1));
            x0 = (int)floor(xs);
            x1 = min(x0 + 1, a.w - 1);
            wx = xs - (double)x0;
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const uint8_t* pl = img + ch * a.plane_stride;
            int v;
            if (MODE == 2) {
                v = pl[(int64_t)y * a.w + x];
            } else if (MODE == 0) {
                const int p00 = pl[(int64_t)y0 * a.w + x0], p01 = pl[(int64_t)y0 * a.w + x1];
                const int p10 = pl[(int64_t)y1 * a.w + x0], p11 = pl[(int64_t)y1 * a.w + x1];
                const int s0 = p00 * a0 + p01 * a1, s1 = p10 * a0 + p11 * a1;
                v = min(max((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2, 0), 255);
            } else {
                const double a00 = pl[(int64_t)y0 * a.w + x0], a01 = pl[(int64_t)y0 * a.w + x1];
                const double a10 = pl[(int64_t)y1 * a.w + x0], a11 = pl[(int64_t)y1 * a.w + x1];
                double t = a00 * (1.0 - wy) * (1.0 - wx);
                t = t + a01 * (1.0 - wy) * wx;
                t = t + a10 * wy * (1.0 - wx);
                t = t + a11 * wy * wx;
                v = (int)fmin(fmax(rint(t), 0.0), 255.0);
            }
            const int pos = e * C + ch;
            words[pos >> 2] |= (uint32_t)v << (8 * (pos & 3));
        }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(a.dst + ((n * a.crop + y) * (int64_t)a.crop + 2 * xp) * C);
#pragma unroll
    for (int q = 0; q < 2 * C / 4; ++q) out[q] = words[q];
}

// ---- the ten-crop over-sample ---------------------------------------------------------------------------------------------------
// The crop-0 kernels above stay as they are; these restate their per-pixel arithmetic once, per MODE (0: cv2 fixed point, 1: exact fp64
// weights, 2: the frame has the size already), evaluated at a coordinate of the RESIZED frame (window offset + position in the crop).
struct AxisTap {
    int i0, i1;        // the two source rows / columns
    int w0, w1;        // MODE 0: their 11-bit weights
    double f;          // MODE 1: the weight of i1
};

template <int MODE>
__device__ inline AxisTap axis_tap(int d, int n_in, int n_out, bool x_axis) {
    AxisTap t;
    t.i0 = t.i1 = d;
    t.w0 = t.w1 = 0;
    t.f = 0.0;
    if (MODE == 0) {
        int s;
        cv2_taps(d, n_in, n_out, x_axis, s, t.w0, t.w1);
        if (x_axis) {                                   // taps clamped by cv2_taps
            t.i0 = s;
            t.i1 = min(s + 1, n_in - 1);
        } else {                                        // the weights stay, the ROWS are clipped
            t.i0 = min(max(s, 0), n_in - 1);
            t.i1 = min(max(s + 1, 0), n_in - 1);
        }
    } else if (MODE == 1) {
        double ds = ((double)d + 0.5) * (double)n_in / (double)n_out - 0.5;
        ds = fmin(fmax(ds, 0.0), (double)(n_in - 1));
        t.i0 = (int)floor(ds);
        t.i1 = min(t.i0 + 1, n_in - 1);
        t.f = ds - (double)t.i0;
    }
    return t;
}

template <int MODE>
__device__ inline int blend(int p00, int p01, int p10, int p11, const AxisTap& ty, const AxisTap& tx) {
    if (MODE == 0) {
        const int s0 = p00 * tx.w0 + p01 * tx.w1, s1 = p10 * tx.w0 + p11 * tx.w1;
        return min(max((((ty.w0 * (s0 >> 4)) >> 16) + ((ty.w1 * (s1 >> 4)) >> 16) + 2) >> 2, 0), 255);
    }
    if (MODE == 1) {
        const double wy = ty.f, wx = tx.f;
        double v = (double)p00 * (1.0 - wy) * (1.0 - wx);
        v = v + (double)p01 * (1.0 - wy) * wx;
        v = v + (double)p10 * wy * (1.0 - wx);
        v = v + (double)p11 * wy * wx;
        return (int)fmin(fmax(rint(v), 0.0), 255.0);
    }
    return p00;
}

struct OversampleArgs {
    const uint8_t* src;   // packed: [n][h][w][c]; planes: plane p of frame n at src + p * plane_stride + n * h * w
    uint8_t* dst;         // [n][10][crop][crop][dst_c], the packed form's channels at dst_c0
    int64_t plane_stride, total;   // total: n * 5 * crop * crop (packed), n * 5 * crop * crop / 2 (planes)
    int h, w, c, rw, rh, crop, dst_c, dst_c0, invert;
    int oy[5], ox[5];     // the five windows in the resized frame (host: oversample_windows)
};

// A wave's 64 threads are 64 neighbouring columns of one row of one window: its stores to crop k are contiguous, and those to crop 5 + k
// the same bytes of that crop's row walked backwards.
template <int MODE>
__global__ void oversample_kernel(OversampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int64_t area = (int64_t)a.crop * a.crop;
    const int x = (int)(i % a.crop), y = (int)((i / a.crop) % a.crop), k = (int)((i / area) % 5);
    const int64_t n = i / (5 * area);
    int oy = 0, ox = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (k == q) {
            oy = a.oy[q];
            ox = a.ox[q];
        }
    const AxisTap ty = axis_tap<MODE>(oy + y, a.h, a.rh, false), tx = axis_tap<MODE>(ox + x, a.w, a.rw, true);
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w * a.c;
    const uint8_t* r0 = img + (int64_t)ty.i0 * a.w * a.c;
    const uint8_t* r1 = img + (int64_t)ty.i1 * a.w * a.c;
    uint8_t* out = a.dst + (((n * 10 + k) * a.crop + y) * (int64_t)a.crop + x) * a.dst_c + a.dst_c0;
    uint8_t* mir = a.dst + (((n * 10 + 5 + k) * a.crop + y) * (int64_t)a.crop + (a.crop - 1 - x)) * a.dst_c + a.dst_c0;
    for (int ch = 0; ch < a.c; ++ch) {
        const int v = blend<MODE>(r0[(int64_t)tx.i0 * a.c + ch], r0[(int64_t)tx.i1 * a.c + ch], r1[(int64_t)tx.i0 * a.c + ch],
                                  r1[(int64_t)tx.i1 * a.c + ch], ty, tx);
        out[ch] = (uint8_t)v;
        mir[ch] = (uint8_t)(a.invert ? 255 - v : v);
    }
}

// The C grey planes of a flow stack: a thread owns two adjacent pixels of one of the five windows and all C planes, as resize_crop_planes_kernel
// does for crop 0.  Their mirror is the pixel pair at column crop - 2 - 2 xp (even, since crop is): the same 2 C bytes with the two pixels
// swapped and the even channels (the x planes) stored as 255 - v -- whole 32-bit words at both destinations.
template <int C, int MODE>
__global__ void oversample_planes_kernel(OversampleArgs a) {
    static_assert((2 * C) % 4 == 0, "a thread's two pixels are whole 32-bit words");
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int half = a.crop / 2;
    const int64_t area = (int64_t)half * a.crop;
    const int xp = (int)(i % half), y = (int)((i / half) % a.crop), k = (int)((i / area) % 5);
    const int64_t n = i / (5 * area);
    int oy = 0, ox = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (k == q) {
            oy = a.oy[q];
            ox = a.ox[q];
        }
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w;
    uint32_t words[2 * C / 4], mwords[2 * C / 4];
#pragma unroll
    for (int q = 0; q < 2 * C / 4; ++q) words[q] = mwords[q] = 0u;
    const AxisTap ty = axis_tap<MODE>(oy + y, a.h, a.rh, false);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const AxisTap tx = axis_tap<MODE>(ox + 2 * xp + e, a.w, a.rw, true);
        const int64_t o00 = (int64_t)ty.i0 * a.w + tx.i0, o01 = (int64_t)ty.i0 * a.w + tx.i1;
        const int64_t o10 = (int64_t)ty.i1 * a.w + tx.i0, o11 = (int64_t)ty.i1 * a.w + tx.i1;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const uint8_t* pl = img + ch * a.plane_stride;
            const int v = MODE == 2 ? (int)pl[o00] : blend<MODE>(pl[o00], pl[o01], pl[o10], pl[o11], ty, tx);
            const int pos = e * C + ch, mpos = (1 - e) * C + ch;
            words[pos >> 2] |= (uint32_t)v << (8 * (pos & 3));
            mwords[mpos >> 2] |= (uint32_t)(ch % 2 == 0 ? 255 - v : v) << (8 * (mpos & 3));
        }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(a.dst + (((n * 10 + k) * a.crop + y) * (int64_t)a.crop + 2 * xp) * C);
    uint32_t* mir = reinterpret_cast<uint32_t*>(a.dst + (((n * 10 + 5 + k) * a.crop + y) * (int64_t)a.crop + (a.crop - 2 - 2 * xp)) * C);
#pragma unroll
    for (int q = 0; q < 2 * C / 4; ++q) {
        out[q] = words[q];
        mir[q] = mwords[q];
    }
}

// tsn/frames.py:oversample_offsets: the four corners, then the centre (integer division = its trunc(H / 2.0 - c / 2.0) for H >= c)
void oversample_windows(OversampleArgs& a) {
    const int fy = a.rh - a.crop, fx = a.rw - a.crop;
    const int oy[5] = {0, 0, fy, fy, fy / 2}, ox[5] = {0, fx, 0, fx, fx / 2};
    for (int k = 0; k < 5; ++k) {
        a.oy[k] = oy[k];
        a.ox[k] = ox[k];
    }
}

// rule = resize rule in the low byte | flag bits
bool rule_known(int32_t rule, int32_t flags_allowed) {
    const int32_t base = rule & 0xff, flags = rule & ~0xff;
    if (base != VQ_RESIZE_CV2_FIXED && base != VQ_RESIZE_EXACT) return false;
    if (flags & ~flags_allowed) return false;
    return !(flags & VQ_RESIZE_MIRROR_INVERT) || (flags & VQ_RESIZE_OVERSAMPLE);
}

}  // namespace

extern "C" int vq_resize_crop_planes(const uint8_t* planes_dev, int32_t n, int32_t h, int32_t w, int32_t c, int64_t plane_stride, int32_t resize_w,
                                     int32_t resize_h, int32_t crop, int32_t rule, uint8_t* crops_dev, int32_t device, void* stream) {
    VQ_REQUIRE(planes_dev && crops_dev, "NULL argument");
    VQ_REQUIRE(n > 0 && h > 0 && w > 0, "frames must be [n][h][w] with positive sizes");
    VQ_REQUIRE(c == 10, "the one-launch form is built for the 10 planes of a flow stack (got %d): use vq_resize_crop per plane", c);
    VQ_REQUIRE(plane_stride >= (int64_t)n * h * w, "plane_stride is smaller than a plane");
    VQ_REQUIRE(resize_w >= crop && resize_h >= crop && crop > 0 && crop % 2 == 0, "crop %d must be even and fit the %dx%d resized frame", crop, resize_w,
               resize_h);
    VQ_REQUIRE(rule_known(rule, VQ_RESIZE_OVERSAMPLE), "unknown resize rule %d", rule);
    VQ_REQUIRE(((uintptr_t)crops_dev & 3u) == 0, "crops_dev must be 4-byte aligned");
    int ndev = 0;
    VQ_HIP(hipGetDeviceCount(&ndev));
    VQ_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    if (rule & VQ_RESIZE_OVERSAMPLE) {
        OversampleArgs o;
        o.src = planes_dev;
        o.dst = crops_dev;
        o.plane_stride = plane_stride;
        o.total = (int64_t)n * 5 * crop * (crop / 2);
        o.h = h;
        o.w = w;
        o.c = c;
        o.rw = resize_w;
        o.rh = resize_h;
        o.crop = crop;
        o.dst_c = c;
        o.dst_c0 = 0;
        o.invert = 1;
        oversample_windows(o);
        const unsigned oblocks = (unsigned)cdiv(o.total, 256);
        if (h == resize_h && w == resize_w)
            oversample_planes_kernel<10, 2><<<oblocks, 256, 0, st>>>(o);
        else if ((rule & 0xff) == VQ_RESIZE_CV2_FIXED)
            oversample_planes_kernel<10, 0><<<oblocks, 256, 0, st>>>(o);
        else
            oversample_planes_kernel<10, 1><<<oblocks, 256, 0, st>>>(o);
        const hipError_t oe = hipGetLastError();
        if (oe != hipSuccess) return fail(VQ_E_HIP, "kernel launch failed: %s", hipGetErrorString(oe));
        return VQ_OK;
    }
    PlanesArgs a;
    a.src = planes_dev;
    a.dst = crops_dev;
    a.plane_stride = plane_stride;
    a.total = (int64_t)n * crop * (crop / 2);
    a.h = h;
    a.w = w;
    a.rw = resize_w;
    a.rh = resize_h;
    a.crop = crop;
    const unsigned blocks = (unsigned)cdiv(a.total, 256);
    if (h == resize_h && w == resize_w)
        resize_crop_planes_kernel<10, 2><<<blocks, 256, 0, st>>>(a);
    else if (rule == VQ_RESIZE_CV2_FIXED)
        resize_crop_planes_kernel<10, 0><<<blocks, 256, 0, st>>>(a);
    else
        resize_crop_planes_kernel<10, 1><<<blocks, 256, 0, st>>>(a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(VQ_E_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    return VQ_OK;
}

extern "C" int vq_resize_crop(const uint8_t* frames, int32_t frames_on_device, int32_t n, int32_t h, int32_t w, int32_t c,
                              int32_t resize_w, int32_t resize_h, int32_t crop, int32_t rule, uint8_t* crops_dev, int32_t dst_channels,
                              int32_t dst_channel0, int32_t device, void* stream) {
    VQ_REQUIRE(frames && crops_dev, "NULL argument");
    VQ_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "frames must be [n][h][w][c] with positive sizes");
    VQ_REQUIRE(resize_w >= crop && resize_h >= crop && crop > 0, "crop %d does not fit the %dx%d resized frame", crop, resize_w, resize_h);
    VQ_REQUIRE(rule_known(rule, VQ_RESIZE_OVERSAMPLE | VQ_RESIZE_MIRROR_INVERT), "unknown resize rule %d", rule);
    VQ_REQUIRE(dst_channel0 >= 0 && dst_channel0 + c <= dst_channels, "channels [%d,%d) outside the %d-channel crop buffer", dst_channel0,
               dst_channel0 + c, dst_channels);
    int ndev = 0;
    VQ_HIP(hipGetDeviceCount(&ndev));
    VQ_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = frames;
    uint8_t* staged = nullptr;
    if (!frames_on_device) {
        const size_t bytes = (size_t)n * h * w * c;
        VQ_HIP(vq::malloc_trim((void**)&staged, bytes));
        hipError_t e = hipMemcpyAsync(staged, frames, bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            (void)hipFree(staged);
            return fail(VQ_E_HIP, "hipMemcpyAsync(frames) failed: %s", hipGetErrorString(e));
        }
        src = staged;
    }
    ResizeArgs a;
    a.src = src;
    a.dst = crops_dev;
    a.total = (int64_t)n * crop * crop;
    a.h = h;
    a.w = w;
    a.c = c;
    a.rw = resize_w;
    a.rh = resize_h;
    a.crop = crop;
    a.dst_c = dst_channels;
    a.dst_c0 = dst_channel0;
    if (rule & VQ_RESIZE_OVERSAMPLE) {
        OversampleArgs o;
        o.src = src;
        o.dst = crops_dev;
        o.plane_stride = 0;
        o.total = 5 * a.total;
        o.h = h;
        o.w = w;
        o.c = c;
        o.rw = resize_w;
        o.rh = resize_h;
        o.crop = crop;
        o.dst_c = dst_channels;
        o.dst_c0 = dst_channel0;
        o.invert = (rule & VQ_RESIZE_MIRROR_INVERT) ? 1 : 0;
        oversample_windows(o);
        const unsigned oblocks = (unsigned)cdiv(o.total, 256);
        if (h == resize_h && w == resize_w)
            oversample_kernel<2><<<oblocks, 256, 0, st>>>(o);
        else if ((rule & 0xff) == VQ_RESIZE_CV2_FIXED)
            oversample_kernel<0><<<oblocks, 256, 0, st>>>(o);
        else
            oversample_kernel<1><<<oblocks, 256, 0, st>>>(o);
    } else if (h == resize_h && w == resize_w)  // a frame that already has the size is copied by either rule (weights 1, 0)
        crop_copy_kernel<<<cdiv(a.total, 256), 256, 0, st>>>(a);
    else if (rule == VQ_RESIZE_CV2_FIXED)
        resize_crop_cv2_kernel<<<cdiv(a.total, 256), 256, 0, st>>>(a);
    else
        resize_crop_kernel<<<cdiv(a.total, 256), 256, 0, st>>>(a);
    hipError_t le = hipGetLastError();
    if (staged) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(staged);
    }
    if (le != hipSuccess) return fail(VQ_E_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    return VQ_OK;
}

// ---- device plumbing for a host that has no tensor library loaded ----------------------------------------------------------------
// The single-GPU command line needs four things of a device runtime: a buffer for the crops of a batch, a stream per preparation lane,
// a wait, a read-back.  With these the drop-in `python calcSig_wOF.py ...` runs without importing torch (0.8 s of a 2.3 s process); ranks
// of a multi-GPU run, and anything that holds torch tensors already, keep using torch (tsn/devmem.py decides once per process).
extern "C" int vq_dev_malloc(void** ptr, int64_t bytes, int32_t device) {
    VQ_REQUIRE(ptr && bytes > 0, "bad argument");
    DeviceGuard g(device);
    VQ_HIP(vq::malloc_trim(ptr, (size_t)bytes));
    return VQ_OK;
}

extern "C" int vq_dev_free(void* ptr, int32_t device) {
    if (!ptr) return VQ_OK;
    DeviceGuard g(device);
    VQ_HIP(hipFree(ptr));
    return VQ_OK;
}

extern "C" int vq_stream_create(void** stream, int32_t device) {
    VQ_REQUIRE(stream, "NULL argument");
    DeviceGuard g(device);
    hipStream_t st;
    VQ_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = (void*)st;
    return VQ_OK;
}

extern "C" int vq_stream_create_priority(void** stream, int32_t device, int32_t priority) {
    VQ_REQUIRE(stream, "NULL argument");
    DeviceGuard g(device);
    int least = 0, greatest = 0;                         // numerically: greatest priority <= least priority
    VQ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t st;
    VQ_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority < 0 ? least : (priority > 0 ? greatest : (least + greatest) / 2)));
    *stream = (void*)st;
    return VQ_OK;
}

extern "C" int vq_stream_destroy(void* stream, int32_t device) {
    if (!stream) return VQ_OK;
    DeviceGuard g(device);
    VQ_HIP(hipStreamDestroy((hipStream_t)stream));
    return VQ_OK;
}

extern "C" int vq_stream_synchronize(void* stream, int32_t device) {
    DeviceGuard g(device);
    VQ_HIP(hipStreamSynchronize((hipStream_t)stream));          // NULL: the default stream
    return VQ_OK;
}

extern "C" int vq_dev_read(void* host, const void* dev, int64_t bytes, int32_t device) {
    VQ_REQUIRE(host && dev && bytes > 0, "bad argument");
    DeviceGuard g(device);
    VQ_HIP(hipMemcpy(host, dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return VQ_OK;
}
