// Frame ingest on gfx950: decoded frames -> the crops the TSN forward consumes.
//
// What it replaces (paths relative to the reference checkout): the resize + over-sample part of
//   src/features_GPU_compute/calcSig_wOF.py:94,111   CaffeNet.predict_single_frame / predict_single_flow_stack(...,
//                                                    frame_size=(340, 256))  ->  crop 0 (top-left 224 x 224, un-mirrored)
// i.e. per frame: cv2.resize(frame, (340, 256)) (INTER_LINEAR), then the top-left crop.  Only the crop x crop pixels that
// survive are computed.  Two rules (vq_amd.h):
//   VQ_RESIZE_CV2_FIXED (default of every caller)  OpenCV's own uint8 rule: float sample positions, 11-bit fixed-point weights,
//       int32 horizontal pass, fixed-point vertical pass (blend<0> below) -- integer arithmetic, so host
//       (tsn/frames.py:resize_cv2_fixed), device and oracle (oracle/frames_oracle.py) agree bit for bit;
//   VQ_RESIZE_EXACT  the same sampling grid with exact fp64 weights, rounded half to even (tsn/frames.py:resize_exact,
//       operation for operation, contraction off).
// Both restate cv2 from memory of imgproc/resize.cpp: "parity unpinned" for lack of cv2 and of the reference's frames.
//
// VQ_RESIZE_OVERSAMPLE (a flag bit on `rule`, both entry points): all TEN crops of pyActionRecog's over-sample -- what predict_single_frame /
// predict_single_flow_stack feed the classifier head, and what the standard TSN test protocol averages -- from one pass over the frame:
// [n][10][crop][crop][C], crop k < 5 the window of the resized frame at tsn/frames.py:oversample_offsets()[k] (four corners, then the
// centre), crop 5 + k its mirror along x; VQ_RESIZE_MIRROR_INVERT stores 255 - v in the mirrored crops (the x planes of a flow stack; the
// planes form does it for its even channels itself).  Order and x-inversion restated from memory: parity unpinned.
//
// ONE path: the value of a pixel of the resized frame is written once (axis_tap / blend, per MODE -- 0: cv2 fixed point, 1: exact fp64
// weights, 2: the frame has the size already and the crop is a copy under either rule) and evaluated at window offset + position in the
// crop by two kernel templates: crop_packed_kernel (a thread owns one pixel, all packed channels) and crop_planes_kernel (a thread owns two
// pixels of all C planes, whole-word stores).  TEN is a template parameter of both: the un-flagged call is the instantiation with window
// (0, 0) and one store; the flagged one decodes the window from the thread index and stores the pixel and its mirror, so a mirror pair is
// equal and crop 0 has the bytes of the un-flagged call by construction.
#include "vq_common.h"

using namespace vq;

namespace {

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

struct AxisTap {
    int i0, i1;        // the two source rows / columns
    int w0, w1;        // MODE 0: their 11-bit weights
    double f;          // MODE 1: the weight of i1
};

// The taps of coordinate d of the resized frame along one axis
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
        // frames.py: ys = clip((arange(h) + 0.5) * ih / h - 0.5, 0, ih - 1)
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
        // a[y0][:, x0] * (1 - wy) * (1 - wx) + a[y0][:, x1] * (1 - wy) * wx + a[y1][:, x0] * wy * (1 - wx) + a[y1][:, x1] * wy * wx
        const double wy = ty.f, wx = tx.f;
        double v = (double)p00 * (1.0 - wy) * (1.0 - wx);
        v = v + (double)p01 * (1.0 - wy) * wx;
        v = v + (double)p10 * wy * (1.0 - wx);
        v = v + (double)p11 * wy * wx;
        return (int)fmin(fmax(rint(v), 0.0), 255.0);      // np.clip(np.rint(out), 0, 255)
    }
    return p00;
}

// Where the four taps of a pixel lie in a row-major grey plane (step 1) or in packed pixels (step = their channels), w pixels a row
struct TapOffsets {
    int64_t o00, o01, o10, o11;
};

__device__ inline TapOffsets tap_offsets(int w, int step, const AxisTap& ty, const AxisTap& tx) {
    return {((int64_t)ty.i0 * w + tx.i0) * step, ((int64_t)ty.i0 * w + tx.i1) * step, ((int64_t)ty.i1 * w + tx.i0) * step,
            ((int64_t)ty.i1 * w + tx.i1) * step};
}

// One value of the resized frame; ch: the channel of packed pixels (the index is loop-invariant + ch: one add per tap and channel)
template <int MODE>
__device__ inline int sample(const uint8_t* p, const TapOffsets& o, int ch, const AxisTap& ty, const AxisTap& tx) {
    if (MODE == 2) return p[o.o00 + ch];
    return blend<MODE>(p[o.o00 + ch], p[o.o01 + ch], p[o.o10 + ch], p[o.o11 + ch], ty, tx);
}

struct CropArgs {
    const uint8_t* src;   // packed: [n][h][w][c]; planes: plane p of frame n at src + p * plane_stride + n * h * w
    uint8_t* dst;         // [n][1 or 10 crops][crop][crop][dst_c], the packed form's channels at dst_c0
    int64_t plane_stride, total;   // total: threads = n * (1 or 5 windows) * crop * crop (packed), half of that (planes)
    int h, w, c, rw, rh, crop, dst_c, dst_c0, invert;
};

// Window k of the over-sample in the resized frame: tsn/frames.py:oversample_offsets, the four corners (0,0) (0,fx) (fy,0) (fy,fx), then
// the centre (integer division = its trunc(H / 2.0 - c / 2.0) for H >= c)
__device__ inline void window_offset(const CropArgs& a, int k, int& oy, int& ox) {
    const int fy = a.rh - a.crop, fx = a.rw - a.crop;
    oy = k == 4 ? fy / 2 : (k & 2) ? fy : 0;
    ox = k == 4 ? fx / 2 : (k & 1) ? fx : 0;
}

// A thread owns one pixel and its c packed channels.  TEN: of one of the five windows, stored to crop k and, mirrored along x, to crop
// 5 + k -- a wave's 64 threads are 64 neighbouring columns of one row of one window: its stores to crop k are contiguous, and those to
// crop 5 + k the same bytes of that crop's row walked backwards.
template <int MODE, bool TEN>
__global__ void crop_packed_kernel(CropArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int64_t area = (int64_t)a.crop * a.crop;
    const int x = (int)(i % a.crop), y = (int)((i / a.crop) % a.crop);
    const int k = TEN ? (int)((i / area) % 5) : 0;
    const int64_t n = i / ((TEN ? 5 : 1) * area);
    int oy = 0, ox = 0;
    if constexpr (TEN) window_offset(a, k, oy, ox);
    const AxisTap ty = axis_tap<MODE>(oy + y, a.h, a.rh, false), tx = axis_tap<MODE>(ox + x, a.w, a.rw, true);
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w * a.c;
    const TapOffsets o = tap_offsets(a.w, a.c, ty, tx);
    const int64_t crop_row = (n * (TEN ? 10 : 1) + k) * a.crop + y;
    uint8_t* out = a.dst + (crop_row * a.crop + x) * a.dst_c + a.dst_c0;
    // the same pixel of crop 5 + k, mirrored along x (TEN only)
    uint8_t* mir = a.dst + ((crop_row + 5 * a.crop) * a.crop + (a.crop - 1 - x)) * a.dst_c + a.dst_c0;
    for (int ch = 0; ch < a.c; ++ch) {
        const int v = sample<MODE>(img, o, ch, ty, tx);
        out[ch] = (uint8_t)v;
        if constexpr (TEN) mir[ch] = (uint8_t)(a.invert ? 255 - v : v);
    }
}

// All C grey planes of a snippet stack in ONE launch (the flow net's ten): a thread owns two horizontally adjacent output pixels, computes
// their taps once (y per thread, x per pixel), reads them from every plane and writes its 2 C bytes as whole 32-bit words of the interleaved
// crop.  The packed form costs a launch per plane -- ten passes whose byte stores are C bytes apart (0.53 ms each for 800 crops: 5.3 ms of
// the GPU per command-line batch, beside the networks).  TEN: the mirror of the pair is the pixel pair at column crop - 2 - 2 xp (even,
// since crop is): the same 2 C bytes with the two pixels swapped and the even channels (the x planes) stored as 255 - v -- whole words too.
template <int C, int MODE, bool TEN>
__global__ void crop_planes_kernel(CropArgs a) {
    static_assert((2 * C) % 4 == 0, "a thread's two pixels are whole 32-bit words");
    constexpr int WORDS = 2 * C / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int half = a.crop / 2;
    const int64_t area = (int64_t)half * a.crop;
    const int xp = (int)(i % half), y = (int)((i / half) % a.crop);
    const int k = TEN ? (int)((i / area) % 5) : 0;
    const int64_t n = i / ((TEN ? 5 : 1) * area);
    int oy = 0, ox = 0;
    if constexpr (TEN) window_offset(a, k, oy, ox);
    const uint8_t* img = a.src + n * (int64_t)a.h * a.w;
    uint32_t words[WORDS], mwords[WORDS];
#pragma unroll
    for (int q = 0; q < WORDS; ++q) words[q] = mwords[q] = 0u;
    const AxisTap ty = axis_tap<MODE>(oy + y, a.h, a.rh, false);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const AxisTap tx = axis_tap<MODE>(ox + 2 * xp + e, a.w, a.rw, true);
        const TapOffsets o = tap_offsets(a.w, 1, ty, tx);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const int v = sample<MODE>(img + ch * a.plane_stride, o, 0, ty, tx);
            const int pos = e * C + ch, mpos = (1 - e) * C + ch;
            words[pos >> 2] |= (uint32_t)v << (8 * (pos & 3));
            if constexpr (TEN) mwords[mpos >> 2] |= (uint32_t)(ch % 2 == 0 ? 255 - v : v) << (8 * (mpos & 3));
        }
    }
    const int64_t crop_row = (n * (TEN ? 10 : 1) + k) * a.crop + y;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.dst + (crop_row * a.crop + 2 * xp) * C);
    uint32_t* mir = reinterpret_cast<uint32_t*>(a.dst + ((crop_row + 5 * a.crop) * a.crop + (a.crop - 2 - 2 * xp)) * C);
#pragma unroll
    for (int q = 0; q < WORDS; ++q) {
        out[q] = words[q];
        if constexpr (TEN) mir[q] = mwords[q];
    }
}

// rule = resize rule in the low byte | flag bits
bool rule_known(int32_t rule, int32_t flags_allowed) {
    const int32_t base = rule & 0xff, flags = rule & ~0xff;
    if (base != VQ_RESIZE_CV2_FIXED && base != VQ_RESIZE_EXACT) return false;
    if (flags & ~flags_allowed) return false;
    return !(flags & VQ_RESIZE_MIRROR_INVERT) || (flags & VQ_RESIZE_OVERSAMPLE);
}

using CropKernel = void (*)(CropArgs);
const CropKernel PACKED[2][3] = {{crop_packed_kernel<0, false>, crop_packed_kernel<1, false>, crop_packed_kernel<2, false>},
                                 {crop_packed_kernel<0, true>, crop_packed_kernel<1, true>, crop_packed_kernel<2, true>}};
const CropKernel PLANES10[2][3] = {{crop_planes_kernel<10, 0, false>, crop_planes_kernel<10, 1, false>, crop_planes_kernel<10, 2, false>},
                                   {crop_planes_kernel<10, 0, true>, crop_planes_kernel<10, 1, true>, crop_planes_kernel<10, 2, true>}};

// The launch of either form (form[TEN][MODE]; a thread owns `pixels` pixels of a row) on `a` with src, dst, plane_stride, the geometry
// and the destination channels filled in: a frame that already has the size is copied by either rule (weights 1, 0)
int launch_crops(const CropKernel (&form)[2][3], int pixels, CropArgs a, int32_t n, int32_t rule, hipStream_t st) {
    const bool ten = (rule & VQ_RESIZE_OVERSAMPLE) != 0;
    const int mode = a.h == a.rh && a.w == a.rw ? 2 : (rule & 0xff) == VQ_RESIZE_CV2_FIXED ? 0 : 1;
    a.total = (int64_t)n * (ten ? 5 : 1) * a.crop * (a.crop / pixels);
    a.invert = (rule & VQ_RESIZE_MIRROR_INVERT) ? 1 : 0;
    form[ten][mode]<<<(unsigned)cdiv(a.total, 256), 256, 0, st>>>(a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(VQ_E_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    return VQ_OK;
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
    CropArgs a{};
    a.src = planes_dev, a.dst = crops_dev, a.plane_stride = plane_stride;
    a.h = h, a.w = w, a.c = c, a.rw = resize_w, a.rh = resize_h, a.crop = crop, a.dst_c = c, a.dst_c0 = 0;
    return launch_crops(PLANES10, 2, a, n, rule, (hipStream_t)stream);
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
    CropArgs a{};
    a.src = src, a.dst = crops_dev, a.plane_stride = 0;
    a.h = h, a.w = w, a.c = c, a.rw = resize_w, a.rh = resize_h, a.crop = crop, a.dst_c = dst_channels, a.dst_c0 = dst_channel0;
    const int rc = launch_crops(PACKED, 1, a, n, rule, st);
    if (staged) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(staged);
    }
    return rc;
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
