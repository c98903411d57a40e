// Shared host-side helpers of libvqamd (error plumbing, HIP call checking).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "vq_amd.h"
#include "host/vq_host.h"      // cdiv, the error string shared with the host-only translation units

namespace vq {

inline int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}

#define VQ_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return ::vq::fail(e_ == hipErrorOutOfMemory ? VQ_E_NOMEM : VQ_E_HIP, "%s failed: %s (%s:%d)", #call, \
                              hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

#define VQ_CHECK_LAUNCH()                                                                         \
    do {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess)                                                                     \
            return ::vq::fail(VQ_E_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define VQ_REQUIRE(cond, ...)                                  \
    do {                                                       \
        if (!(cond)) return ::vq::fail(VQ_E_INVALID, __VA_ARGS__); \
    } while (0)

// RAII: make `device` current for the duration of an API call.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (kernel, DEVICE) pair, and one process may hold handles on several
// GPUs (vq_db_create / vq_tsn_create take a device): remember per device where it has been raised.  Use inside a function that
// returns int, with the handle's device current.
struct PerDeviceOnce {
    std::mutex mu;
    unsigned long long done = 0;          // bit d: set on device d
    bool need(int device) {
        std::lock_guard<std::mutex> lk(mu);
        return device < 0 || device >= 64 || !((done >> device) & 1ull);
    }
    void mark(int device) {
        std::lock_guard<std::mutex> lk(mu);
        if (device >= 0 && device < 64) done |= 1ull << device;
    }
};
#define VQ_DYN_LDS(kern, bytes)                                                                                                  \
    do {                                                                                                                         \
        static ::vq::PerDeviceOnce once_;                                                                                        \
        int dev_ = -1;                                                                                                           \
        (void)hipGetDevice(&dev_);                                                                                               \
        if (once_.need(dev_)) {                                                                                                  \
            VQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            once_.mark(dev_);                                                                                                    \
        }                                                                                                                        \
    } while (0)


// A stored feature value as the fp64 the arithmetic runs in.  binary16 -> binary32 -> binary64 is exact, so an fp16 database (VQ_F16)
// computes what an fp32 or fp64 database holding the same values computes.
__device__ __forceinline__ double widen(double x) { return x; }
__device__ __forceinline__ double widen(float x) { return (double)x; }
__device__ __forceinline__ double widen(__half x) { return (double)__half2float(x); }
// binary16 -> binary64 is exact (through binary32, subnormals included): an fp16 database scores like the fp64 arithmetic on its values
__device__ __forceinline__ double half_to_double(_Float16 h) { return (double)(float)h; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The one-query scan reads the database once, whole 1 KB per wave instruction, and it is far larger than every cache: its loads
// carry the non-temporal hint (6.15 ms per pass at cfg 4 instead of 6.8-7.0 on the same box: 6.66 TB/s).
typedef float vq_f4 __attribute__((ext_vector_type(4)));
typedef double vq_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 stream_load4(const float* p) {
    const vq_f4 r = __builtin_nontemporal_load(reinterpret_cast<const vq_f4*>(p));
    return make_float4(r.x, r.y, r.z, r.w);
}

// csrc/vq_boot.hip: closed-form target bootstrapping on rows that already live on the device.  row_off [P][stride]
// element offsets into base_dev (the n_valid[p] validated matches first, then the n_invalid[p] non-matches).
int bootstrap_from_device_rows(const void* base_dev, int dtype, const std::vector<int64_t>& row_off, int stride, const int32_t* n_valid,
                               const int32_t* n_invalid, int P, int D, double mu, hipStream_t stream, double* targets_host,
                               double* targets_dev_copy);

// csrc/vq_db.hip: copy the n scores of the last scan to dst_dev on `st`, ORDERED BEHIND that scan (which ran on the handle's
// own stream): an event recorded on the handle's stream, waited for by `st`.  VQ_E_STATE without a scan.  Takes the handle's lock.
int db_copy_scores_ordered(vq_db* db, double* dst_dev, int64_t* n_out, hipStream_t st);

// csrc/vq_tsn.hip (device_pool, vq::PoolBlock): closed extractors leave their big device blocks in a process-wide pool for the next
// extractor of the same shape (VQ_DEVICE_POOL_GB); this gives them back to the driver -- called by the other modules when an allocation of theirs runs out of memory.
void device_pool_trim();

// hipMalloc for everything the library allocates itself: when the device is out of memory the blocks that closed extractors left in
// the pool go back to the driver and the allocation is tried once more (the pool must never be the reason another handle cannot grow).
// Allocations made OUTSIDE the library (torch, the host application) cannot see the pool: VQ_DEVICE_POOL_GB bounds what it may hold.
inline hipError_t malloc_trim(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        device_pool_trim();
        e = hipMalloc(p, bytes);
    }
    return e;
}
template <typename T>
inline hipError_t malloc_trim(T** p, size_t bytes) {
    return malloc_trim(reinterpret_cast<void**>(p), bytes);
}

// Move-only owners of what a handle keeps on a device: device memory, pinned host memory, an event, a stream.  A handle that holds
// them as members needs no free function; it must be destroyed with its device current.  Creation reports the HIP error (use VQ_HIP).
template <typename T, hipError_t (*Release)(T)>
struct Owned {
    T v{};
    Owned() = default;
    Owned(Owned&& o) noexcept : v(o.v) { o.v = T{}; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            v = o.v;
            o.v = T{};
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (v) (void)Release(v);
        v = T{};
    }
    operator T() const { return v; }
    explicit operator bool() const { return v != T{}; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return reset(), hipEventCreateWithFlags(&v, flags); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags = hipStreamDefault) { return reset(), hipStreamCreateWithFlags(&v, flags); }
};
template <typename T>
struct PinnedMem : Owned<void*, hipHostFree> {
    hipError_t alloc(size_t count) { return reset(), hipHostMalloc(&v, count * sizeof(T)); }
    T* get() const { return static_cast<T*>(v); }
    operator T*() const { return get(); }
};
template <typename T>
struct DeviceMem : Owned<void*, hipFree> {
    size_t bytes = 0;
    DeviceMem() = default;
    DeviceMem(DeviceMem&& o) noexcept : Owned(std::move(o)), bytes(o.bytes) { o.bytes = 0; }
    DeviceMem& operator=(DeviceMem&& o) noexcept {
        if (this != &o) {
            Owned::operator=(std::move(o));
            bytes = o.bytes;
            o.bytes = 0;
        }
        return *this;
    }
    // at least `need` bytes (vq::malloc_trim); never shrinks, and what the block held is gone when it had to grow
    hipError_t grow(size_t need) {
        if (need <= bytes) return hipSuccess;
        reset();
        bytes = 0;
        const hipError_t e = malloc_trim(&v, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    T* get() const { return static_cast<T*>(v); }
    operator T*() const { return get(); }
};

}  // namespace vq
