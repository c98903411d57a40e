// The handle of a resident feature database: life cycle, upload, layouts, query setters, readers, the one-query round and the row
// views.  The scans are csrc/vq_sim.hip and csrc/vq_sim_batch.hip, the ranking is csrc/vq_rank.hip; what they share: csrc/vq_db.h.
//   src/models/target_clip.py:311-313 _scale_feature     -> scale_query_kernel
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "vq_db.h"
#include "vq_select.h"      // SEL_CHUNK: the blocks of the selection scratch

namespace vq {
std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
}  // namespace vq

using namespace vq;

// The 16-query pass's view of a database: [tile of 16 clips][slice][k / U][clip][U], U elements = 16 bytes (4 floats, 2 doubles, 8 halves:
// csrc/vq_tile_index.h) -- every load instruction of a wave then takes 1 KB of contiguous memory (fp64: four runs of 256 bytes; whole
// 128-byte lines either way: the non-temporal hint pays), where the row-major layout gives it 64 bytes of each of 16 clips 40 KB
// apart.  The two conversions move 16-byte units and do not look inside them, so ONE pair of kernels serves every storage type: du =
// units per vector (D / 4 for fp32, D / 2 for fp64, D / 8 for fp16).  One workgroup per (tile, slice): the 16 rows come in whole (a
// wave reads 1 KB of one clip per instruction), turn in LDS ([16][du + 1] units: 65 792 bytes for fp32, 131 328 for fp64, 33 024 for
// fp16 at D = 1024) and go out in the tiled order.  Rows past n repeat the last clip (the pass never stores them).
__global__ __launch_bounds__(256) void mirror_build_kernel(const vq_f4* feats, vq_f4* mirror, int64_t n, int NV, int du) {
    extern __shared__ __attribute__((aligned(16))) vq_f4 tile_lds[];          // [16][du + 1]
    const int64_t tile = blockIdx.x / NV;
    const int v = (int)(blockIdx.x - tile * NV);
    const int row = du + 1;
    for (int i = threadIdx.x; i < 16 * du; i += 256) {
        const int c = i / du, g = i - c * du;
        const int64_t clip = min(tile * 16 + c, n - 1);
        tile_lds[c * row + g] = __builtin_nontemporal_load(feats + (clip * NV + v) * (int64_t)du + g);
    }
    __syncthreads();
    vq_f4* out = mirror + (tile * NV + v) * 16 * (int64_t)du;
    for (int j = threadIdx.x; j < 16 * du; j += 256) {
        const int g = j >> 4, c = j & 15;
        out[j] = tile_lds[c * row + g];
    }
}

// the inverse of mirror_build_kernel: one workgroup per (tile, slice) of a tiled block -> the 16 row segments (rows past n: none)
__global__ __launch_bounds__(256) void untile_kernel(const vq_f4* tiled, vq_f4* rows, int64_t n, int NV, int du) {
    extern __shared__ __attribute__((aligned(16))) vq_f4 tile_lds[];          // [16][du + 1]
    const int64_t tile = blockIdx.x / NV;
    const int v = (int)(blockIdx.x - tile * NV);
    const int row = du + 1;
    const vq_f4* in = tiled + (tile * NV + v) * 16 * (int64_t)du;
    for (int j = threadIdx.x; j < 16 * du; j += 256) {
        const int g = j >> 4, c = j & 15;
        tile_lds[c * row + g] = in[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * du; i += 256) {
        const int c = i / du, g = i - c * du;
        const int64_t clip = tile * 16 + c;
        if (clip < n) rows[(clip * NV + v) * (int64_t)du + g] = tile_lds[c * row + g];
    }
}

// vq_db_upload into a tiled database: staged row-major rows -> their places in the tiles (16 bytes per thread; d4 = the 16-byte units
// of a vector: D / 4 for fp32, D / 2 for fp64)
__global__ void scatter_rows_tiled_kernel(const float4* staged, float4* tiled, int64_t row0, int64_t nrows, int NV, int d4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_row = (int64_t)NV * d4;
    if (i >= nrows * per_row) return;
    const int64_t r = i / per_row, rem = i - r * per_row;
    const int v = (int)(rem / d4), g = (int)(rem - (int64_t)v * d4);
    const int64_t clip = row0 + r, tile = clip >> 4;
    tiled[((tile * NV + v) * d4 + g) * 16 + (clip & 15)] = staged[i];
}

// upload_unpadded (vq_db_upload on a padded handle): staged vectors of d elements -> vectors at pitch D, the pads d .. D - 1 written as +0.0 (all bits clear in every
// storage type).  U = the unsigned integer of the element's size; one element per thread, a wave's stores are contiguous.
template <typename U>
__global__ void pad_rows_kernel(const U* staged, U* padded, int64_t nvec, int d, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvec * D) return;
    const int64_t v = i / D;
    const int k = (int)(i - v * D);
    padded[i] = k < d ? staged[v * d + k] : (U)0;
}

// target_clip.py:311-313: t = r / (r . r), one block per (s,e) vector of row `row`, fp64 throughout.
// element k of vector (row, v) in the database's layout: feat_index (csrc/vq_tile_index.h), unit = vq_db::unit()
template <typename T>
__global__ __launch_bounds__(256) void scale_query_kernel(const T* feats, int64_t row, int NV, int D, double* t, int unit) {
    __shared__ double part[4];
    const int v = blockIdx.x;
    double p = 0.0;
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        const double x = widen(feats[feat_index(unit, row, NV, v, D, k)]);
        p = fma(x, x, p);
    }
    p = wave_sum(p);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = p;
    __syncthreads();
    const double rr = ((part[0] + part[1]) + part[2]) + part[3];
    for (int k = threadIdx.x; k < D; k += blockDim.x) t[(int64_t)v * D + k] = widen(feats[feat_index(unit, row, NV, v, D, k)]) / rr;
}

// counter-based synthetic rows (shared with oracle/sim_oracle.py::synth_features)
__device__ __forceinline__ uint32_t synth_u24(uint64_t seed_mul, uint64_t idx) {
    uint64_t z = idx + seed_mul;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 40);
}

template <typename T>
__global__ void generate_kernel(T* feats, int64_t total, uint64_t seed_mul, uint64_t idx0, int per_stream /*E*D*/,
                                int S, const float* scales) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t k = i + q;
        if (k >= total) break;
        const int s = (int)((k / per_stream) % S);
        const float u = (float)synth_u24(seed_mul, idx0 + (uint64_t)k) * 5.9604644775390625e-08f;  // 2^-24
        if constexpr (sizeof(T) == 2) {
            // the fp32 value of the other storage types, THEN rounded to nearest even (subnormal halves are kept).  The product is made
            // opaque: left alone the compiler folds multiply and conversion into one v_fma_mixlo_f16, which rounds the exact product once
            float x = u * scales[s];
            asm volatile("" : "+v"(x));
            feats[k] = __float2half_rn(x);
        } else {
            feats[k] = (T)(u * scales[s]);
        }
    }
}

// rows of the database -> a dense [cnt][row_elems] block (vq_db_read_rows: the few validated clips a sharded round sends to the
// rank that solves the bootstrapping problems).  16 bytes per thread.
template <typename U>       // U = uint4: rows of whole 16-byte units; uint2: fp16 rows whose D is no multiple of 8 (8-byte units, rows layout)
__global__ void gather_rows_kernel(const U* feats, const int64_t* rows, int64_t cnt, int64_t row_vec16, U* out, int tiled_nv, int tiled_d4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt * row_vec16) return;
    const int64_t r = i / row_vec16, k = i - r * row_vec16;
    if (tiled_nv) {                                   // tiled: piece g of (clip, v) is one 16-byte unit of the tile (tiled_d4 of them per vector)
        const int v = (int)(k / tiled_d4), g = (int)(k - (int64_t)v * tiled_d4);
        const int64_t clip = rows[r];
        out[i] = feats[(((clip >> 4) * tiled_nv + v) * tiled_d4 + g) * 16 + (clip & 15)];
    } else {
        out[i] = feats[rows[r] * row_vec16 + k];
    }
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// The results of a query round, device block and (behind the query and the weights) host block alike: avg [N][S] f64 | ne [N][S] i32 |
// scores [N] f64 | result [4] i64 (n_match, n_near, near_argmax, 0) | first kRoundPrefix match rows | first kRoundPrefix near rows;
// every piece starts on a 64-byte boundary.  off[0..5] = the pieces, off[6] = bytes.
static void round_layout(int64_t n, int S, int64_t off[8]) {
    off[0] = 0;
    off[1] = off[0] + up64(n * S * 8);
    off[2] = off[1] + up64(n * S * 4);
    off[3] = off[2] + up64(n * 8);
    off[4] = off[3] + 64;
    off[5] = off[4] + kRoundPrefix * 8;
    off[6] = off[5] + kRoundPrefix * 8;
    off[7] = 0;
}

// shapes the fast one-query kernels (and with them the tiled layout) exist for
static bool fast_scan_shape(const vq_db* db) { return db->D == 1024 && db->S >= 1 && db->S <= 2 && db->E >= 1 && db->E <= 5; }

// rows (by number) -> a dense row-major [L][S][E][D] block in the handle's scratch, whatever the layout; caller holds the lock
int vq::gather_rows_device(vq_db* db, const int64_t* rows_host, int L, const void** dense, const int64_t* rows_dev) {
    const int64_t row_bytes = (int64_t)db->S * db->E * db->D * (int64_t)db->elem();      // D % 4 == 0: whole 16-byte pieces (fp16: 8-byte)
    const int64_t rb = ((int64_t)L * 8 + 15) / 16 * 16;
    VQ_HIP(db->grid_buf.grow((size_t)(rb + (int64_t)L * row_bytes)));
    char* base = db->grid_buf;
    if (!rows_dev) VQ_HIP(hipMemcpyAsync(base, rows_host, (size_t)L * 8, hipMemcpyHostToDevice, db->stream));
    const int64_t* rows = rows_dev ? rows_dev : (const int64_t*)base;
    const bool tiled = db->tiled();
    if (row_bytes % 16) {
        const int64_t vec = row_bytes / 8;
        gather_rows_kernel<uint2><<<cdiv((int64_t)L * vec, 256), 256, 0, db->stream>>>((const uint2*)db->feats, rows, L, vec, (uint2*)(base + rb), 0, 0);
    } else {
        const int64_t vec = row_bytes / 16;
        gather_rows_kernel<uint4><<<cdiv((int64_t)L * vec, 256), 256, 0, db->stream>>>((const uint4*)db->feats, rows, L, vec, (uint4*)(base + rb),
                                                                                      tiled ? db->S * db->E : 0, tiled ? db->D / db->unit() : 0);
    }
    VQ_CHECK_LAUNCH();
    *dense = base + rb;
    return VQ_OK;
}

// In place: a tile's 16 rows and its tiled form occupy the same bytes, so the block is converted a bounded run of tiles at a time
// through a scratch block (rows -> scratch in the new order -> back).  One sweep of reads and writes each way; caller holds the lock.
static int convert_layout(vq_db* db, int to) {
    const int NV = db->S * db->E;
    const int du = db->D * (int)db->elem() / 16;                           // 16-byte units of a vector: what the two kernels move
    const int64_t ntiles = (db->n + 15) / 16, tile_bytes = (int64_t)16 * NV * db->D * (int64_t)db->elem();
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)(256u << 20) / tile_bytes));
    DeviceMem<char> scratch;
    hipError_t e = scratch.grow((size_t)(per * tile_bytes));
    if (e != hipSuccess) return fail(VQ_E_NOMEM, "no room for the %lld MB conversion block: %s", (long long)(per * tile_bytes >> 20), hipGetErrorString(e));
    const size_t lds = 16 * (size_t)(du + 1) * 16;                         // 65 792 bytes (fp32) / 131 328 (fp64) at D = 1024: above the 64 KB default limit
    // raised per (kernel, device) like every other large-LDS launch (vq_common.h); the caller holds a DeviceGuard
    VQ_DYN_LDS(mirror_build_kernel, lds);
    VQ_DYN_LDS(untile_kernel, lds);
    int rc = VQ_OK;
    for (int64_t t0 = 0; t0 < ntiles && rc == VQ_OK; t0 += per) {
        const int64_t k = std::min(per, ntiles - t0);
        char* block = (char*)db->feats + t0 * tile_bytes;
        const int64_t rows_here = std::min<int64_t>(db->n - t0 * 16, k * 16);
        if (to != VQ_LAYOUT_ROWS)
            mirror_build_kernel<<<(unsigned)(k * NV), 256, lds, db->stream>>>((const vq_f4*)block, (vq_f4*)scratch.get(), rows_here, NV, du);
        else
            untile_kernel<<<(unsigned)(k * NV), 256, lds, db->stream>>>((const vq_f4*)block, (vq_f4*)scratch.get(), rows_here, NV, du);
        e = hipGetLastError();
        // tiled -> rows leaves the rows past n of the last tile unwritten in the scratch block: copy whole rows only
        const size_t bytes = to != VQ_LAYOUT_ROWS ? (size_t)(k * tile_bytes) : (size_t)(rows_here * (tile_bytes / 16));
        if (e == hipSuccess) e = hipMemcpyAsync(block, scratch, bytes, hipMemcpyDeviceToDevice, db->stream);
        if (e != hipSuccess) rc = fail(VQ_E_HIP, "layout conversion failed: %s", hipGetErrorString(e));
    }
    e = hipStreamSynchronize(db->stream);
    if (rc == VQ_OK && e != hipSuccess) rc = fail(VQ_E_HIP, "layout conversion failed: %s", hipGetErrorString(e));
    if (rc == VQ_OK) db->layout = to;
    return rc;
}

namespace vq {
int db_copy_scores_ordered(vq_db* db, double* dst_dev, int64_t* n_out, hipStream_t st) {
    VQ_REQUIRE(db && dst_dev, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores: scan (or rescore) first");
    if (db->active >= 0) return fail(VQ_E_UNSUPPORTED, "a row view is in use: the scores cover its %lld positions, not the shard's rows (vq_db_rows_use(db, -1) first)", (long long)db->na);
    DeviceGuard g(db->device);
    if (n_out) *n_out = db->n;
    if (!db->n) return VQ_OK;
    if (st != db->stream) {                     // the scan was only ENQUEUED on db->stream: nothing else orders st behind it
        hipEvent_t ev;
        VQ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, db->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
        (void)hipEventDestroy(ev);              // destruction is deferred until the event has completed
        if (e != hipSuccess) return fail(VQ_E_HIP, "ordering the score copy behind the scan failed: %s", hipGetErrorString(e));
    }
    VQ_HIP(hipMemcpyAsync(dst_dev, db->scores, (size_t)db->n * 8, hipMemcpyDeviceToDevice, st));
    return VQ_OK;
}
}  // namespace vq

extern "C" {

const char* vq_last_error(void) { return last_error_ref().c_str(); }
int vq_abi_version(void) { return VQ_ABI_VERSION; }

int vq_device_count(int* count) {
    VQ_REQUIRE(count, "count is NULL");
    VQ_HIP(hipGetDeviceCount(count));
    return VQ_OK;
}

struct vq_timer_t {
    Event a, b;
};
int vq_timer_create(void** timer) {
    VQ_REQUIRE(timer, "timer is NULL");
    auto t = std::make_unique<vq_timer_t>();
    VQ_HIP(t->a.create());
    VQ_HIP(t->b.create());
    *timer = t.release();
    return VQ_OK;
}
int vq_timer_start(void* timer, void* stream) {
    VQ_HIP(hipEventRecord(static_cast<vq_timer_t*>(timer)->a, (hipStream_t)stream));
    return VQ_OK;
}
int vq_timer_stop(void* timer, void* stream) {
    VQ_HIP(hipEventRecord(static_cast<vq_timer_t*>(timer)->b, (hipStream_t)stream));
    return VQ_OK;
}
int vq_timer_elapsed_ms(void* timer, float* ms) {
    auto* t = static_cast<vq_timer_t*>(timer);
    VQ_HIP(hipEventSynchronize(t->b));
    VQ_HIP(hipEventElapsedTime(ms, t->a, t->b));
    return VQ_OK;
}
int vq_timer_destroy(void* timer) {
    delete static_cast<vq_timer_t*>(timer);
    return VQ_OK;
}

}  // extern "C"

// vq_db_create without and with the flags of include/vq_amd_dim.h: a handle of logical length d stored at pitch D (d <= D, D % 4 == 0; the
// caller has checked both, and S and E); clear: the whole feature block starts as +0.0, not only the rows past n of the last tile
static int create_db(int64_t n, int32_t S, int32_t E, int32_t d, int32_t D, int32_t dtype, int32_t device, bool short_rows, bool clear, vq_db** out) {
    VQ_REQUIRE(dtype == VQ_F32 || dtype == VQ_F64 || dtype == VQ_F16, "dtype must be VQ_F32, VQ_F64 or VQ_F16");
    VQ_REQUIRE(n < (1ll << 31) * (long long)SEL_CHUNK, "n too large");
    int ndev = 0;
    VQ_HIP(hipGetDeviceCount(&ndev));
    VQ_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    auto db = std::make_unique<vq_db>();      // a failing allocation below frees what was made, with the device still current
    db->device = device;
    db->n = n;
    db->na = n;
    db->S = S;
    db->E = E;
    db->D = D;
    db->d = d;
    db->short_rows = short_rows;
    db->dtype = dtype;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) db->cus = prop.multiProcessorCount;
    const size_t nblk = (size_t)cdiv(n, SEL_CHUNK);
    const size_t fbytes = (size_t)((n + 15) / 16 * 16) * S * E * D * db->elem();      // whole tiles of 16 clips (vq_db_set_layout)
    const size_t tbytes = ((size_t)S * E * D * 8 + 63) / 64 * 64;                     // query | weights [8]: adjacent, like the head of a round's host block
    round_layout(n, S, db->round_off);
    const auto nomem = [](hipError_t e, size_t bytes) {
        return e == hipSuccess ? VQ_OK : fail(VQ_E_NOMEM, "vq::malloc_trim(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    };
    const auto alloc = [&](auto& block, size_t bytes) { return nomem(block.grow(bytes), bytes); };
    int rc = nomem(malloc_trim(&db->feats, fbytes), fbytes);
    if (rc == VQ_OK && clear) {
        const hipError_t e = hipMemset(db->feats, 0, fbytes);
        if (e != hipSuccess) return fail(VQ_E_HIP, "clearing the feature block failed: %s", hipGetErrorString(e));
    } else if (rc == VQ_OK && n % 16) {
        (void)hipMemset((char*)db->feats + (size_t)n * S * E * D * db->elem(), 0, fbytes - (size_t)n * S * E * D * db->elem());
    }
    if (rc == VQ_OK) rc = alloc(db->t, tbytes + 64);
    if (rc == VQ_OK) rc = alloc(db->round_dev, (size_t)db->round_off[6]);
    if (rc == VQ_OK) rc = alloc(db->blk_cnt, nblk * sizeof(int2));
    if (rc == VQ_OK) rc = alloc(db->blk_max, nblk * 8);
    if (rc == VQ_OK) rc = alloc(db->blk_arg, nblk * 8);
    if (rc == VQ_OK) rc = alloc(db->rows0, (size_t)n * 8);
    if (rc == VQ_OK) rc = alloc(db->rows1, (size_t)n * 8);
    if (rc == VQ_OK) rc = alloc(db->tk_state, 2 * 8);
    if (rc == VQ_OK) rc = alloc(db->tk_hist, 256 * 4);
    if (rc != VQ_OK) return rc;
    db->w = (double*)((char*)db->t.get() + tbytes);
    db->avg = (double*)(db->round_dev + db->round_off[0]);
    db->ne = (int32_t*)(db->round_dev + db->round_off[1]);
    db->scores = (double*)(db->round_dev + db->round_off[2]);
    db->sel_result = (int64_t*)(db->round_dev + db->round_off[3]);
    db->matchp = (int64_t*)(db->round_dev + db->round_off[4]);
    db->nearp = (int64_t*)(db->round_dev + db->round_off[5]);
    *out = db.release();
    return VQ_OK;
}

extern "C" {

int vq_db_create(int64_t n, int32_t S, int32_t E, int32_t D, int32_t dtype, int32_t device, vq_db** out) {
    VQ_REQUIRE(out, "out is NULL");
    *out = nullptr;
    VQ_REQUIRE(n > 0 && S > 0 && E > 0 && D > 0, "n, S, E, D must be positive (got %lld, %d, %d, %d)", (long long)n, S, E, D);
    VQ_REQUIRE(S <= 8, "at most 8 streams are supported (got %d)", S);
    VQ_REQUIRE(S * E <= 64, "S*E must be <= 64 (got %d)", S * E);
    // include/vq_amd_dim.h: the bits above the storage type.  With VQ_DIM_PADDED (VQ_DIM_SHORT_ROWS implies it) D is the logical
    // length, stored at the next multiple of 4 in a cleared block; without, every check and every byte is what it was
    const int32_t flags = dtype & ~0xFF;
    if (flags == 0) {
        VQ_REQUIRE(D % 4 == 0, "D must be a multiple of 4 (got %d)", D);
        return create_db(n, S, E, D, D, dtype, device, false, false, out);
    }
    VQ_REQUIRE((flags & ~(VQ_DIM_PADDED | VQ_DIM_SHORT_ROWS)) == 0, "dtype carries unknown flag bits (got %d): VQ_DIM_PADDED, VQ_DIM_SHORT_ROWS", dtype);
    VQ_REQUIRE(D <= (1 << 30), "D too large (got %d)", D);
    return create_db(n, S, E, D, (D + 3) / 4 * 4, dtype & 0xFF, device, (flags & VQ_DIM_SHORT_ROWS) != 0, true, out);
}

int vq_db_destroy(vq_db* db) {
    if (!db) return VQ_OK;
    DeviceGuard g(db->device);          // the owners free in the destructor: with the handle's device current
    (void)hipStreamSynchronize(db->stream);
    delete db;
    return VQ_OK;
}

int vq_db_set_stream(vq_db* db, void* s) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    db->stream = (hipStream_t)s;
    return VQ_OK;
}

int vq_db_shape(vq_db* db, int64_t* n, int32_t* S, int32_t* E, int32_t* D, int32_t* dtype) {
    VQ_REQUIRE(db, "db is NULL");
    if (n) *n = db->n;
    if (S) *S = db->S;
    if (E) *E = db->E;
    if (D) *D = db->D;
    if (dtype) *dtype = db->dtype;
    return VQ_OK;
}

static int upload_unpadded(vq_db* db, int64_t row0, int64_t nrows, const void* rows_host);

int vq_db_upload(vq_db* db, int64_t row0, int64_t nrows, const void* feats_host) {
    VQ_REQUIRE(db && feats_host, "NULL argument");
    if (db->d != db->D) return upload_unpadded(db, row0, nrows, feats_host);      // include/vq_amd_dim.h: rows of d elements, padded on the device
    VQ_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= db->n, "rows [%lld,%lld) outside [0,%lld)", (long long)row0,
               (long long)(row0 + nrows), (long long)db->n);
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const size_t row_bytes = (size_t)db->S * db->E * db->D * db->elem();
    if (db->tiled()) {
        // rows land in a staging block and are dealt into their tiles by a kernel, a bounded chunk at a time
        const int64_t chunk = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)row_bytes);
        DeviceMem<float4> stage;
        VQ_HIP(stage.grow((size_t)std::min<int64_t>(chunk, std::max<int64_t>(nrows, 1)) * row_bytes));
        const int NV = db->S * db->E, d4 = db->D / db->unit();           // 16-byte units of a vector
        for (int64_t r = 0; r < nrows; r += chunk) {
            const int64_t k = std::min(chunk, nrows - r);
            hipError_t e = hipMemcpyAsync(stage, (const char*)feats_host + r * row_bytes, k * row_bytes, hipMemcpyHostToDevice, db->stream);
            if (e == hipSuccess) {
                scatter_rows_tiled_kernel<<<cdiv(k * NV * d4, 256), 256, 0, db->stream>>>(stage, (float4*)db->feats, row0 + r, k, NV, d4);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
            if (e != hipSuccess) return fail(VQ_E_HIP, "upload into the tiled layout failed: %s", hipGetErrorString(e));
        }
    } else {
        VQ_HIP(hipMemcpyAsync((char*)db->feats + row0 * row_bytes, feats_host, nrows * row_bytes, hipMemcpyHostToDevice,
                              db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    db->stale();
    return VQ_OK;
}

// vq_db_upload on a handle with d != D: rows_host [nrows][S][E][d], unpadded
static int upload_unpadded(vq_db* db, int64_t row0, int64_t nrows, const void* rows_host) {
    VQ_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= db->n, "rows [%lld,%lld) outside [0,%lld)", (long long)row0,
               (long long)(row0 + nrows), (long long)db->n);
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const int NV = db->S * db->E;
    const size_t row_bytes = (size_t)NV * db->D * db->elem(), raw_bytes = (size_t)NV * db->d * db->elem();
    // the unpadded rows land in a staging block, a bounded chunk at a time, and are written at pitch by a kernel: straight into their
    // rows, or (a tiled database) into a second staging block that is dealt into the tiles as vq_db_upload deals it
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(64u << 20) / (int64_t)row_bytes);
    const size_t most = (size_t)std::min<int64_t>(chunk, std::max<int64_t>(nrows, 1));
    DeviceMem<char> raw;
    DeviceMem<float4> stage;
    VQ_HIP(raw.grow(most * raw_bytes));
    if (db->tiled()) VQ_HIP(stage.grow(most * row_bytes));
    const int d4 = db->tiled() ? db->D / db->unit() : 0;
    for (int64_t r = 0; r < nrows; r += chunk) {
        const int64_t k = std::min(chunk, nrows - r), nvec = k * NV;
        char* dst = db->tiled() ? (char*)stage.get() : (char*)db->feats + (size_t)(row0 + r) * row_bytes;
        hipError_t e = hipMemcpyAsync(raw, (const char*)rows_host + (size_t)r * raw_bytes, (size_t)k * raw_bytes, hipMemcpyHostToDevice, db->stream);
        if (e == hipSuccess) {
            const unsigned blocks = (unsigned)cdiv(nvec * db->D, 256);
            if (db->dtype == VQ_F64)
                pad_rows_kernel<uint64_t><<<blocks, 256, 0, db->stream>>>((const uint64_t*)raw.get(), (uint64_t*)dst, nvec, db->d, db->D);
            else if (db->dtype == VQ_F32)
                pad_rows_kernel<uint32_t><<<blocks, 256, 0, db->stream>>>((const uint32_t*)raw.get(), (uint32_t*)dst, nvec, db->d, db->D);
            else
                pad_rows_kernel<uint16_t><<<blocks, 256, 0, db->stream>>>((const uint16_t*)raw.get(), (uint16_t*)dst, nvec, db->d, db->D);
            e = hipGetLastError();
        }
        if (e == hipSuccess && db->tiled()) {
            scatter_rows_tiled_kernel<<<cdiv(k * NV * d4, 256), 256, 0, db->stream>>>(stage, (float4*)db->feats, row0 + r, k, NV, d4);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(db->stream);      // the staging blocks are reused by the next chunk
        if (e != hipSuccess) return fail(VQ_E_HIP, "upload of unpadded rows failed: %s", hipGetErrorString(e));
    }
    db->stale();
    return VQ_OK;
}

int vq_db_adopt_device(vq_db* db, void* feats_dev) {
    VQ_REQUIRE(db && feats_dev, "NULL argument");
    VQ_REQUIRE(((uintptr_t)feats_dev & 15) == 0, "device feature block must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    db->release_feats();
    db->feats = feats_dev;
    db->owns_feats = false;
    db->stale();
    db->feats_exposed = true;                 // the caller owns the memory (row-major, possibly not whole tiles): never re-tiled
    db->layout = VQ_LAYOUT_ROWS;
    return VQ_OK;
}

int vq_db_set_present(vq_db* db, const uint8_t* present_host) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const size_t bytes = (size_t)db->n * db->S * db->E;
    if (!present_host) {
        db->present = DeviceMem<uint8_t>();
    } else {
        VQ_HIP(db->present.grow(bytes));
        VQ_HIP(hipMemcpyAsync(db->present, present_host, bytes, hipMemcpyHostToDevice, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    db->stale();
    return VQ_OK;
}

int vq_db_generate(vq_db* db, uint64_t seed, int64_t global_row0, const float* scales_host) {
    VQ_REQUIRE(db && scales_host, "NULL argument");
    if (db->d != db->D) return fail(VQ_E_UNSUPPORTED, "the generator fills whole vectors: not for a logical length %d stored at pitch %d (include/vq_amd_dim.h)", db->d, db->D);
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    float* scales_dev = reinterpret_cast<float*>(db->w);   // 64 bytes of scratch; w is rewritten by every scan
    VQ_HIP(hipMemcpyAsync(scales_dev, scales_host, db->S * sizeof(float), hipMemcpyHostToDevice, db->stream));
    const int64_t per_row = (int64_t)db->S * db->E * db->D;
    const int64_t total = db->n * per_row;
    const uint64_t seed_mul = seed * 0x9E3779B97F4A7C15ull;
    const int64_t threads = (total + 3) / 4;
    const int64_t blocks = (threads + 255) / 256;
    VQ_REQUIRE(blocks < (1ll << 31), "DB too large for one generate launch");
    const int rc = with_dtype(db, [&](auto x) {
        using T = decltype(x);
        generate_kernel<T><<<(unsigned)blocks, 256, 0, db->stream>>>((T*)db->feats, total, seed_mul, (uint64_t)(global_row0 * per_row),
                                                                      db->E * db->D, db->S, scales_dev);
        return VQ_OK;
    });
    if (rc != VQ_OK) return rc;
    VQ_CHECK_LAUNCH();
    VQ_HIP(hipStreamSynchronize(db->stream));
    db->stale();
    if (db->tiled()) {                            // the generator writes rows; a tiled database gets its layout back
        const int was = db->layout;
        db->layout = VQ_LAYOUT_ROWS;
        return convert_layout(db, was);
    }
    return VQ_OK;
}

int vq_db_feats_devptr(vq_db* db, void** p) {
    VQ_REQUIRE(db && p, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->layout != VQ_LAYOUT_ROWS) return fail(VQ_E_STATE, "the database is tiled: its block is not [N][S][E][D] (vq_db_set_layout(VQ_LAYOUT_ROWS) first)");
    *p = db->feats;
    db->feats_exposed = true;                 // whoever holds the raw pointer assumes row-major memory: the layout is frozen
    return VQ_OK;
}

int vq_db_set_query(vq_db* db, const double* t_host) {
    VQ_REQUIRE(db && t_host, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    VQ_HIP(hipMemcpyAsync(db->t, t_host, (size_t)db->S * db->E * db->D * 8, hipMemcpyHostToDevice, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    db->have_query = true;
    db->stale();
    return VQ_OK;
}

int vq_db_bootstrap_target(vq_db* db, const int64_t* valid_rows, int32_t n_valid, const int64_t* invalid_rows, int32_t n_invalid,
                           double mu, double* targets_host, int32_t set_query) {
    VQ_REQUIRE(db && valid_rows, "NULL argument");
    VQ_REQUIRE(n_valid >= 1 && n_invalid >= 0 && (n_invalid == 0 || invalid_rows), "need >= 1 validated match (and invalid_rows if n_invalid > 0)");
    for (int k = 0; k < n_valid; ++k)
        VQ_REQUIRE(valid_rows[k] >= 0 && valid_rows[k] < db->n, "valid row %lld outside [0,%lld)", (long long)valid_rows[k], (long long)db->n);
    for (int k = 0; k < n_invalid; ++k)
        VQ_REQUIRE(invalid_rows[k] >= 0 && invalid_rows[k] < db->n, "invalid row %lld outside [0,%lld)", (long long)invalid_rows[k],
                   (long long)db->n);
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const int P = db->S * db->E, stride = n_valid + n_invalid;
    // the validated rows are gathered into a dense [stride][P][D] block first (whatever the layout; tens of rows of 40 KB)
    std::vector<int64_t> rows((size_t)stride);
    for (int k = 0; k < stride; ++k) rows[k] = k < n_valid ? valid_rows[k] : invalid_rows[k - n_valid];
    const void* dense = nullptr;
    int rc = gather_rows_device(db, rows.data(), stride, &dense);
    if (rc != VQ_OK) return rc;
    std::vector<int64_t> off((size_t)P * stride);
    std::vector<int32_t> nv(P, n_valid), ni(P, n_invalid);
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < stride; ++k) off[(size_t)p * stride + k] = ((int64_t)k * P + p) * db->D;      // p = s * E + e
    rc = bootstrap_from_device_rows(dense, db->dtype, off, stride, nv.data(), ni.data(), P, db->D, mu, db->stream, targets_host,
                                    set_query ? db->t.get() : nullptr);
    if (rc != VQ_OK) return rc;
    if (set_query) {
        db->have_query = true;
        db->stale();
    }
    return VQ_OK;
}

int vq_db_set_query_from_row(vq_db* db, int64_t row, double* t_out_host) {
    VQ_REQUIRE(db, "db is NULL");
    VQ_REQUIRE(row >= 0 && row < db->n, "row %lld outside [0,%lld)", (long long)row, (long long)db->n);
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const int NV = db->S * db->E;
    const int rc = with_dtype(db, [&](auto x) {
        using T = decltype(x);
        scale_query_kernel<T><<<NV, 256, 0, db->stream>>>((const T*)db->feats, row, NV, db->D, db->t, db->unit());
        return VQ_OK;
    });
    if (rc != VQ_OK) return rc;
    VQ_CHECK_LAUNCH();
    if (t_out_host) {
        VQ_HIP(hipMemcpyAsync(t_out_host, db->t, (size_t)NV * db->D * 8, hipMemcpyDeviceToHost, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    db->have_query = true;
    db->stale();
    return VQ_OK;
}


int vq_db_read_similarities(vq_db* db, double* avg_host, int32_t* ne_host, double* sims_host) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_avg) return fail(VQ_E_STATE, "no similarities cached (call vq_db_scan first)");
    if (sims_host && !db->have_sims) return fail(VQ_E_STATE, "per-split similarities were not kept (scan with keep_sims=1)");
    DeviceGuard g(db->device);
    if (!db->na) return VQ_OK;                        // an empty row view
    if (avg_host) VQ_HIP(hipMemcpyAsync(avg_host, db->avg, (size_t)db->na * db->S * 8, hipMemcpyDeviceToHost, db->stream));
    if (ne_host) VQ_HIP(hipMemcpyAsync(ne_host, db->ne, (size_t)db->na * db->S * 4, hipMemcpyDeviceToHost, db->stream));
    if (sims_host)
        VQ_HIP(hipMemcpyAsync(sims_host, db->sims, (size_t)db->na * db->S * db->E * 8, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_read_scores(vq_db* db, double* scores_host) {
    VQ_REQUIRE(db && scores_host, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->have_scores) return fail(VQ_E_STATE, "no scores computed (scan with weights, or rescore)");
    DeviceGuard g(db->device);
    if (!db->na) return VQ_OK;
    VQ_HIP(hipMemcpyAsync(scores_host, db->scores, (size_t)db->na * 8, hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_scores_devptr(vq_db* db, void** p) {
    VQ_REQUIRE(db && p, "NULL argument");
    *p = db->scores;
    return VQ_OK;
}
int vq_db_avg_devptr(vq_db* db, void** p) {
    VQ_REQUIRE(db && p, "NULL argument");
    *p = db->avg;
    return VQ_OK;
}
int vq_db_ne_devptr(vq_db* db, void** p) {
    VQ_REQUIRE(db && p, "NULL argument");
    *p = db->ne;
    return VQ_OK;
}

int vq_db_read_rows(vq_db* db, const int64_t* rows_host, int32_t L, void* out_host) {
    VQ_REQUIRE(db && out_host, "NULL argument");
    VQ_REQUIRE(L >= 0 && (L == 0 || rows_host), "bad rows");
    for (int l = 0; l < L; ++l)
        VQ_REQUIRE(rows_host[l] >= 0 && rows_host[l] < db->n, "rows[%d] = %lld outside [0,%lld)", l, (long long)rows_host[l], (long long)db->n);
    if (L == 0) return VQ_OK;
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    const void* dense = nullptr;
    const int rc = gather_rows_device(db, rows_host, L, &dense);
    if (rc != VQ_OK) return rc;
    VQ_HIP(hipMemcpyAsync(out_host, dense, (size_t)L * db->S * db->E * db->D * db->elem(), hipMemcpyDeviceToHost, db->stream));
    VQ_HIP(hipStreamSynchronize(db->stream));
    return VQ_OK;
}

int vq_db_layout(vq_db* db, int32_t* layout) {
    VQ_REQUIRE(db && layout, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    *layout = db->layout;
    return VQ_OK;
}

int vq_db_set_layout(vq_db* db, int32_t layout) {
    VQ_REQUIRE(db, "db is NULL");
    VQ_REQUIRE(layout == VQ_LAYOUT_ROWS || layout == VQ_LAYOUT_TILED || layout == VQ_LAYOUT_TILED64 || layout == VQ_LAYOUT_TILED16,
               "layout must be VQ_LAYOUT_ROWS, VQ_LAYOUT_TILED, VQ_LAYOUT_TILED64 or VQ_LAYOUT_TILED16");
    std::lock_guard<std::mutex> lk(db->mu);
    if (layout == db->layout) return VQ_OK;
    if (layout != VQ_LAYOUT_ROWS) {
        // each storage type has ONE tiled layout (the unit is the 16 bytes a lane loads): TILED is fp32's, TILED64 is fp64's, TILED16 is fp16's
        if (layout != db->tiled_layout() || !fast_scan_shape(db))
            return fail(VQ_E_UNSUPPORTED, "each storage type has one tiled layout -- fp32 VQ_LAYOUT_TILED, fp64 VQ_LAYOUT_TILED64, fp16 VQ_LAYOUT_TILED16 -- for D = 1024, S <= 2, E <= 5 (layout %d: got dtype %d, D %d, S %d, E %d)",
                        layout, db->dtype, db->D, db->S, db->E);
        if (!db->owns_feats || db->feats_exposed)
            return fail(VQ_E_STATE, "the feature block is not the library's alone (adopted, or its address was handed out): it stays row-major");
    }
    DeviceGuard g(db->device);
    return convert_layout(db, layout);
}

int vq_db_write_avg(vq_db* db, const double* avg_host, const int32_t* ne_host) {
    VQ_REQUIRE(db && avg_host, "NULL argument");
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    if (db->na) {
        VQ_HIP(hipMemcpyAsync(db->avg, avg_host, (size_t)db->na * db->S * 8, hipMemcpyHostToDevice, db->stream));
        if (ne_host) VQ_HIP(hipMemcpyAsync(db->ne, ne_host, (size_t)db->na * db->S * 4, hipMemcpyHostToDevice, db->stream));
        VQ_HIP(hipStreamSynchronize(db->stream));
    }
    db->have_avg = true;
    db->have_scores = false;
    return VQ_OK;
}

int vq_host_alloc(void** ptr, int64_t bytes) {
    VQ_REQUIRE(ptr && bytes > 0, "vq_host_alloc: bad argument");
    *ptr = nullptr;
    VQ_HIP(hipHostMalloc(ptr, (size_t)bytes, hipHostMallocDefault));
    return VQ_OK;
}

int vq_host_free(void* ptr) {
    if (ptr) VQ_HIP(hipHostFree(ptr));
    return VQ_OK;
}

int vq_db_round_layout(vq_db* db, int64_t off[10]) {
    VQ_REQUIRE(db && off, "NULL argument");
    const int64_t head = up64((int64_t)db->S * db->E * db->D * 8) + 64;         // query | weights [8]
    off[0] = 0;
    off[1] = head - 64;
    for (int i = 0; i < 6; ++i) off[2 + i] = head + db->round_off[i];
    off[8] = head + db->round_off[6];
    off[9] = kRoundPrefix;
    return VQ_OK;
}

int vq_db_query_round(vq_db* db, void* block, int64_t block_bytes, int32_t flags, double threshold, double lower) {
    VQ_REQUIRE(db && block, "NULL argument");
    VQ_REQUIRE((flags & ~7) == 0 && flags != 0, "flags: 1 = scan, 2 = scores under the block's weights, 4 = select");
    const bool do_scan = flags & 1, do_scores = flags & 2, do_select = flags & 4;
    VQ_REQUIRE(!do_select || do_scores, "a selection needs the scores of the same call");
    int64_t off[10];
    vq_db_round_layout(db, off);
    VQ_REQUIRE(block_bytes >= off[8], "the round block needs %lld bytes (vq_db_round_layout), got %lld", (long long)off[8], (long long)block_bytes);
    std::lock_guard<std::mutex> lk(db->mu);
    if (!do_scan && !db->have_avg) return fail(VQ_E_STATE, "vq_db_query_round: no similarities cached (scan first, or set flag 1)");
    DeviceGuard g(db->device);
    char* host = (char*)block;
    if (do_scan) {                                   // query and weights in ONE copy (adjacent on both sides)
        VQ_HIP(hipMemcpyAsync(db->t, host + off[0], (size_t)(off[1] - off[0]) + (do_scores ? db->S * 8 : 0), hipMemcpyHostToDevice, db->stream));
        db->have_query = true;
        db->stale();
    } else if (do_scores) {
        VQ_HIP(hipMemcpyAsync(db->w, host + off[1], db->S * 8, hipMemcpyHostToDevice, db->stream));
    }
    if (do_scan) {
        const int rc = launch_scan(db, do_scores, false);
        if (rc != VQ_OK) return rc;
        db->have_avg = true;
        db->have_scores = do_scores;
    } else if (do_scores) {
        const int rc = launch_rescore(db);
        if (rc != VQ_OK) return rc;
        db->have_scores = true;
    }
    if (do_select) {
        const int rc = select_threshold(db, threshold, lower, nullptr, true);
        if (rc != VQ_OK) return rc;
    }
    // one copy back: from the similarities (a scan) or from the scores (a re-weighting) to the end of what was computed
    const int first = do_scan ? 0 : 2;
    const int64_t end = do_select ? db->round_off[6] : (do_scores ? db->round_off[3] : db->round_off[2]);
    if (db->active < 0) {
        VQ_HIP(hipMemcpyAsync(host + off[2] + db->round_off[first], db->round_dev + db->round_off[first], (size_t)(end - db->round_off[first]),
                              hipMemcpyDeviceToHost, db->stream));
    } else {
        // a row view: the block keeps the layout for N, every array holds its first M entries and only those travel
        const int64_t m = db->na;
        const int64_t len[3] = {m * db->S * 8, m * db->S * 4, m * 8};
        for (int i = first; i < 3 && db->round_off[i] < end; ++i)
            if (len[i]) VQ_HIP(hipMemcpyAsync(host + off[2] + db->round_off[i], db->round_dev + db->round_off[i], (size_t)len[i], hipMemcpyDeviceToHost, db->stream));
        if (do_select)
            VQ_HIP(hipMemcpyAsync(host + off[2] + db->round_off[3], db->round_dev + db->round_off[3], (size_t)(db->round_off[6] - db->round_off[3]),
                                  hipMemcpyDeviceToHost, db->stream));
    }
    VQ_HIP(hipStreamSynchronize(db->stream));
    if (do_select) {
        const int64_t* res = (const int64_t*)(host + off[5]);
        db->last_n0 = res[0];
        db->last_n1 = res[1];
    }
    return VQ_OK;
}

// ---- row views -------------------------------------------------------------------------------------------------------------------
int vq_db_rows_define(vq_db* db, const int64_t* rows_host, int64_t m, int32_t* view_out) {
    VQ_REQUIRE(db && view_out, "NULL argument");
    VQ_REQUIRE(m >= 0 && m <= db->n && (m == 0 || rows_host), "a row view has 0 <= m <= %lld rows (got %lld)", (long long)db->n, (long long)m);
    for (int64_t i = 0; i < m; ++i) {
        VQ_REQUIRE(rows_host[i] >= 0 && rows_host[i] < db->n, "rows[%lld] = %lld outside [0,%lld)", (long long)i, (long long)rows_host[i], (long long)db->n);
        if (i) {
            VQ_REQUIRE(rows_host[i] != rows_host[i - 1], "rows[%lld] = %lld is a duplicate: a row view lists every row once", (long long)i, (long long)rows_host[i]);
            VQ_REQUIRE(rows_host[i] > rows_host[i - 1], "rows[%lld] = %lld after %lld: a row view is strictly ascending (database order)", (long long)i,
                       (long long)rows_host[i], (long long)rows_host[i - 1]);
        }
    }
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    // the tiled form of the same view, built whenever the database could be tiled: a view defined on rows survives vq_db_set_layout
    std::vector<int64_t> host(rows_host, rows_host + m);
    int64_t ntiles = 0;
    if (fast_scan_shape(db)) {                        // every storage type has a tiled layout at these shapes
        for (int64_t i = 0; i < m; ++i) ntiles += (i == 0 || (rows_host[i] >> 4) != (rows_host[i - 1] >> 4)) ? 1 : 0;
        host.resize((size_t)(m + ntiles + ntiles * 16), -1);
        int64_t* tiles = host.data() + m;
        int64_t* pos = tiles + ntiles;
        int64_t t = -1;
        for (int64_t i = 0; i < m; ++i) {
            if (i == 0 || (rows_host[i] >> 4) != (rows_host[i - 1] >> 4)) tiles[++t] = rows_host[i] >> 4;
            pos[t * 16 + (rows_host[i] & 15)] = i;
        }
    }
    vq_db::RowView v;
    v.defined = true;
    v.m = m;
    v.ntiles = ntiles;
    VQ_HIP(v.rows.grow(std::max<size_t>(64, host.size() * 8)));
    if (ntiles) {
        v.tiles = v.rows + m;
        v.pos = v.tiles + ntiles;
    }
    if (!host.empty()) {
        hipError_t e = hipMemcpyAsync(v.rows, host.data(), host.size() * 8, hipMemcpyHostToDevice, db->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
        if (e != hipSuccess) return fail(VQ_E_HIP, "uploading the row view failed: %s", hipGetErrorString(e));
    }
    size_t slot = 0;
    while (slot < db->views.size() && db->views[slot].defined) ++slot;
    if (slot == db->views.size()) db->views.emplace_back();
    db->views[slot] = std::move(v);
    *view_out = (int32_t)slot;
    return VQ_OK;
}

static int check_view(vq_db* db, int32_t view) {
    if (view < 0 || (size_t)view >= db->views.size() || !db->views[view].defined) return fail(VQ_E_INVALID, "no row view %d on this handle", view);
    return VQ_OK;
}

int vq_db_rows_use(vq_db* db, int32_t view) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (view != -1) {
        const int rc = check_view(db, view);
        if (rc != VQ_OK) return rc;
    }
    if (view == db->active) return VQ_OK;
    db->active = view;
    db->na = view < 0 ? db->n : db->views[view].m;
    // what the handle holds was computed over another population
    db->stale();
    db->last_n0 = db->last_n1 = 0;
    return VQ_OK;
}

int vq_db_rows_drop(vq_db* db, int32_t view) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    const int rc = check_view(db, view);
    if (rc != VQ_OK) return rc;
    if (view == db->active) return fail(VQ_E_STATE, "row view %d is in use (vq_db_rows_use another one, or -1, first)", view);
    DeviceGuard g(db->device);
    VQ_HIP(hipStreamSynchronize(db->stream));            // a scan over it may still be running
    db->views[view] = vq_db::RowView();                  // its block goes with it
    return VQ_OK;
}

int vq_db_rows_active(vq_db* db, int32_t* view, int64_t* m) {
    VQ_REQUIRE(db, "db is NULL");
    std::lock_guard<std::mutex> lk(db->mu);
    if (view) *view = db->active;
    if (m) *m = db->na;
    return VQ_OK;
}

}  // extern "C"
