// The reference's feature files onto a resident database, the decimal text converted on the device (include/vq_amd_csv.h).
//
// Replaces src/api/api_load_records.py:45-58 ([float(x) for x in row[1:]] under csv.reader) for the files the reference's writer
// produces: the host finds the lines (csrc/host/vq_csv_read.cc), the text goes up in chunks of whole lines, and ONE WORKGROUP OF
// 256 THREADS PER LINE
//   1. stages the line in LDS with 16-byte loads (the aligned 16-byte units that cover it; at most 26 D + 22 bytes for written files),
//   2. finds the commas -- each wave walks a quarter of the line 64 bytes at a time, __ballot + popcount give every comma its
//      number -- into a table of D + 1 offsets in LDS,
//   3. converts: thread j takes fields j, j + 256, ... (vq_decimal.h: scan to (w, q), one or two 64 x 64 -> 128 multiplications,
//      correctly rounded binary64, then ONE rounding to the database's type) and stores the element where the database's layout
//      wants it; in the row-major layout a wave's 64 stores are contiguous.
// Every byte a thread looks at lies inside the line's own [start, end) in LDS.  A field the device does not decide goes to a
// bounded list (an atomic counter and a capped array of (line, field)); the host parses those from the text it still holds
// (vq::csv_parse_value) and a second small kernel patches them in.  If the list overflows, the chunk is run again in pieces of so
// few lines that it cannot (the kernel is idempotent), so no field is ever dropped.
#include <algorithm>
#include <cstring>
#include <vector>

#include "host/vq_csv_read.h"
#include "vq_db.h"
#include "vq_decimal.h"

using namespace vq;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kDefaultChunk = 64ll << 20;       // like the staging of an upload into the tiled layout
constexpr int64_t kMaxChunk = 1ll << 30;
constexpr unsigned kFailCap = 1u << 16;             // fields handed to the host per launch

struct CsvArgs {
    const char* text;          // the chunk: 16-byte aligned, allocated in whole 16-byte units
    const int64_t* off;        // [lines + 1] byte offsets of the chunk's lines, relative to the chunk
    const int64_t* rows;       // [lines] database row of each line, -1: skip
    void* feats;
    unsigned* counters;        // [0] fields handed to the host, [1] lines that did not look like what the host indexed (never expected)
    int2* fail_list;           // [fail_cap] (line of the chunk, value field)
    unsigned fail_cap;
    int64_t line0;             // first line of this launch
    int lds_text;              // bytes of LDS for the staged line (multiple of 16); the offset table follows
    int dtype, unit, NV, slot, D;     // unit: elements per 16-byte unit of a tiled block, 0 = row-major (feat_index, csrc/vq_tile_index.h)
    int pitch;                 // D = the fields of a line (the database's logical length), pitch = its stored length: equal unless the handle was created with VQ_DIM_PADDED
};

// the double's bits as the database stores them; false: a finite value that binary16 cannot hold (nothing stored)
__host__ __device__ inline bool storage_bits(int dtype, uint64_t bits, uint64_t* out) {
    int overflow = 0;
    if (dtype == VQ_F64) {
        *out = bits;
    } else if (dtype == VQ_F32) {
        *out = vq_f64_to_f32_bits(bits, &overflow);      // astype(float32): inf is stored
    } else {
        *out = vq_f64_to_f16_bits(bits, &overflow);
        if (overflow) return false;
    }
    return true;
}

__device__ __forceinline__ void store_elem(void* feats, int dtype, int64_t idx, uint64_t v) {
    if (dtype == VQ_F64)
        static_cast<uint64_t*>(feats)[idx] = v;
    else if (dtype == VQ_F32)
        static_cast<uint32_t*>(feats)[idx] = (uint32_t)v;
    else
        static_cast<uint16_t*>(feats)[idx] = (uint16_t)v;
}

__global__ __launch_bounds__(kThreads) void csv_rows_kernel(CsvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ int wave_commas[kThreads / 64];
    const int64_t line = a.line0 + blockIdx.x;
    const int64_t row = a.rows[line];
    if (row < 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t s = a.off[line], e = a.off[line + 1];
    if (e > s && a.text[e - 1] == '\n') --e;
    if (e > s && a.text[e - 1] == '\r') --e;
    const int64_t base = s & ~15ll;
    const int head = (int)(s - base);
    if (e - s > a.lds_text || head + (e - s) > a.lds_text) {      // the host sized the LDS for the longest line: not expected
        if (tid == 0) atomicAdd(&a.counters[1], 1u);
        return;
    }
    const int len = (int)(e - s);
    {
        const int units = (head + len + 15) >> 4;
        const uint4* g = reinterpret_cast<const uint4*>(a.text + base);
        uint4* l = reinterpret_cast<uint4*>(lds);
        for (int u = tid; u < units; u += kThreads) l[u] = g[u];
    }
    __syncthreads();
    const char* t = lds + head;                                    // the line: t[0 .. len)
    int* fo = reinterpret_cast<int*>(lds + a.lds_text);            // fo[k], k < D: where comma k is; fo[D] = len
    const int D = a.D;
    const int seg = (((len + 3) >> 2) + 63) & ~63;
    const int lo = min(wave * seg, len), hi = min(lo + seg, len);
    int count = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        count += __popcll(__ballot(i < hi && t[i] == ','));
    }
    if (lane == 0) wave_commas[wave] = count;
    __syncthreads();
    int run = 0, total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) run += wave_commas[w];
        total += wave_commas[w];
    }
    if (total != D) {                                              // uniform over the workgroup; the host counted the same bytes
        if (tid == 0) atomicAdd(&a.counters[1], 1u);
        return;
    }
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool c = i < hi && t[i] == ',';
        const unsigned long long m = __ballot(c);
        if (c) {
            const int k = run + __popcll(m & ((1ull << lane) - 1ull));
            if (k < D) fo[k] = i;
        }
        run += __popcll(m);
    }
    if (tid == 0) fo[D] = len;
    __syncthreads();
    for (int j = tid; j < D; j += kThreads) {
        const int b = fo[j] + 1, en = fo[j + 1];                   // commas ascend: b <= en <= len
        uint64_t bits = 0, out = 0;
        bool ok = vq_dec_parse(t + b, t + en, &bits) == VQ_DEC_OK;
        if (ok) ok = storage_bits(a.dtype, bits, &out);
        if (ok) {
            store_elem(a.feats, a.dtype, feat_index(a.unit, row, a.NV, a.slot, a.pitch, j), out);
        } else {
            const unsigned k = atomicAdd(&a.counters[0], 1u);
            if (k < a.fail_cap) a.fail_list[k] = make_int2((int)line, j);
        }
    }
}

__global__ void csv_patch_kernel(void* feats, int dtype, const int64_t* idx, const uint64_t* val, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) store_elem(feats, dtype, idx[i], val[i]);
}

}  // namespace

int vq_db_load_csv(vq_db* db, const char* text_host, int64_t bytes, int32_t stream, int32_t split, const int64_t* rows_host, int64_t n_rows,
                   int64_t chunk_bytes, int64_t* host_fields) {
    VQ_REQUIRE(db && text_host, "NULL argument");
    VQ_REQUIRE(bytes >= 0 && n_rows >= 0 && chunk_bytes >= 0 && (rows_host || n_rows == 0), "bytes, n_rows, chunk_bytes >= 0 and rows_host required");
    VQ_REQUIRE(stream >= 0 && stream < db->S && split >= 0 && split < db->E, "slot (%d, %d) outside [0,%d) x [0,%d)", stream, split, db->S, db->E);
    if (host_fields) *host_fields = 0;
    CsvIndex ix;
    int64_t n = 0;
    if (int rc = csv_index(text_host, bytes, true, &ix, &n)) return rc;
    VQ_REQUIRE(n == n_rows, "the file has %lld data rows, rows_host names %lld", (long long)n, (long long)n_rows);
    if (n == 0) return VQ_OK;
    VQ_REQUIRE(ix.dim == db->d, "the file's rows have %d values, the database's %d", ix.dim, db->d);
    {
        std::vector<int64_t> named;
        named.reserve((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            VQ_REQUIRE(rows_host[i] >= -1 && rows_host[i] < db->n, "rows_host[%lld] = %lld outside [-1,%lld)", (long long)i, (long long)rows_host[i], (long long)db->n);
            if (rows_host[i] >= 0) named.push_back(rows_host[i]);
        }
        std::sort(named.begin(), named.end());
        const auto dup = std::adjacent_find(named.begin(), named.end());
        VQ_REQUIRE(dup == named.end(), "rows_host names row %lld twice", (long long)(dup == named.end() ? 0 : *dup));
    }
    const int D = db->d, pitch = db->D;        // fields per line | elements between stored vectors (the pads stay as they are: +0.0)
    int64_t longest = 0;
    for (int64_t i = 0; i < n; ++i) longest = std::max(longest, csv_line_end(text_host + ix.line_off[i], text_host + ix.line_off[i + 1]) - (text_host + ix.line_off[i]));
    if (longest > 65000 - 4 * (int64_t)D)
        return fail(VQ_E_UNSUPPORTED, "a line of %lld bytes with %d values does not fit a workgroup's LDS (at most 65000 - 4 D bytes)", (long long)longest, D);
    const int lds_text = (int)((longest + 15 + 15) / 16 * 16);                  // the line may start up to 15 bytes into its first unit
    const size_t lds_bytes = (size_t)lds_text + 4 * ((size_t)D + 1);
    const int64_t chunk_cap = std::min(kMaxChunk, chunk_bytes == 0 ? kDefaultChunk : chunk_bytes);

    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard g(db->device);
    VQ_DYN_LDS(csv_rows_kernel, 65536 - 64);      // the kernel has 16 static bytes of its own
    // the chunks: maximal runs of whole lines of at most chunk_cap bytes (one line at least)
    std::vector<int64_t> cuts{0};
    int64_t most_bytes = 0, most_lines = 0;
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0 + 1;
        while (i1 < n && ix.line_off[i1 + 1] - ix.line_off[i0] <= chunk_cap) ++i1;
        VQ_REQUIRE(ix.line_off[i1] - ix.line_off[i0] <= kMaxChunk, "a line of more than %lld bytes", (long long)kMaxChunk);
        most_bytes = std::max(most_bytes, ix.line_off[i1] - ix.line_off[i0]);
        most_lines = std::max(most_lines, i1 - i0);
        cuts.push_back(i1);
        i0 = i1;
    }
    const unsigned fail_cap = std::max<unsigned>(kFailCap, (unsigned)D);
    DeviceMem<char> d_text;
    DeviceMem<int64_t> d_off, d_rows, d_pidx;
    DeviceMem<uint64_t> d_pval;
    DeviceMem<unsigned> d_counters;
    DeviceMem<int2> d_fail;
    VQ_HIP(d_text.grow((size_t)(most_bytes + 15) / 16 * 16 + 16));
    VQ_HIP(d_off.grow((size_t)(most_lines + 1) * 8));
    VQ_HIP(d_rows.grow((size_t)most_lines * 8));
    VQ_HIP(d_counters.grow(16));
    VQ_HIP(d_fail.grow((size_t)fail_cap * sizeof(int2)));
    std::vector<int64_t> rel;
    std::vector<int2> list;
    std::vector<int64_t> pidx;
    std::vector<uint64_t> pval;
    int64_t resolved = 0;
    const int unit = db->unit();
    const int NV = db->S * db->E, slot = stream * db->E + split;

    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const int64_t i0 = cuts[c], i1 = cuts[c + 1], lines = i1 - i0, c0 = ix.line_off[i0], cbytes = ix.line_off[i1] - c0;
        rel.resize((size_t)lines + 1);
        for (int64_t k = 0; k <= lines; ++k) rel[(size_t)k] = ix.line_off[i0 + k] - c0;
        VQ_HIP(hipMemcpyAsync(d_text.get(), text_host + c0, (size_t)cbytes, hipMemcpyHostToDevice, db->stream));
        VQ_HIP(hipMemcpyAsync(d_off.get(), rel.data(), (size_t)(lines + 1) * 8, hipMemcpyHostToDevice, db->stream));
        VQ_HIP(hipMemcpyAsync(d_rows.get(), rows_host + i0, (size_t)lines * 8, hipMemcpyHostToDevice, db->stream));
        CsvArgs a;
        a.text = d_text.get();
        a.off = d_off.get();
        a.rows = d_rows.get();
        a.feats = db->feats;
        a.counters = d_counters.get();
        a.fail_list = d_fail.get();
        a.fail_cap = fail_cap;
        a.lds_text = lds_text;
        a.dtype = db->dtype;
        a.unit = unit;
        a.NV = NV;
        a.slot = slot;
        a.D = D;
        a.pitch = pitch;
        // the whole chunk in one launch; if it hands back more fields than the list holds, again in pieces that cannot
        int64_t piece = lines;
        for (int64_t l0 = 0; l0 < lines;) {
            const int64_t l1 = std::min(lines, l0 + piece);
            unsigned counters[2] = {0, 0};
            VQ_HIP(hipMemsetAsync(d_counters.get(), 0, 16, db->stream));
            a.line0 = l0;
            csv_rows_kernel<<<(unsigned)(l1 - l0), kThreads, lds_bytes, db->stream>>>(a);
            VQ_CHECK_LAUNCH();
            VQ_HIP(hipMemcpyAsync(counters, d_counters.get(), 8, hipMemcpyDeviceToHost, db->stream));
            VQ_HIP(hipStreamSynchronize(db->stream));
            if (counters[1]) return fail(VQ_E_STATE, "the device counted other fields than the host in %u lines from line %lld on", counters[1], (long long)(i0 + l0 + 2));
            if (counters[0] > fail_cap) {                        // only ever on the first, whole-chunk launch
                piece = std::max<int64_t>(1, fail_cap / (unsigned)D);
                continue;
            }
            const unsigned cnt = counters[0];
            if (cnt) {
                list.resize(cnt);
                VQ_HIP(hipMemcpy(list.data(), d_fail.get(), (size_t)cnt * sizeof(int2), hipMemcpyDeviceToHost));
                std::sort(list.begin(), list.end(), [](const int2& x, const int2& y) { return x.x != y.x ? x.x < y.x : x.y < y.y; });
                pidx.resize(cnt);
                pval.resize(cnt);
                for (unsigned k = 0; k < cnt; ++k) {
                    const int64_t li = i0 + list[k].x;            // data row of the file; its line is li + 2 (1-based, after the header)
                    const int field = list[k].y + 1;
                    const char* lb = text_host + ix.line_off[li];
                    const char* le = csv_line_end(lb, text_host + ix.line_off[li + 1]);
                    const char *fb = nullptr, *fe = nullptr;
                    uint64_t bits = 0, out = 0;
                    if (!csv_field(lb, le, field, &fb, &fe) || csv_parse_value(fb, fe, &bits) != 0)
                        return fail(VQ_E_INVALID, "line %lld field %d: '%.*s' is not a number", (long long)(li + 2), field,
                                    fb ? (int)std::min<int64_t>(40, fe - fb) : 0, fb ? fb : "");
                    if (!storage_bits(db->dtype, bits, &out))
                        return fail(VQ_E_INVALID, "line %lld field %d: %.*s does not fit float16 (largest finite value 65504)", (long long)(li + 2), field,
                                    (int)std::min<int64_t>(40, fe - fb), fb);
                    pidx[k] = feat_index(unit, rows_host[li], NV, slot, pitch, list[k].y);
                    pval[k] = out;
                }
                VQ_HIP(d_pidx.grow((size_t)fail_cap * 8));
                VQ_HIP(d_pval.grow((size_t)fail_cap * 8));
                VQ_HIP(hipMemcpyAsync(d_pidx.get(), pidx.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, db->stream));
                VQ_HIP(hipMemcpyAsync(d_pval.get(), pval.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, db->stream));
                csv_patch_kernel<<<cdiv(cnt, 256), 256, 0, db->stream>>>(db->feats, db->dtype, d_pidx.get(), d_pval.get(), (int)cnt);
                VQ_CHECK_LAUNCH();
                VQ_HIP(hipStreamSynchronize(db->stream));
                resolved += cnt;
            }
            l0 = l1;
        }
    }
    db->stale();
    if (host_fields) *host_fields = resolved;
    return VQ_OK;
}
