// Hot path A on gfx950: the frozen TSN BN-Inception forward pass + segment consensus.
//
// What it replaces (paths relative to the reference checkout):
//   src/features_GPU_compute/calcSig_wOF.py:88-113  per-snippet CaffeNet forward (rgb / flow)
//   src/features_GPU_compute/calcSig_wOF.py:82      np.array(frame_features).mean(axis=0)  (consensus)
//   src/features_GPU_compute/models/ucf101/tsn_bn_inception_{rgb,flow}_deploy.prototxt  (the layers)
//
// Layout: activations NHWC fp32 in HBM, one tensor slot per blob; a Concat output is one slot and
// its producers write at their channel offset (zero-copy concat).  Convolution + frozen BN + ReLU is a
// single kernel launch over all B*T crops of a batch:
//   * direct form (vq_tsn_conv.hip): implicit GEMM, M = crops*Ho*Wo pixels, N = Cout, K = k*k*Cin, on the fp32
//     matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, 256 FLOP/clk/CU) from LDS-staged,
//     register-prefetched tiles -- the 1x1, stride-2 and stem layers;
//   * Winograd F(2x2,3x3) form (vq_wino.hip) -- the 3x3 / stride-1 layers.
// Preprocessing, pooling, the class-score layer and the consensus: vq_tsn_ops.hip.  This file has no kernel: it is the handle, the
// executor, the autotuner, the device pool and the entry points.  The executor has the plan validated and the launch sequence built once (host/vq_tsn_plan.cc: everything that needs no GPU),
// autotunes the tiling per layer and batch size, and runs the layer list on one stream (profiling) or as sub-batches on several
// (production).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "vq_common.h"
#include "vq_tsn_conv.h"
#include "vq_tsn_kernels.h"
#include "host/vq_block_pool.h"

using namespace vq;

// ------------------------------------------------------------------------------------------------
// handle + executor
// ------------------------------------------------------------------------------------------------
// What one launch needs beyond the plan: where it goes, what it covers, which events time it.  Handed down the launch path, which
// reads the handle (const vq_tsn*) and writes nothing into it; a function that changes a field for what it calls makes a copy.
struct Launch {
    hipStream_t stream;
    hipEvent_t ev_start, ev_stop;   // profiling (both may be null)
    int crop0;                      // first crop the launch works on (sub-batches, 32-bit offset chunks)
    int T;                          // snippets per clip of the forward in flight
    bool fused_consensus;           // the global pool launch also forms the consensus (whole clips per launch, T <= kMaxFusedT)
};

// Activation slots, weights and split-K scratch of a closed extractor are kept (up to VQ_DEVICE_POOL_GB, default 40; 0 = off) for the
// next one of the same shape in the process: on some hosts a hipMalloc of tens of GB right behind the hipFree of as much waits ~1 s for
// the driver to reclaim the memory (seen as 1.2 s extractor builds in back-to-back command-line runs of one process).  A block is only
// reused at its exact size on its device; whatever a forward reads it has written before.
// bookkeeping in csrc/host/vq_block_pool.cc (host-only, sanitizer-built); the HIP calls stay here
static vq::BlockPool& device_pool() {
    static vq::BlockPool p(vq::BlockPool::cap_from_env());
    return p;
}
void vq::device_pool_trim() {
    for (void* blk : device_pool().drain()) (void)hipFree(blk);
}

namespace vq {
// Move-only owner of a block that comes from the pool and goes back to it (to the driver when the pool is full or off).  Whoever
// destroys it has made sure that nothing on the device still uses the block: the pool hands it to the next extractor as it is.
struct PoolBlock {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
    PoolBlock() = default;
    PoolBlock(PoolBlock&& o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr; }
    PoolBlock& operator=(PoolBlock&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p, bytes = o.bytes, device = o.device;
            o.p = nullptr;
        }
        return *this;
    }
    PoolBlock(const PoolBlock&) = delete;
    PoolBlock& operator=(const PoolBlock&) = delete;
    ~PoolBlock() { reset(); }
    // a pooled block of exactly this size on this device, else hipMalloc; out of memory: the pooled blocks go back and it tries once more
    hipError_t alloc(int dev, size_t n) {
        reset();
        void* q = device_pool().take(dev, n);
        if (!q) {
            hipError_t e = hipMalloc(&q, n);
            if (e == hipErrorOutOfMemory) {
                (void)hipGetLastError();
                vq::device_pool_trim();
                e = hipMalloc(&q, n);
            }
            if (e != hipSuccess) return e;
        }
        p = q, bytes = n, device = dev;
        return hipSuccess;
    }
    void reset() {
        if (p && !device_pool().give(device, p, bytes)) (void)hipFree(p);
        p = nullptr;
    }
    float* floats() const { return static_cast<float*>(p); }
};
}  // namespace vq

// The members that own something on the device come last, in the REVERSE of the order they are released in: the profiling ring, the
// sub-batch events and streams go first, then the blocks return to the pool or the driver.  vq_tsn_destroy deletes the handle with
// its device current and behind a hipDeviceSynchronize: a block never reaches the pool while something may still use it.
struct vq_tsn {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    int max_crops = 0;
    int in_channels = 0;
    TsnPlan plan;                         // tensors, layers, launch sequence, K splits: everything decided without the GPU (host/vq_tsn_plan.h)
    TsnOptions opt;                       // the VQ_TSN_* switches of the environment, read at creation (host/vq_tsn_plan.h)
    std::map<int, std::vector<int>> tuned;   // tile_key(n_crops, paired) -> per-layer index into kTiles / Winograd variant
    std::map<int, int> split_pref;           // batch size -> 0: this size runs faster on ONE stream than as sub-batches (vq_tsn_set_split); absent: split
    std::set<int> tuned_borrowed;            // keys whose table was copied from a neighbouring size by ensure_tuned (not measured: never persisted)
    int forced_tile = -1;                 // VQ_TSN_TILE: every direct conv uses this tiling
    std::vector<int> seg_table_off;       // per layer: first entry of seg_table
    size_t split_slice_floats = 0;        // floats between the slices of split_scratch (= max_crops * plan.split_crop_floats)
    int64_t blob_floats = 0;
    int feature_slot = -1;
    std::vector<float> mean_cached;       // what mean_dev holds (uploaded only when the caller's mean changes)
    int last_crops = 0;
    int profile_depth = 0;                // > 0: HIP events around every launch (bench roofline accounting)
    int profile_count = 0;                // profiled forwards so far (ring of profile_depth event sets)
    int profile_every = 1;                // while profiling: every n-th forward carries the events, all run on one stream
    int profile_tick = 0;                 // forwards since vq_tsn_set_profile
    bool profile_split = false;           // while profiling: the un-sampled forwards run split over the sub-batch streams (vq_tsn_set_profile_split)
    int n_split = 1;                      // VQ_TSN_SPLIT: sub-batches of one forward run on separate streams
    std::vector<int> split_parts;         // VQ_TSN_SPLIT=a,b,..: relative sizes of the sub-batches (default equal)
    int parts_sum = 1;                    // ... and their sum
    // ---- what the handle owns on the device, last released first
    DeviceMem<double> feat_dev;           // [max_crops][D] (B <= max_crops)
    DeviceMem<float> mean_dev;
    DeviceMem<uint8_t> crops_dev;         // host crops on their way in: grows with the largest forward
    DeviceMem<float> zero_bias;           // zeros for the slices' epilogues (the bias is added once, by the combine pass)
    PoolBlock split_scratch;              // [slice][max_crops * Ho * Wo][Cout] partial sums of the split layer in flight
    DeviceMem<ConvSeg> seg_table;         // destination tables of all conv layers, back to back
    DeviceMem<float> zeros;               // 256 bytes of zeros (load target of masked lanes)
    PoolBlock blob;                       // weights + biases
    std::vector<PoolBlock> slots;         // device activations, max_crops each
    std::vector<Stream> split_streams;    // [n_split]; entry 0 unused (caller's stream)
    Event fork_ev;
    std::vector<Event> join_ev;           // per extra stream
    std::vector<Event> events;            // profile_depth x n_items x {start, stop}

    float* slot(int i) const { return slots[(size_t)i].floats(); }
};

// May layer L be given tiling t: by the sweep (timed), which tries every tiling with a kernel for the layer, or by the occupancy
// heuristic, which scores the plain kernel's BK = 32 tilings (launch_conv then finds a pooled-input layer its substitute)
static bool tile_candidate(const vq_layer_desc& L, const ConvTile& t, bool timed) {
    if (!timed) return t.pipe == 0 && t.bk == 32 && t.conv[0];
    if (L.pre_pool_k > 0 ? !pooled_ok(t, L.cin) : !t.conv[0]) return false;
    return t.bn < 2 * ((L.cout + 63) / 64 * 64);     // a column tile that is mostly padding cannot win: do not let a timing fluke choose it
}

static int heuristic_tile(const vq_tsn* net, int li, int n_crops) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    const int M = n_crops * td.h * td.w, N = L.cout;
    int best = 0;
    double bs = -1;
    for (int i = 0; i < kNumTiles; ++i) {
        const ConvTile& t = kTiles[i];
        if (!tile_candidate(L, t, false)) continue;
        const long long tiles = (long long)cdiv(M, t.bm) * cdiv(N, t.bn);
        const double per_cu = (double)tiles / net->cus;
        const double balance = per_cu / std::ceil(per_cu);                      // tail quantisation
        const double padding = ((double)M * N) / ((double)tiles * t.bm * t.bn); // ragged edges
        const double area = (double)t.bm * t.bn;
        const double intrinsic = area >= 128 * 128 ? 1.0 : area >= 128 * 96 ? 0.97 : area >= 128 * 64 ? 0.92 : area >= 64 * 64 ? 0.8 : 0.7;
        const double sc = balance * padding * intrinsic;
        if (sc > bs) {
            bs = sc;
            best = i;
        }
    }
    return best;
}

static void fill_conv_args(const vq_tsn* net, const Launch& ln, int li, int n_crops, ConvArgs& a) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& ts = net->plan.tensors[L.src];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    a.in = net->slot(L.src) + (size_t)ln.crop0 * ts.h * ts.w * ts.c;
    a.out = net->slot(L.dst);
    a.out_row0 = ln.crop0 * td.h * td.w;
    a.w = net->blob.floats() + L.w_off;
    a.bias = net->blob.floats() + L.b_off;
    a.zeros = net->zeros.get();
    a.segs = net->seg_table.get() + net->seg_table_off[li];
    a.H = ts.h;
    a.W = ts.w;
    a.Cs_in = ts.c;
    a.coff_in = L.src_coff;
    a.Cin = L.cin;
    a.Ho = td.h;
    a.Wo = td.w;
    a.Cs_out = td.c;
    a.coff_out = L.dst_coff;
    a.Cout = L.cout;
    a.k = L.k;
    a.kw = L.k;
    a.col_off = 4;
    a.c_step = 0;        // 0: the kernel's BK
    a.stride = L.stride;
    a.pad = L.pad;
    a.M = n_crops * td.h * td.w;
    a.Kp = (L.k * L.k * L.cin + KPAD - 1) / KPAD * KPAD;
    a.relu = L.relu;
    a.pool_k = L.pre_pool_k;
    a.pool_s = L.pre_pool_stride;
    a.ksplit = 1;
    a.k_per = 0;
    a.seg_stride = 0;
    a.tiles_m = a.tiles_n = 0;
    a.in_bytes = (unsigned)((size_t)n_crops * ts.h * ts.w * ts.c * sizeof(float));   // < 2^31: LaunchItem::max_crops
    a.w_bytes = (unsigned)((size_t)L.cout * a.Kp * sizeof(float));
}

static int launch_conv_layer(const vq_tsn* net, const Launch& ln, int li, int n_crops, int tile_idx) {
    ConvArgs a;
    fill_conv_args(net, ln, li, n_crops, a);
    const vq_layer_desc& L = net->plan.layers[li];
    // A convolution without padding that reads ALL channels of its slot finds the kw taps of a kernel row side by side
    // in memory ([kw][Cin] is one contiguous run of the NHWC row, and the packed weights have the same order): fold the
    // row into the channel axis -- k rows of one tap with kw*Cin channels.  The space-to-depth stem (4x4 over 12
    // channels) becomes 4 taps of 48 contiguous floats and, with BK = 16, runs on the aligned path: no per-chunk tap
    // decoding in its K loop.
    const bool stem_rows = L.src == 0 && net->plan.input.s2d_pad >= 0 && net->plan.input.s2d_order == 1;
    if (stem_rows) {
        // The x-major space-to-depth stem (vq_input_desc.s2d_order = 1): a kernel row is 7 x-taps x (2 rows x c channels) = 14 c contiguous
        // floats of the slot (RGB: 42, + 2 of the next pixel against zero weights = 44; flow stack: 140), and the weights are packed
        // [Cout][steps][4 rows][4]: chunk column r of a staged row holds kernel row r, every K-step advances 4 floats along all four
        // rows at once.  K = 176 (RGB) / 560 (flow) instead of the 192 / 640 of the (p,q,c) order, whose zero taps are scattered
        // through every 16-float step -- with the address arithmetic of the aligned path (a per-lane row offset fixed for the whole
        // loop, a uniform scalar offset per step).
        a.k = a.kw = 1;
        a.Cin = 4 * L.k * L.cin;                       // never reached: the walk stays inside its one "tap"
        a.col_off = net->plan.tensors[L.src].w * net->plan.tensors[L.src].c;
        a.c_step = 4;
        a.Kp = stem_rows_kp(net->plan.input.c);
        a.w_bytes = (unsigned)((size_t)L.cout * a.Kp * sizeof(float));
    } else if (L.pad == 0 && L.k > 1 && L.cin == net->plan.tensors[L.src].c && L.src_coff == 0) {
        a.kw = 1;
        a.Cin = L.k * L.cin;
    }
    // (a tiling without a kernel for this layer: launch_conv's message, with the layer in front)
    auto run = [&](const Launch& on) {
        const int rc = launch_conv(tile_idx, a, on.stream, on.ev_start, on.ev_stop);
        return rc == VQ_E_INVALID ? fail(rc, "layer %d: %s", li, std::string(last_error_ref()).c_str()) : rc;
    };
    if (net->plan.ksplit[li] == 1) return run(ln);
    // K slices into the scratch planes (zero bias, no ReLU: the slice tables say so), then the combine pass into the
    // layer's destination.  The profiling events bracket the pair: the slices carry the start event, the combine pass the stop event.
    a.ksplit = net->plan.ksplit[li];
    a.k_per = a.Kp / a.ksplit;
    a.seg_stride = (L.cout + 31) / 32;
    a.bias = net->zero_bias.get();
    // Sub-batches of one forward run on separate streams and may be at DIFFERENT split layers at the same moment: every
    // crop owns a fixed stretch of each scratch plane (split_crop_floats, room for the largest split layer), and a
    // launch writes its [M][Cout] partial sums at the first whole row inside the stretch of its first crop.
    a.out_row0 = (int)cdiv((int64_t)ln.crop0 * (int64_t)net->plan.split_crop_floats, (int64_t)L.cout);
    Launch slices = ln, combine = ln;
    slices.ev_stop = nullptr;
    combine.ev_start = nullptr;
    const int rc = run(slices);
    if (rc != VQ_OK) return rc;
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    float* out = net->slot(L.dst) + (size_t)ln.crop0 * td.h * td.w * td.c + L.dst_coff;
    VQ_REQUIRE((int64_t)a.M * L.cout < (1ll << 31) && (int64_t)a.M * td.c < (1ll << 31), "layer %d: K-split combine pass beyond 32-bit offsets (split the batch)", li);
    return launch_splitk_combine(net->split_scratch.floats() + (size_t)a.out_row0 * L.cout, a.ksplit, net->split_slice_floats, a.M, L.cout,
                                 net->blob.floats() + L.b_off, L.relu, out, td.c, combine.stream, combine.ev_start, combine.ev_stop);
}

static void fill_wino_job(const vq_tsn* net, const Launch& ln, int li, int n_crops, WinoJob& a, int variant) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& ts = net->plan.tensors[L.src];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    memset(&a, 0, sizeof a);
    a.in = net->slot(L.src) + (size_t)ln.crop0 * ts.h * ts.w * ts.c;
    a.u = net->blob.floats() + L.w_off;
    a.bias = net->blob.floats() + L.b_off;
    a.out = net->slot(L.dst) + (size_t)ln.crop0 * td.h * td.w * td.c;
    a.H = ts.h;
    a.W = ts.w;
    a.Cs_in = ts.c;
    a.coff_in = L.src_coff;
    a.Cin = L.cin;
    a.Cs_out = td.c;
    a.coff_out = L.dst_coff;
    a.Cout = L.cout;
    a.th = (ts.h + 1) / 2;
    a.tw = (ts.w + 1) / 2;
    a.P = n_crops * a.th * a.tw;
    a.relu = L.relu;
    // VQ_OP_CONV_WINOGRAD16: both filter layouts, the 32-tile one first; variants 2, 3 run the units of 16 tiles on the second
    a.t16 = L.op == VQ_OP_CONV_WINOGRAD16 && variant >= 2;
    if (a.t16) a.u += (size_t)16 * L.cout * L.cin;
    a.in_bytes = (unsigned)((size_t)n_crops * ts.h * ts.w * ts.c * sizeof(float));
    a.out_bytes = (unsigned)((size_t)n_crops * td.h * td.w * td.c * sizeof(float));
    a.u_bytes = (unsigned)((size_t)16 * L.cout * L.cin * sizeof(float));
}

static void fill_pool_args(const vq_tsn* net, const Launch& ln, int li, int n_crops, PoolArgs& a) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& ts = net->plan.tensors[L.src];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    memset(&a, 0, sizeof a);
    a.in = net->slot(L.src) + (size_t)ln.crop0 * ts.h * ts.w * ts.c;
    a.out = net->slot(L.dst) + (size_t)ln.crop0 * td.h * td.w * td.c;
    a.H = ts.h;
    a.W = ts.w;
    a.Cs_in = ts.c;
    a.coff_in = L.src_coff;
    a.C = L.cin;
    a.Ho = td.h;
    a.Wo = td.w;
    a.Cs_out = td.c;
    a.coff_out = L.dst_coff;
    a.k = L.k;
    a.stride = L.stride;
    a.pad = L.pad;
    a.is_max = L.op == VQ_OP_MAXPOOL;
    a.total = (int64_t)n_crops * td.h * td.w * (L.cin / 4);
    a.bias = (L.op == VQ_OP_AVGPOOL && L.has_bias) ? net->blob.floats() + L.b_off : nullptr;
    a.relu = (L.op == VQ_OP_AVGPOOL) ? L.relu : 0;
    // the specialised path addresses both slots with 32-bit byte offsets; slots beyond that keep the generic path (mode 0)
    const size_t in_bytes = (size_t)n_crops * ts.h * ts.w * ts.c * sizeof(float), out_bytes = (size_t)n_crops * td.h * td.w * td.c * sizeof(float);
    a.in_bytes = in_bytes <= 0x7FFFFFF0u ? (unsigned)in_bytes : 0u;
    a.out_bytes = out_bytes <= 0x7FFFFFF0u ? (unsigned)out_bytes : 0u;
    pool_plan(a, n_crops);
}

// The Winograd layers among `members` (independent of each other) plus the pooling layers among them as one launch.
static int launch_wino_layers(const vq_tsn* net, const Launch& ln, const std::vector<int>& members, int n_crops, int variant) {
    WinoGroup g;
    memset(&g, 0, sizeof g);
    for (int li : members) {
        if (is_wino(net->plan.layers[li].op)) {
            VQ_REQUIRE(g.n_jobs < kWinoMaxJobs, "a Winograd launch carries at most %d convolutions", kWinoMaxJobs);
            fill_wino_job(net, ln, li, n_crops, g.job[g.n_jobs++], variant);
        } else {
            VQ_REQUIRE(g.n_pools < kWinoMaxPools, "a Winograd launch carries at most %d pooling layers", kWinoMaxPools);
            fill_pool_args(net, ln, li, n_crops, g.pool[g.n_pools++]);
        }
    }
    bool both = true;
    for (int li : members)
        if (net->plan.layers[li].op == VQ_OP_CONV_WINOGRAD) both = false;
    if (variant >= 2 && !both) {                         // a table written for another layout: the same channel blocks on 32 tiles (same bits)
        variant -= 2;
        for (int q = 0; q < g.n_jobs; ++q) VQ_REQUIRE(!g.job[q].t16, "internal: mixed Winograd layouts in one launch");
    }
    return launch_wino_group(g, variant, ln.stream, ln.ev_start, ln.ev_stop);
}

static int run_layer(const vq_tsn* net, const Launch& ln, int li, int n_crops, int tune_key);

// Launch one item on crops [crop0, crop0 + n_crops) of the batch; tune_key = the batch size whose tuning table applies.
// A launch addresses its slots with 32-bit byte offsets, so an item whose slots exceed 2^31 bytes at this batch size
// runs as several launches over crop ranges (the results do not depend on the cut: every crop is independent).
// `whole`: the stream, the events around the item and its first crop (crop0).
static int run_item(const vq_tsn* net, const Launch& whole, const LaunchItem& it, int n_crops, int tune_key) {
    for (int done = 0; done < n_crops;) {
        const int n = std::min(n_crops - done, it.max_crops);
        Launch ln = whole;
        ln.crop0 = whole.crop0 + done;
        // profiling: the first chunk carries the start event, the last one the stop event
        if (done != 0) ln.ev_start = nullptr;
        if (done + n != n_crops) ln.ev_stop = nullptr;
        int rc;
        if (it.kind == 1) {
            auto tn = net->tuned.find(tune_key);
            rc = launch_wino_layers(net, ln, it.layers, n, tn != net->tuned.end() ? tn->second[it.layers[0]] : 0);
        } else {
            rc = run_layer(net, ln, it.layers[0], n, tune_key);
        }
        if (rc != VQ_OK) return rc;
        done += n;
    }
    return VQ_OK;
}

// Time every candidate tiling of every conv launch at this batch size (activations hold whatever the slots
// contain; only durations matter) and keep the fastest.
// The chip's clock follows its load: a sweep that starts on an idle GPU times its first candidates at a lower clock than its last ones
// (round 5: a 96-crop table tuned at the start of a test, behind seconds of host work, gave the first three launches of the forward -- conv1,
// conv2/3x3_reduce, the inception_3a group -- the LAST candidates of the list, one of them 1.8x slower than the best: 2.91 ms per step
// instead of 2.73, kept by the tiling cache).  So the sweep starts behind ~30 ms of the forward's own launches, and the fastest
// candidates of a launch are timed again, back to back, before the winner is taken.
// ``paired``: the size is that of a SUB-BATCH of the default forward (two sub-batches on two streams, side by side): a candidate is timed
// the way it will run -- the same launch on all sub-batch streams at once, on the crop ranges of the sub-batches -- because the best tiling of a
// launch that has the chip to itself (few, large workgroups fill it badly) is not the best one beside its twin.
// A table lives under tile_key(size, paired): a size tuned side by side is another table than the same size tuned alone.
constexpr int kPairedKey = 1 << 24;
static inline int tile_key(int n_crops, bool paired) { return n_crops + (paired ? kPairedKey : 0); }

static int autotune(vq_tsn* net, int n_crops, bool paired) {
    const int key = tile_key(n_crops, paired);
    std::vector<int>& choice = net->tuned[key];
    choice.assign(net->plan.layers.size(), 0);
    net->tuned_borrowed.erase(key);
    const int ways = paired ? std::max(1, std::min(net->n_split, net->max_crops / n_crops)) : 1;     // streams that run the launch side by side
    Event e0, e1;
    std::vector<Event> f((size_t)ways);                       // f[1 .. ways-1]
    VQ_HIP(e0.create());
    VQ_HIP(e1.create());
    for (int l = 1; l < ways; ++l) VQ_HIP(f[l].create());
    // way l: the launch on crops [l * n_crops, (l + 1) * n_crops) on its stream (only durations matter: no clips, no consensus)
    std::vector<Launch> way((size_t)ways);
    for (int l = 0; l < ways; ++l) way[l] = Launch{l > 0 ? net->split_streams[l] : net->stream, nullptr, nullptr, l * n_crops, 1, false};
    auto timed = [&](const LaunchItem& it, int reps, float* ms) -> int {
        VQ_HIP(hipEventRecord(e0, net->stream));
        int rc = run_item(net, way[0], it, n_crops, key);      // warm
        if (rc != VQ_OK) return rc;
        VQ_HIP(hipEventRecord(e1, net->stream));
        VQ_HIP(hipEventSynchronize(e1));
        float warm = 0.f;
        VQ_HIP(hipEventElapsedTime(&warm, e0, e1));
        // long launches need fewer repetitions (the command line's first run on a machine tunes two networks at 2 x 400 crops) -- but not
        // one look at a 0.3 ms launch: with that, the 224-crop tables of cfg 3 came out 9 % slower (2 345 against 2 580 clips/s)
        // (and with two looks at launches above 0.5 ms still 2 480: only launches of more than 2 ms are timed once)
        if (warm > 2.0f) reps = 1;
        VQ_HIP(hipEventRecord(e0, net->stream));
        for (int l = 1; l < ways; ++l) VQ_HIP(hipStreamWaitEvent(net->split_streams[l], e0, 0));
        for (int r = 0; r < reps; ++r)
            for (int l = 0; l < ways; ++l) {
                rc = run_item(net, way[l], it, n_crops, key);
                if (rc != VQ_OK) return rc;
            }
        VQ_HIP(hipEventRecord(e1, net->stream));
        for (int l = 1; l < ways; ++l) VQ_HIP(hipEventRecord(f[l], net->split_streams[l]));
        VQ_HIP(hipEventSynchronize(e1));
        VQ_HIP(hipEventElapsedTime(ms, e0, e1));
        for (int l = 1; l < ways; ++l) {
            float other = 0.f;
            VQ_HIP(hipEventSynchronize(f[l]));
            VQ_HIP(hipEventElapsedTime(&other, e0, f[l]));
            *ms = std::max(*ms, other);
        }
        return VQ_OK;
    };
    {   // bring the clock up: the heuristic tilings (choice = 0 entries are replaced below) through the whole launch list
        std::vector<int> saved = choice;
        net->tuned.erase(key);                                // run_layer falls back to the heuristic without a table
        for (int r = 0; r < 10; ++r)
            for (const LaunchItem& it : net->plan.items) {
                const int rc = run_item(net, way[0], it, n_crops, key);
                if (rc != VQ_OK) return rc;
            }
        VQ_HIP(hipStreamSynchronize(net->stream));
        net->tuned[key] = saved;
    }
    std::vector<int>& pick = net->tuned[key];
    for (const LaunchItem& it : net->plan.items) {
        const int li = it.layers[0];
        if (!is_conv(net->plan.layers[li].op)) continue;
        const bool wino = is_wino(net->plan.layers[li].op);
        std::vector<std::pair<float, int>> seen;
        const int n_wino = net->plan.layers[li].op == VQ_OP_CONV_WINOGRAD16 ? 2 * kWinoVariants : kWinoVariants;     // + the 16-tile units
        for (int t = 0; t < (wino ? n_wino : kNumTiles); ++t) {
            if (!wino && !tile_candidate(net->plan.layers[li], kTiles[t], true)) continue;
            for (int m : it.layers) pick[m] = t;               // a grouped launch runs one variant for all its members
            float ms = 0.f;
            const int rc = timed(it, 3, &ms);
            if (rc != VQ_OK) return rc;
            seen.emplace_back(ms, t);
        }
        std::sort(seen.begin(), seen.end());
        float best = 1e30f;
        int win = seen.empty() ? 0 : seen[0].second;
        for (size_t k = 0; k < std::min<size_t>(3, seen.size()) && seen.size() > 1; ++k) {      // the finalists, back to back
            for (int m : it.layers) pick[m] = seen[k].second;
            float ms = 0.f;
            const int rc = timed(it, 5, &ms);
            if (rc != VQ_OK) return rc;
            if (ms < best) {
                best = ms;
                win = seen[k].second;
            }
        }
        for (int m : it.layers) pick[m] = win;
    }
    return VQ_OK;
}

// Make sure a tiling table exists for this batch size.  The first size seen is autotuned; a later size within 1.6x of
// a tuned one borrows that table (the ragged last batch of a video must not cost 2 s of tuning launches -- every
// tiling gives the same bits, only the speed differs); anything further away is tuned itself.
static int ensure_tuned(vq_tsn* net, int n_crops, bool paired) {
    const int key = tile_key(n_crops, paired);
    if (net->forced_tile >= 0 || net->tuned.find(key) != net->tuned.end()) return VQ_OK;
    // the nearest size timed the same way (side by side / alone); failing that the nearest one timed the other way
    for (const bool p : {paired, !paired}) {            // the nearest size timed the same way; failing that the other way
        std::vector<int> sizes;                                   // measured (not borrowed) tables of that pairing
        for (const auto& kv : net->tuned)
            if ((kv.first >= kPairedKey) == p && !net->tuned_borrowed.count(kv.first)) sizes.push_back(kv.first - (p ? kPairedKey : 0));
        if (const int nearest = nearest_size(sizes, n_crops)) {
            net->tuned[key] = net->tuned[tile_key(nearest, p)];
            net->tuned_borrowed.insert(key);
            return VQ_OK;
        }
    }
    if (!net->opt.autotune) return VQ_OK;             // VQ_TSN_AUTOTUNE=0: the occupancy heuristic for sizes without a table
    return autotune(net, n_crops, paired);
}

static int run_layer(const vq_tsn* net, const Launch& ln, int li, int n_crops, int tune_key) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& ts = net->plan.tensors[L.src];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    if (L.op == VQ_OP_CONV) {
        int t = net->forced_tile;   // VQ_TSN_TILE (read at creation): test / tuning aid
        if (t < 0) {
            auto it = net->tuned.find(tune_key);
            t = it != net->tuned.end() ? it->second[li] : heuristic_tile(net, li, n_crops);
        }
        return launch_conv_layer(net, ln, li, n_crops, t);
    }
    if (is_wino(L.op)) {
        auto it = net->tuned.find(tune_key);
        return launch_wino_layers(net, ln, std::vector<int>{li}, n_crops, it != net->tuned.end() ? it->second[li] : 0);
    }
    if (L.op == VQ_OP_MAXPOOL || L.op == VQ_OP_AVGPOOL) {
        PoolArgs a;
        fill_pool_args(net, ln, li, n_crops, a);
        return launch_pool(a, ln.stream, ln.ev_start, ln.ev_stop);
    }
    if (L.op == VQ_OP_GLOBAL_AVGPOOL) {
        const float* gin = net->slot(L.src) + (size_t)ln.crop0 * ts.h * ts.w * ts.c;
        float* gout = net->slot(L.dst) + (size_t)ln.crop0 * td.c;
        const int T = ln.T;
        // the feature blob: global pool and segment consensus in one pass (the launch covers whole clips)
        if (li == net->plan.consensus_layer && ln.fused_consensus)
            return launch_gavgpool_consensus(gin, gout, net->feat_dev.get() + (size_t)(ln.crop0 / T) * net->plan.D, n_crops / T, T, ts.h * ts.w, ts.c,
                                             L.src_coff, L.cin, td.c, L.dst_coff, ln.stream, ln.ev_start, ln.ev_stop);
        return launch_gavgpool(gin, gout, n_crops, ts.h * ts.w, ts.c, L.src_coff, L.cin, td.c, L.dst_coff, ln.stream, ln.ev_start, ln.ev_stop);
    }
    if (L.op == VQ_OP_INNER_PRODUCT) {
        const float* xin = net->slot(L.src) + (size_t)ln.crop0 * ts.c + L.src_coff;
        float* yout = net->slot(L.dst) + (size_t)ln.crop0 * td.c + L.dst_coff;
        return launch_inner_product(xin, ts.c, net->blob.floats() + L.w_off, net->blob.floats() + L.b_off, yout, td.c, n_crops, L.cin, L.cout, ln.stream,
                                    ln.ev_start, ln.ev_stop);
    }
    return fail(VQ_E_INVALID, "layer %d: unknown op %d", li, L.op);
}

extern "C" {

int vq_tsn_create(const vq_tensor_desc* tensors, int32_t n_tensors, const vq_layer_desc* layers, int32_t n_layers,
                  const vq_conv_segment* segments, int32_t n_segments, const float* blob_host, int64_t blob_floats,
                  const vq_input_desc* input, int32_t feature_slot, int32_t max_crops, int32_t device, vq_tsn** out) {
    VQ_REQUIRE(out, "out is NULL");
    *out = nullptr;
    TsnPlan plan;
    const int vrc = validate_plan(tensors, n_tensors, layers, n_layers, segments, n_segments, blob_host, blob_floats, input, feature_slot, max_crops, &plan);
    if (vrc != VQ_OK) return vrc;
    const int in_channels = input->c;
    int ndev = 0;
    VQ_HIP(hipGetDeviceCount(&ndev));
    VQ_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    auto net = std::make_unique<vq_tsn>();     // a failed step below releases what the steps before it made (with the device current)
    net->device = device;
    net->max_crops = max_crops;
    net->in_channels = in_channels;
    net->plan = std::move(plan);
    net->feature_slot = feature_slot;
    net->blob_floats = blob_floats;
    net->opt = tsn_options_from_env();
    const TsnOptions& opt = net->opt;
    if (opt.tile_set) net->forced_tile = tile_index(opt.tile[0], opt.tile[1], opt.tile[2], opt.tile[3]);
    net->n_split = opt.n_split;
    net->split_parts = opt.split_parts;
    net->parts_sum = parts_sum(net->split_parts);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) net->cus = prop.multiProcessorCount;
    net->slots.resize(n_tensors);
    for (int i = 0; i < n_tensors; ++i)
        VQ_HIP(net->slots[i].alloc(device, (size_t)max_crops * tensors[i].h * tensors[i].w * tensors[i].c * sizeof(float)));
    VQ_HIP(net->blob.alloc(device, (size_t)blob_floats * sizeof(float)));
    VQ_HIP(hipMemcpy(net->blob.p, blob_host, (size_t)blob_floats * sizeof(float), hipMemcpyHostToDevice));
    // the K split of the 7 x 7 layers (choose_ksplit) and its scratch planes; VQ_TSN_SPLITK=0 turns it off (A/B measurements)
    choose_ksplit(net->plan, opt.splitk);
    if (net->plan.split_crop_floats > 0) {
        net->split_slice_floats = (size_t)max_crops * net->plan.split_crop_floats;
        VQ_HIP(net->split_scratch.alloc(device, net->split_slice_floats * 4 * sizeof(float)));      // up to 4 slices
        VQ_HIP(net->zero_bias.grow((size_t)net->plan.max_cout * sizeof(float)));
        VQ_HIP(hipMemset(net->zero_bias, 0, net->zero_bias.bytes));
    }
    {   // destination tables: one entry per 32 output columns of every convolution
        std::vector<ConvSeg> table;
        net->seg_table_off.assign(n_layers, 0);
        for (int i = 0; i < n_layers; ++i) {
            const vq_layer_desc& L = layers[i];
            if (L.op != VQ_OP_CONV) continue;
            net->seg_table_off[i] = (int)table.size();
            if (net->plan.ksplit[i] > 1) {       // slice q of a split layer writes plane q of the scratch, raw
                for (int q = 0; q < net->plan.ksplit[i]; ++q)
                    for (int b = 0; b < (L.cout + 31) / 32; ++b)
                        table.push_back(ConvSeg{net->split_scratch.floats() + (size_t)q * net->split_slice_floats, L.cout, 0});
                continue;
            }
            if (L.seg_count > 0) {
                int col0 = 0;
                for (int q = 0; q < L.seg_count; ++q) {
                    const vq_conv_segment& sg = segments[L.seg_first + q];
                    for (int b = 0; b < sg.cout / 32; ++b)
                        table.push_back(ConvSeg{net->slot(sg.dst) + sg.dst_coff - col0, tensors[sg.dst].c, sg.relu});
                    col0 += sg.cout;
                }
            } else {
                for (int b = 0; b < (L.cout + 31) / 32; ++b)
                    table.push_back(ConvSeg{net->slot(L.dst) + L.dst_coff, tensors[L.dst].c, L.relu});
            }
        }
        VQ_HIP(net->seg_table.grow(std::max<size_t>(table.size(), 1) * sizeof(ConvSeg)));
        VQ_HIP(hipMemcpy(net->seg_table, table.data(), table.size() * sizeof(ConvSeg), hipMemcpyHostToDevice));
    }
    build_items(net->plan, opt.group_wino, opt.group_pool);
    net->split_streams.resize(net->n_split);
    net->join_ev.resize(net->n_split);
    for (int l = 1; l < net->n_split; ++l) {
        VQ_HIP(net->split_streams[l].create(hipStreamNonBlocking));
        VQ_HIP(net->join_ev[l].create(hipEventDisableTiming));
    }
    VQ_HIP(net->fork_ev.create(hipEventDisableTiming));
    VQ_HIP(net->zeros.grow(256));
    VQ_HIP(hipMemset(net->zeros, 0, 256));
    VQ_HIP(net->mean_dev.grow((size_t)in_channels * sizeof(float)));
    VQ_HIP(net->feat_dev.grow((size_t)max_crops * net->plan.D * sizeof(double)));
    *out = net.release();
    return VQ_OK;
}

int vq_tsn_destroy(vq_tsn* net) {
    if (!net) return VQ_OK;
    DeviceGuard g(net->device);
    // everything that may still read or write the blocks must be done before the pool hands them to the next extractor: the
    // handle's stream, its sub-batch streams, a stream set earlier (the hipFree this replaced waited for the whole device too)
    (void)hipDeviceSynchronize();
    delete net;                  // inside the guard: the members release what they own with the handle's device current
    return VQ_OK;
}

int vq_tsn_set_stream(vq_tsn* net, void* s) {
    VQ_REQUIRE(net, "net is NULL");
    std::lock_guard<std::mutex> lk(net->mu);
    net->stream = (hipStream_t)s;
    return VQ_OK;
}

// The launches of one forward, in order, on net->stream (and the sub-batch streams): preprocess, the launch items, the consensus.
static int forward_launches(vq_tsn* net, const uint8_t* src, int n_crops, int T, const BatchCut& cut, const Event* ev) {
    const std::vector<int>&sub = cut.sub, &sub_off = cut.sub_off;
    const int n_split = (int)sub.size();
    const vq_tensor_desc& t0 = net->plan.tensors[0];
    const int in_c = net->in_channels;
    const int n_items = (int)net->plan.items.size();
    // uint8 crops [crop0, crop0 + n) -> the fp32 input slot, on stream st
    auto preprocess = [&](int crop0, int n, hipStream_t st) -> int {
        return launch_preprocess(src + (size_t)crop0 * net->plan.input.h * net->plan.input.w * in_c, net->slot(0) + (size_t)crop0 * t0.h * t0.w * t0.c, n,
                                 net->plan.input, t0, net->mean_dev, st);
    };
    if (n_split > 1) {
        // Batch split: the sub-batches are independent, so each runs the whole launch list -- its share of the preprocessing included
        // -- on its own stream with no synchronisation in between; one sub-batch's launch ramp and tail overlap the other's steady
        // state.  (Measured in round 5, tools/trace_prod.sh: the two streams run in step, the GPU is idle 0.007 of 2.6 ms; letting
        // sub-batch b start k launches behind sub-batch b-1, so that memory-bound and compute-bound launches meet, LOSES:
        // 12 090 -> 11 950 / 11 870 / 11 670 clips/s for k = 1 / 2 / 3: the lone tail costs more than the mixing gains.)
        VQ_HIP(hipEventRecord(net->fork_ev, net->stream));
        for (int l = 1; l < n_split; ++l) VQ_HIP(hipStreamWaitEvent(net->split_streams[l], net->fork_ev, 0));
        for (int sb = 0; sb < n_split; ++sb) {
            const int rc = preprocess(sub_off[sb], sub[sb], sb > 0 ? net->split_streams[sb] : net->stream);
            if (rc != VQ_OK) return rc;
        }
        Launch on[8];                                     // n_split <= 8 (VQ_TSN_SPLIT)
        for (int sb = 0; sb < n_split; ++sb)
            on[sb] = Launch{sb > 0 ? net->split_streams[sb] : net->stream, nullptr, nullptr, sub_off[sb], T, cut.fused_consensus};
        for (const LaunchItem& it : net->plan.items)
            for (int sb = 0; sb < n_split; ++sb) {
                const int rc = run_item(net, on[sb], it, sub[sb], tile_key(sub[sb], true));
                if (rc != VQ_OK) return rc;
            }
        for (int l = 1; l < n_split; ++l) {
            VQ_HIP(hipEventRecord(net->join_ev[l], net->split_streams[l]));
            VQ_HIP(hipStreamWaitEvent(net->stream, net->join_ev[l], 0));
        }
    } else {
        const int prc = preprocess(0, n_crops, net->stream);
        if (prc != VQ_OK) return prc;
        for (int q = 0; q < n_items; ++q) {
            const Launch ln{net->stream, ev ? ev[2 * q].v : nullptr, ev ? ev[2 * q + 1].v : nullptr, 0, T, cut.fused_consensus};
            const int rc = run_item(net, ln, net->plan.items[q], n_crops, tile_key(n_crops, false));
            if (rc != VQ_OK) return rc;
        }
    }
    if (ev) ++net->profile_count;
    const int B = n_crops / T;
    if (!cut.fused_consensus)                     // consensus not fused into the global-pool launch: separate pass
        return launch_consensus(net->slot(net->feature_slot), net->feat_dev, B, T, net->plan.D, net->plan.D, net->stream);
    return VQ_OK;
}

int vq_tsn_forward(vq_tsn* net, const uint8_t* crops, int32_t crops_on_device, int32_t n_crops, int32_t T,
                   const float* mean_host, double* feat_host, float* per_snippet_host) {
    VQ_REQUIRE(net && crops && mean_host, "NULL argument");
    VQ_REQUIRE(n_crops > 0 && n_crops <= net->max_crops, "n_crops %d outside (0,%d]", n_crops, net->max_crops);
    VQ_REQUIRE(T > 0 && n_crops % T == 0, "n_crops (%d) must be a multiple of T (%d)", n_crops, T);
    std::lock_guard<std::mutex> lk(net->mu);
    DeviceGuard g(net->device);
    const int in_c = net->in_channels;
    const int64_t npix = (int64_t)n_crops * net->plan.input.h * net->plan.input.w;
    const uint8_t* src = crops;
    if (!crops_on_device) {
        const size_t bytes = (size_t)npix * in_c;
        VQ_HIP(net->crops_dev.grow(bytes));
        VQ_HIP(hipMemcpyAsync(net->crops_dev, crops, bytes, hipMemcpyHostToDevice, net->stream));
        src = net->crops_dev;
    }
    if (net->mean_cached.size() != (size_t)in_c || memcmp(net->mean_cached.data(), mean_host, in_c * sizeof(float)) != 0) {
        net->mean_cached.assign(mean_host, mean_host + in_c);     // pageable copy from a buffer that outlives this call
        VQ_HIP(hipMemcpyAsync(net->mean_dev, net->mean_cached.data(), in_c * sizeof(float), hipMemcpyHostToDevice, net->stream));
        VQ_HIP(hipStreamSynchronize(net->stream));
    }
    if (net->opt.poison)
        for (size_t i = 0; i < net->slots.size(); ++i) {
            const vq_tensor_desc& t = net->plan.tensors[i];
            VQ_HIP(hipMemsetAsync(net->slot(i), 0xFF, (size_t)net->max_crops * t.h * t.w * t.c * sizeof(float), net->stream));
        }
    const int n_items = (int)net->plan.items.size();
    const Event* ev = nullptr;
    const bool profiling = net->profile_depth > 0;
    if (profiling && net->profile_tick++ % net->profile_every == 0)
        ev = net->events.data() + (size_t)(net->profile_count % net->profile_depth) * (2 * n_items);
    // A sampled forward stays on the caller's stream (each duration is then the launch alone); so do the forwards between two
    // sampled ones (they issue exactly the same launches) unless vq_tsn_set_profile_split asked for the product's own mode there.
    bool one_stream = profiling && (ev || !net->profile_split);
    if (!one_stream && !net->split_pref.empty()) {       // a measured preference of the nearest batch size within 1.6x (default: split)
        std::vector<int> sizes;
        for (const auto& kv : net->split_pref) sizes.push_back(kv.first);
        const int best = nearest_size(sizes, n_crops);
        if (best > 0 && net->split_pref[best] == 0) one_stream = true;
    }
    const BatchCut cut = cut_batch(net->plan, n_crops, T, net->split_parts, net->parts_sum, one_stream);
    const int n_split = (int)cut.sub.size();
    for (int sb = 0; sb < n_split; ++sb) {      // n_split == 1: sub[0] is the whole batch
        const int rc = ensure_tuned(net, cut.sub[sb], n_split > 1);
        if (rc != VQ_OK) return rc;
    }
    const int frc = forward_launches(net, src, n_crops, T, cut, ev);
    if (frc != VQ_OK) return frc;
    net->last_crops = n_crops;
    const int B = n_crops / T;
    if (feat_host)
        VQ_HIP(hipMemcpyAsync(feat_host, net->feat_dev, (size_t)B * net->plan.D * sizeof(double), hipMemcpyDeviceToHost, net->stream));
    if (per_snippet_host)
        VQ_HIP(hipMemcpyAsync(per_snippet_host, net->slot(net->feature_slot), (size_t)n_crops * net->plan.D * sizeof(float),
                              hipMemcpyDeviceToHost, net->stream));
    if (feat_host || per_snippet_host || !crops_on_device) VQ_HIP(hipStreamSynchronize(net->stream));
    return VQ_OK;
}

int vq_tsn_feat_devptr(vq_tsn* net, void** feat_dev, void** per_snippet_dev) {
    VQ_REQUIRE(net, "net is NULL");
    if (feat_dev) *feat_dev = net->feat_dev;
    if (per_snippet_dev) *per_snippet_dev = net->slot(net->feature_slot);
    return VQ_OK;
}

int vq_tsn_read_tensor(vq_tsn* net, int32_t slot, int32_t n_crops, float* host) {
    VQ_REQUIRE(net && host, "NULL argument");
    VQ_REQUIRE(slot >= 0 && slot < (int)net->plan.tensors.size(), "slot out of range");
    VQ_REQUIRE(n_crops > 0 && n_crops <= net->max_crops, "n_crops out of range");
    std::lock_guard<std::mutex> lk(net->mu);
    DeviceGuard g(net->device);
    const vq_tensor_desc& t = net->plan.tensors[slot];
    VQ_HIP(hipMemcpyAsync(host, net->slot(slot), (size_t)n_crops * t.h * t.w * t.c * sizeof(float), hipMemcpyDeviceToHost,
                          net->stream));
    VQ_HIP(hipStreamSynchronize(net->stream));
    return VQ_OK;
}

int vq_tsn_set_profile(vq_tsn* net, int32_t depth) {
    VQ_REQUIRE(net, "net is NULL");
    VQ_REQUIRE(depth >= 0 && depth <= 1024, "profile depth must be in [0,1024]");
    std::lock_guard<std::mutex> lk(net->mu);
    DeviceGuard g(net->device);
    VQ_HIP(hipStreamSynchronize(net->stream));
    std::vector<Event> ring((size_t)depth * 2 * net->plan.items.size());      // swapped in only when complete
    for (Event& e : ring) VQ_HIP(e.create());
    net->events = std::move(ring);
    net->profile_depth = depth;
    net->profile_count = 0;
    net->profile_tick = 0;
    return VQ_OK;
}

int vq_tsn_set_profile_every(vq_tsn* net, int32_t every) {
    VQ_REQUIRE(net && every >= 1, "every must be >= 1");
    std::lock_guard<std::mutex> lk(net->mu);
    net->profile_every = every;
    net->profile_tick = 0;
    return VQ_OK;
}

// Share of a grouped launch's time attributed to one member, as a rough time estimate: matrix-core work of a
// convolution (16 multiplies per tile and channel pair) at 100 TFLOP/s, bytes of a pooling layer at 4 TB/s.
static double wino_weight(const vq_tsn* net, int li) {
    const vq_layer_desc& L = net->plan.layers[li];
    const vq_tensor_desc& td = net->plan.tensors[L.dst];
    if (!is_wino(L.op)) {
        const vq_tensor_desc& ts = net->plan.tensors[L.src];
        return ((double)ts.h * ts.w + (double)td.h * td.w) * L.cin * 4.0 / 4e12;
    }
    return 2.0 * 16.0 * ((td.h + 1) / 2) * ((td.w + 1) / 2) * (double)L.cin * L.cout / 100e12;
}

int vq_tsn_set_profile_split(vq_tsn* net, int32_t unsampled_split) {
    VQ_REQUIRE(net, "net is NULL");
    std::lock_guard<std::mutex> lk(net->mu);
    net->profile_split = unsampled_split != 0;
    return VQ_OK;
}

int vq_tsn_layer_times(vq_tsn* net, float* ms, double* flops, int32_t n_layers) {
    VQ_REQUIRE(net && ms, "NULL argument");
    VQ_REQUIRE(n_layers == (int)net->plan.layers.size(), "n_layers must be %d", (int)net->plan.layers.size());
    std::lock_guard<std::mutex> lk(net->mu);
    if (net->profile_depth == 0 || net->profile_count == 0) return fail(VQ_E_STATE, "no profiled forward has run");
    DeviceGuard g(net->device);
    VQ_HIP(hipStreamSynchronize(net->stream));
    const int sets = std::min(net->profile_count, net->profile_depth);
    const int n_items = (int)net->plan.items.size();
    for (int i = 0; i < n_layers; ++i) ms[i] = 0.f;
    for (int sidx = 0; sidx < sets; ++sidx) {
        const Event* ev = net->events.data() + (size_t)sidx * (2 * n_items);
        for (int q = 0; q < n_items; ++q) {
            float t = 0.f;
            VQ_HIP(hipEventElapsedTime(&t, ev[2 * q], ev[2 * q + 1]));
            const LaunchItem& it = net->plan.items[q];
            double wsum = 0;
            for (int m : it.layers) wsum += it.kind == 1 ? wino_weight(net, m) : 1.0;
            for (int m : it.layers)                               // a grouped launch: split by matrix-core work
                ms[m] += (float)(t / sets * ((it.kind == 1 ? wino_weight(net, m) : 1.0) / wsum));
        }
    }
    if (flops) {
        for (int i = 0; i < n_layers; ++i) {
            const vq_layer_desc& L = net->plan.layers[i];
            const vq_tensor_desc& td = net->plan.tensors[L.dst];
            flops[i] = is_conv(L.op) ? 2.0 * net->last_crops * td.h * td.w * L.cout * first_layer_k2c(net->plan.input, L)
                                          : (L.op == VQ_OP_INNER_PRODUCT ? 2.0 * net->last_crops * L.cin * L.cout : 0.0);
        }
    }
    return VQ_OK;
}

int vq_tsn_launch_items(vq_tsn* net, int32_t* item_of_layer, int32_t n_layers, int32_t* n_items) {
    VQ_REQUIRE(net && item_of_layer && n_items, "NULL argument");
    VQ_REQUIRE(n_layers == (int)net->plan.layers.size(), "n_layers must be %d", (int)net->plan.layers.size());
    for (int i = 0; i < n_layers; ++i) item_of_layer[i] = net->plan.item_of_layer[i];
    *n_items = (int)net->plan.items.size();
    return VQ_OK;
}

int vq_tsn_tuned_sizes(vq_tsn* net, int32_t* sizes, int32_t cap, int32_t* n) {
    VQ_REQUIRE(net && n && (cap == 0 || sizes), "NULL argument");
    std::lock_guard<std::mutex> lk(net->mu);
    std::set<int> distinct;
    for (const auto& kv : net->tuned) distinct.insert(kv.first >= kPairedKey ? kv.first - kPairedKey : kv.first);
    int k = 0;
    for (int v : distinct) {
        if (k < cap) sizes[k] = v;
        ++k;
    }
    *n = k;
    return VQ_OK;
}

int vq_device_pool_trim(void) {
    vq::device_pool_trim();
    return VQ_OK;
}

int vq_tsn_set_split(vq_tsn* net, int32_t n_crops, int32_t split) {
    VQ_REQUIRE(net && n_crops > 0, "bad argument");
    std::lock_guard<std::mutex> lk(net->mu);
    if (split < 0)
        net->split_pref.erase(n_crops);
    else
        net->split_pref[n_crops] = split ? 1 : 0;
    return VQ_OK;
}

int vq_tsn_tune(vq_tsn* net, int32_t n_crops, int32_t paired) {
    VQ_REQUIRE(net, "net is NULL");
    VQ_REQUIRE(n_crops > 0 && n_crops * (paired ? std::min(net->n_split, 2) : 1) <= net->max_crops, "n_crops out of range");
    std::lock_guard<std::mutex> lk(net->mu);
    DeviceGuard g(net->device);
    const int rc = autotune(net, n_crops, paired != 0);
    if (rc != VQ_OK) net->tuned.erase(tile_key(n_crops, paired != 0));
    VQ_HIP(hipStreamSynchronize(net->stream));
    return rc;
}

int vq_tsn_tile_tables(vq_tsn* net, int32_t* sizes, int32_t* flags, int32_t cap, int32_t* n) {
    VQ_REQUIRE(net && n && (cap == 0 || (sizes && flags)), "NULL argument");
    std::lock_guard<std::mutex> lk(net->mu);
    int k = 0;
    for (const auto& kv : net->tuned) {
        if (k < cap) {
            const bool paired = kv.first >= kPairedKey;
            sizes[k] = paired ? kv.first - kPairedKey : kv.first;
            flags[k] = (paired ? 1 : 0) | (net->tuned_borrowed.count(kv.first) ? 2 : 0);
        }
        ++k;
    }
    *n = k;
    return VQ_OK;
}

int vq_tsn_get_tiles(vq_tsn* net, int32_t n_crops, int32_t paired, int32_t* tiles, int32_t n_layers) {
    VQ_REQUIRE(net && tiles, "NULL argument");
    VQ_REQUIRE(n_layers == (int)net->plan.layers.size(), "n_layers must be %d", (int)net->plan.layers.size());
    std::lock_guard<std::mutex> lk(net->mu);
    auto it = net->tuned.find(tile_key(n_crops, paired != 0));
    for (int i = 0; i < n_layers; ++i) {
        tiles[4 * i] = tiles[4 * i + 1] = tiles[4 * i + 2] = tiles[4 * i + 3] = 0;
        if (is_wino(net->plan.layers[i].op)) {   // 32 tiles (128 pixels) x 32 (v+1) channels, 8 channels per step
            const int lead = net->plan.items[net->plan.item_of_layer[i]].layers[0];   // a grouped launch runs ONE variant: its first member's
            const int v = it != net->tuned.end() ? it->second[lead] : 0;
            tiles[4 * i] = v >= 2 ? 64 : 128;             // pixels per unit: 16 or 32 tiles of 2 x 2
            tiles[4 * i + 1] = 32 * ((v & 1) + 1);
            tiles[4 * i + 2] = v >= 2 ? 16 : 8;           // channels per step
            tiles[4 * i + 3] = 2;
            continue;
        }
        if (net->plan.layers[i].op != VQ_OP_CONV) continue;
        const int t = it != net->tuned.end() ? it->second[i] : heuristic_tile(net, i, n_crops);
        tiles[4 * i] = kTiles[t].bm;
        tiles[4 * i + 1] = kTiles[t].bn;
        tiles[4 * i + 2] = kTiles[t].bk;
        tiles[4 * i + 3] = kTiles[t].pipe;
    }
    return VQ_OK;
}

int vq_tsn_layer_tiles(vq_tsn* net, int32_t n_crops, int32_t* tiles, int32_t n_layers) {
    VQ_REQUIRE(net, "NULL argument");
    bool paired = false;
    {
        std::lock_guard<std::mutex> lk(net->mu);
        paired = net->tuned.find(tile_key(n_crops, false)) == net->tuned.end() && net->tuned.find(tile_key(n_crops, true)) != net->tuned.end();
    }
    return vq_tsn_get_tiles(net, n_crops, paired ? 1 : 0, tiles, n_layers);
}

int vq_tsn_set_tiles(vq_tsn* net, int32_t n_crops, int32_t paired, const int32_t* tiles, int32_t n_layers) {
    VQ_REQUIRE(net && tiles, "NULL argument");
    VQ_REQUIRE(n_layers == (int)net->plan.layers.size(), "n_layers must be %d", (int)net->plan.layers.size());
    VQ_REQUIRE(n_crops > 0 && n_crops <= net->max_crops, "n_crops out of range");
    std::vector<int> choice(net->plan.layers.size(), 0);
    for (int i = 0; i < n_layers; ++i) {
        if (is_wino(net->plan.layers[i].op)) {
            const int bn = tiles[4 * i + 1], bk = tiles[4 * i + 2];
            const bool t16 = tiles[4 * i] == 64 && bk == 16;
            VQ_REQUIRE(tiles[4 * i + 3] == 2 && (bn == 32 || bn == 64) && (t16 || (tiles[4 * i] == 128 && bk == 8)) &&
                           (!t16 || net->plan.layers[i].op == VQ_OP_CONV_WINOGRAD16),
                       "layer %d: no Winograd variant for tile %dx%dx%d", i, tiles[4 * i], bn, bk);
            choice[i] = bn / 32 - 1 + (t16 ? 2 : 0);
            continue;
        }
        if (net->plan.layers[i].op != VQ_OP_CONV) continue;
        const int found = tile_index(tiles[4 * i], tiles[4 * i + 1], tiles[4 * i + 2], tiles[4 * i + 3]);
        VQ_REQUIRE(found >= 0, "layer %d: no kernel for tile %dx%dx%d pipe=%d", i, tiles[4 * i], tiles[4 * i + 1], tiles[4 * i + 2],
                   tiles[4 * i + 3]);
        choice[i] = found;
    }
    std::lock_guard<std::mutex> lk(net->mu);
    const int key = tile_key(n_crops, paired != 0);
    net->tuned[key] = choice;
    net->tuned_borrowed.erase(key);
    return VQ_OK;
}

// "The tiling of a forward of n_crops, however it runs": the one-stream table of that size and the paired tables of the sub-batch
// sizes the default forward cuts it into.
int vq_tsn_set_layer_tiles(vq_tsn* net, int32_t n_crops, const int32_t* tiles, int32_t n_layers) {
    int rc = vq_tsn_set_tiles(net, n_crops, 0, tiles, n_layers);
    if (rc != VQ_OK) return rc;
    const int parts_sum = net->parts_sum;
    if (net->n_split > 1 && parts_sum > 0 && n_crops % parts_sum == 0)
        for (int v : net->split_parts) {
            rc = vq_tsn_set_tiles(net, n_crops / parts_sum * v, 1, tiles, n_layers);
            if (rc != VQ_OK) return rc;
        }
    return VQ_OK;
}

int vq_tsn_flops_per_crop(vq_tsn* net, double* flops) {
    VQ_REQUIRE(net && flops, "NULL argument");
    *flops = net->plan.flops_per_crop;
    return VQ_OK;
}

}  // extern "C"
