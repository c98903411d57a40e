// What the TSN executor (csrc/vq_tsn.hip) decides without touching the GPU: the validation of a layer plan against its tensor table,
// the launch sequence, which convolutions run split over K, how a batch is cut into sub-batches, and which tuned batch size stands in
// for another, and the creation-time switches of the environment.  Host-only translation unit (no HIP include), so that tests/sanitize/san_driver.cc can drive every check of it under
// the sanitizers; the constants both sides need live here once (csrc/vq_tsn_kernels.h includes this header for them).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vq_amd.h"
#include "vq_host.h"

namespace vq {

constexpr int KPAD = 32;           // weights are packed [Cout][Kp] with Kp a multiple of 32
constexpr int FC_COLS = 8;         // outputs per wave of inner_product_kernel (a grid row of 65535 workgroups at most)
constexpr int kMaxFusedT = 16;     // gavgpool_consensus_kernel: clips of up to this many snippets
constexpr int kWinoMaxJobs = 4;
// Independent layers of one graph level (the 3x3 and the first double-3x3 arm of an inception module, and the module's
// pooling arm) as ONE launch: their workgroups fill each other's tail rounds and kernel boundaries disappear.
constexpr int kWinoMaxPools = 2;

// ... except the x-major space-to-depth stem (7x7 / stride 2 over c channels): four kernel rows of 7 x-taps x 2 rows x c floats each,
// every row padded to whole 16-byte chunks, walked side by side (csrc/vq_tsn.hip: launch_conv_layer)
inline int stem_rows_kp(int c) { return 4 * ((14 * c + 3) / 4 * 4); }

// k*k*Cin of a convolution in ALGORITHMIC terms: a layer that reads slot 0 counts the un-padded input channels and,
// in space-to-depth form, the kernel size of the original convolution.
inline double first_layer_k2c(const vq_input_desc& in, const vq_layer_desc& L) {
    if (L.src != 0) return (double)L.k * L.k * L.cin;
    const int k = (in.s2d_pad >= 0 && in.s2d_kernel > 0) ? in.s2d_kernel : L.k;
    return (double)k * k * in.c;
}

inline bool is_wino(int op) { return op == VQ_OP_CONV_WINOGRAD || op == VQ_OP_CONV_WINOGRAD16; }
inline bool is_conv(int op) { return op == VQ_OP_CONV || is_wino(op); }

inline int pool_out_size(int size, int k, int s, int p) {
    int out = (size + 2 * p - k + s - 1) / s + 1;
    if (p > 0 && (out - 1) * s >= size + p) --out;
    return out;
}

// One kernel launch of a forward: a single layer, or the Winograd convolutions of one graph level together.
struct LaunchItem {
    int kind = 0;              // 0 = one layer, 1 = Winograd group
    std::vector<int> layers;   // kind 1: longest K loop first (its workgroups are dispatched first; the short ones fill the tail)
    int max_crops = 0;         // crops one launch may cover: every slot it touches stays below 2^31 bytes (32-bit offsets)
};

struct TsnPlan {
    vq_input_desc input = {0, 0, 0, -1, 0, 0};
    std::vector<vq_tensor_desc> tensors;
    std::vector<vq_layer_desc> layers;
    std::vector<vq_conv_segment> segments;
    std::vector<LaunchItem> items;        // the launch sequence (a topological order of the layer graph by levels)
    std::vector<int> item_of_layer;
    std::vector<int> ksplit;              // per layer: K slices of a direct convolution (1 = not split; layer geometry only)
    size_t split_crop_floats = 0;         // scratch floats one crop owns per slice: largest Ho*Wo*Cout of a split layer + one row of slack
    int max_cout = 4;                     // widest split layer (the zero bias of the slices' epilogues)
    int consensus_layer = -1;             // the global-pool layer that writes the feature slot: runs fused with the consensus
    double flops_per_crop = 0;
    int D = 0;                            // channels of the feature slot
};

// Validate every layer against the tensor table BEFORE anything is launched (a mismatch would be an out-of-bounds access on the
// device) and fill plan's tensors, layers, segments, input, D, flops_per_crop and consensus_layer.  VQ_E_INVALID with the message in
// vq_last_error() otherwise.
int validate_plan(const vq_tensor_desc* tensors, int32_t n_tensors, const vq_layer_desc* layers, int32_t n_layers,
                  const vq_conv_segment* segments, int32_t n_segments, const float* blob_host, int64_t blob_floats,
                  const vq_input_desc* input, int32_t feature_slot, int32_t max_crops, TsnPlan* plan);
constexpr int kValidatePlanRequires = 49;   // `require` sites of validate_plan, the unknown-op exit included (san_driver: one mutation each)

// plan.items / plan.item_of_layer: the launch sequence, level by level.
void build_items(TsnPlan& plan, bool group_wino, bool group_pool);

// plan.ksplit, plan.split_crop_floats, plan.max_cout: which direct convolutions run split over K (none when !enabled).
void choose_ksplit(TsnPlan& plan, bool enabled);

// The switches vq_tsn_create reads from the environment, parsed once (include/vq_amd.h documents them).
struct TsnOptions {
    bool autotune = true;          // VQ_TSN_AUTOTUNE != 0
    bool group_wino = true;        // VQ_TSN_GROUP != 0: independent Winograd layers share a launch
    bool group_pool = true;        // VQ_TSN_GROUP_POOL != 0: a level's pooling rides in its Winograd launch
    bool poison = false;           // VQ_TSN_POISON != 0: NaN-fill every activation slot before a forward
    bool splitk = true;            // VQ_TSN_SPLITK != 0: the 7 x 7 layers run split over K (choose_ksplit)
    bool tile_set = false;         // VQ_TSN_TILE = "BMxBN[xBK[xP]]" (P = 1: pipelined kernel) gave at least BM and BN:
    int tile[4] = {0, 0, 32, 0};   // ... [bm, bn, bk, pipe], which the executor resolves with tile_index
    int n_split = 2;               // VQ_TSN_SPLIT = "n": n equal sub-batches (1 .. 8), or "a,b,..": up to 8 sub-batches of these
    std::vector<int> split_parts = {1, 1};   // relative sizes ("2,1": 2/3 and 1/3 of the crops; an entry below 1 counts as 1)
};
// From the values of the seven variables, each null when unset
TsnOptions parse_tsn_options(const char* autotune, const char* group, const char* group_pool, const char* poison, const char* tile,
                             const char* split, const char* splitk);
TsnOptions tsn_options_from_env();

inline int parts_sum(const std::vector<int>& split_parts) {
    int sum = 0;
    for (int v : split_parts) sum += v;
    return sum;
}

// The sub-batches of one forward (one entry, the whole batch, when it runs in one piece) and whether the consensus rides in
// the global-pool launch.
struct BatchCut {
    std::vector<int> sub, sub_off;
    bool fused_consensus = false;
};
BatchCut cut_batch(const TsnPlan& plan, int n_crops, int T, const std::vector<int>& split_parts, int parts_sum, bool one_stream);

// The member of `sizes` closest to n_crops among those within 1.6x of it (the first of equals); 0: none.
int nearest_size(const std::vector<int>& sizes, int n_crops);

}  // namespace vq
