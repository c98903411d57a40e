// The decisions of the TSN executor that need no GPU (see vq_tsn_plan.h).
//
// Host-only translation unit (no HIP): also built by tests/sanitize/Makefile with -fsanitize=address,undefined.
#include "vq_tsn_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define VQ_REQUIRE(cond, ...)                                            \
    do {                                                                 \
        if (!(cond)) return ::vq::host_fail(VQ_E_INVALID, __VA_ARGS__); \
    } while (0)

namespace vq {

int validate_plan(const vq_tensor_desc* tensors, int32_t n_tensors, const vq_layer_desc* layers, int32_t n_layers,
                  const vq_conv_segment* segments, int32_t n_segments, const float* blob_host, int64_t blob_floats,
                  const vq_input_desc* input, int32_t feature_slot, int32_t max_crops, TsnPlan* plan) {
    VQ_REQUIRE(tensors && layers && blob_host && input, "NULL argument");
    const int in_channels = input->c;
    VQ_REQUIRE(n_tensors > 0 && n_layers > 0 && blob_floats > 0 && max_crops > 0, "sizes must be positive");
    VQ_REQUIRE(n_segments >= 0 && (n_segments == 0 || segments), "bad segment table");
    VQ_REQUIRE(feature_slot > 0 && feature_slot < n_tensors, "feature_slot out of range");
    VQ_REQUIRE(tensors[feature_slot].h == 1 && tensors[feature_slot].w == 1, "feature slot must be 1x1xD");
    VQ_REQUIRE(tensors[0].c % 4 == 0, "input slot channels must be padded to a multiple of 4 (got %d)", tensors[0].c);
    VQ_REQUIRE(input->h > 0 && input->w > 0 && in_channels > 0, "input crops must be h x w x c with positive sizes");
    if (input->s2d_pad < 0) {
        VQ_REQUIRE(tensors[0].h == input->h && tensors[0].w == input->w, "input slot is %dx%d but the crops are %dx%d", tensors[0].h,
                   tensors[0].w, input->h, input->w);
        VQ_REQUIRE(in_channels <= tensors[0].c && tensors[0].c - in_channels < 4, "in_channels %d does not fit the %d-channel input slot",
                   in_channels, tensors[0].c);
    } else {
        VQ_REQUIRE(tensors[0].c == 4 * in_channels, "space-to-depth input slot needs 4 x %d channels (got %d)", in_channels, tensors[0].c);
        VQ_REQUIRE(input->s2d_pad <= 64, "space-to-depth shift out of range");
        VQ_REQUIRE(input->s2d_order == 0 || input->s2d_order == 1, "s2d_order must be 0 or 1");
    }
    // validate every layer against the tensor table BEFORE anything is launched: a mismatch here would be
    // an out-of-bounds access on the device
    double macs = 0;
    for (int i = 0; i < n_layers; ++i) {
        const vq_layer_desc& L = layers[i];
        const bool multi = L.op == VQ_OP_CONV && L.seg_count > 0;
        VQ_REQUIRE(L.src >= 0 && L.src < n_tensors && L.dst > 0 && L.dst < n_tensors && L.src != L.dst,
                   "layer %d: bad tensor slots %d -> %d", i, L.src, L.dst);
        const vq_tensor_desc& ts = tensors[L.src];
        const vq_tensor_desc& td = tensors[L.dst];
        // one crop of any slot must stay addressable with a signed 32-bit byte offset (the kernels' buffer offsets);
        // larger batches are cut into crop ranges per launch (LaunchItem::max_crops)
        VQ_REQUIRE((size_t)ts.h * ts.w * ts.c * sizeof(float) <= 0x7FFFFFF0u && (size_t)td.h * td.w * td.c * sizeof(float) <= 0x7FFFFFF0u,
                   "layer %d: one crop of a tensor slot exceeds 2 GiB", i);
        VQ_REQUIRE(L.src_coff >= 0 && L.cin > 0 && L.src_coff + L.cin <= ts.c, "layer %d: reads channels [%d,%d) of a %d-channel slot",
                   i, L.src_coff, L.src_coff + L.cin, ts.c);
        VQ_REQUIRE(multi || (L.dst_coff >= 0 && L.cout > 0 && L.dst_coff + L.cout <= td.c),
                   "layer %d: writes channels [%d,%d) of a %d-channel slot", i, L.dst_coff, L.dst_coff + L.cout, td.c);
        if (multi) {
            VQ_REQUIRE(L.seg_first >= 0 && L.seg_first + L.seg_count <= n_segments, "layer %d: segments outside the table", i);
            int sum = 0;
            for (int q = 0; q < L.seg_count; ++q) {
                const vq_conv_segment& sg = segments[L.seg_first + q];
                VQ_REQUIRE(sg.dst > 0 && sg.dst < n_tensors && sg.dst != L.src, "layer %d segment %d: bad slot", i, q);
                const vq_tensor_desc& t2 = tensors[sg.dst];
                VQ_REQUIRE(sg.cout > 0 && sg.cout % 32 == 0 && sg.dst_coff >= 0 && sg.dst_coff % 4 == 0 && sg.dst_coff + sg.cout <= t2.c,
                           "layer %d segment %d: channels [%d,%d) do not fit a %d-channel slot (cout must be a multiple of 32)", i, q,
                           sg.dst_coff, sg.dst_coff + sg.cout, t2.c);
                VQ_REQUIRE(t2.h == td.h && t2.w == td.w && t2.c % 4 == 0, "layer %d segment %d: spatial size differs", i, q);
                sum += sg.cout;
            }
            VQ_REQUIRE(sum == L.cout, "layer %d: segments cover %d of %d output channels", i, sum, L.cout);
        }
        VQ_REQUIRE(L.k >= 1 && L.stride >= 1 && L.pad >= 0 && L.pad < L.k, "layer %d: bad kernel/stride/pad", i);
        // (an InnerProduct writes single floats: its destination slot, cout and dst_coff are free -- 101 class scores)
        const bool fc = L.op == VQ_OP_INNER_PRODUCT;
        VQ_REQUIRE(ts.c % 4 == 0 && L.src_coff % 4 == 0 && L.cin % 4 == 0 && (fc || (td.c % 4 == 0 && L.dst_coff % 4 == 0 && L.cout % 4 == 0)),
                   "layer %d: channel counts and offsets must be multiples of 4", i);
        if (L.op == VQ_OP_CONV) {
            VQ_REQUIRE(L.k <= 8, "layer %d: conv kernels up to 8x8 (the tap mask is 64 bits)", i);
            if (L.pre_pool_k > 0) {
                VQ_REQUIRE(L.pre_pool_k == 3 && L.pre_pool_stride >= 1 && L.pre_pool_stride <= 3,
                           "layer %d: the pooled-input form takes a 3x3 max window with stride 1..3", i);
                VQ_REQUIRE(L.k == 1 && L.stride == 1 && L.pad == 0 && L.cin % 32 == 0, "layer %d: the pooled-input form is a 1x1 convolution over a multiple of 32 channels", i);
                VQ_REQUIRE(td.h == pool_out_size(ts.h, 3, L.pre_pool_stride, 0) && td.w == pool_out_size(ts.w, 3, L.pre_pool_stride, 0),
                           "layer %d: pooled-input size mismatch (Caffe ceil rule)", i);
            } else
            VQ_REQUIRE(td.h == (ts.h + 2 * L.pad - L.k) / L.stride + 1 && td.w == (ts.w + 2 * L.pad - L.k) / L.stride + 1,
                       "layer %d: conv output size mismatch", i);
            int64_t kp = (int64_t)(L.k * L.k * L.cin + KPAD - 1) / KPAD * KPAD;
            if (L.src == 0 && input->s2d_pad >= 0 && input->s2d_order == 1) {      // x-major stem: [Cout][steps][4][4], see launch_conv_layer
                VQ_REQUIRE(L.k == 4 && L.cin == 4 * in_channels && L.stride == 1 && L.pad == 0 && L.src_coff == 0 && L.pre_pool_k == 0 &&
                               L.seg_count == 0 && input->s2d_kernel == 7,
                           "layer %d: the x-major space-to-depth stem is a 7x7 / stride-2 convolution reading the whole input slot", i);
                kp = stem_rows_kp(in_channels);
            }
            VQ_REQUIRE(L.w_off >= 0 && L.w_off % 4 == 0 && L.w_off + (int64_t)L.cout * kp <= blob_floats,
                       "layer %d: weights outside the blob", i);
            VQ_REQUIRE(L.b_off >= 0 && L.b_off + L.cout <= blob_floats, "layer %d: bias outside the blob", i);
            VQ_REQUIRE(L.cin % KPAD == 0 || L.src_coff == 0, "layer %d: small-Cin convolution must read a whole slot", i);
            VQ_REQUIRE(L.cin % KPAD == 0 || L.cin == ts.c, "layer %d: small-Cin convolution must read a whole slot", i);
            macs += (double)td.h * td.w * L.cout * first_layer_k2c(*input, L);   // algorithmic, un-padded
        } else if (is_wino(L.op)) {
            VQ_REQUIRE(L.k == 3 && L.stride == 1 && L.pad == 1 && L.seg_count == 0, "layer %d: Winograd form is 3x3 / stride 1 / pad 1, one destination", i);
            VQ_REQUIRE(L.cin % (L.op == VQ_OP_CONV_WINOGRAD16 ? 16 : 8) == 0 && L.cout % 32 == 0,
                       "layer %d: Winograd form needs Cin %% 8 == 0 (16-tile units: %% 16) and Cout %% 32 == 0", i);
            VQ_REQUIRE(td.h == ts.h && td.w == ts.w, "layer %d: conv output size mismatch", i);
            VQ_REQUIRE(L.w_off >= 0 && L.w_off % 4 == 0 &&
                           L.w_off + (int64_t)(L.op == VQ_OP_CONV_WINOGRAD16 ? 2 : 1) * 16 * L.cout * L.cin <= blob_floats,
                       "layer %d: transformed filters outside the blob", i);
            VQ_REQUIRE(L.b_off >= 0 && L.b_off % 4 == 0 && L.b_off + L.cout <= blob_floats, "layer %d: bias outside the blob", i);
            macs += (double)td.h * td.w * L.cout * L.cin * 9;   // algorithmic (direct-form) count
        } else if (L.op == VQ_OP_MAXPOOL || L.op == VQ_OP_AVGPOOL) {
            VQ_REQUIRE(L.cin == L.cout, "layer %d: pooling keeps the channel count", i);
            VQ_REQUIRE(!(L.op == VQ_OP_AVGPOOL && L.has_bias) || (L.b_off >= 0 && L.b_off % 4 == 0 && L.b_off + L.cout <= blob_floats),
                       "layer %d: pooling bias outside the blob", i);
            VQ_REQUIRE(td.h == pool_out_size(ts.h, L.k, L.stride, L.pad) && td.w == pool_out_size(ts.w, L.k, L.stride, L.pad),
                       "layer %d: pooling output size mismatch (Caffe ceil rule)", i);
        } else if (L.op == VQ_OP_GLOBAL_AVGPOOL) {
            VQ_REQUIRE(L.cin == L.cout && td.h == 1 && td.w == 1, "layer %d: global pool must write a 1x1 slot", i);
        } else if (L.op == VQ_OP_INNER_PRODUCT) {
            VQ_REQUIRE(ts.h == 1 && ts.w == 1 && td.h == 1 && td.w == 1, "layer %d: InnerProduct reads and writes 1x1 slots", i);
            VQ_REQUIRE(L.seg_count == 0 && L.pre_pool_k == 0 && L.relu == 0, "layer %d: InnerProduct has one destination, no pooled input, no ReLU", i);
            VQ_REQUIRE(L.has_bias == 1, "layer %d: InnerProduct always adds its bias: has_bias must be 1 and b_off address it", i);
            VQ_REQUIRE(L.w_off >= 0 && L.w_off % 4 == 0 && L.w_off + (int64_t)L.cout * L.cin <= blob_floats, "layer %d: weights outside the blob", i);
            VQ_REQUIRE(L.b_off >= 0 && L.b_off + L.cout <= blob_floats, "layer %d: bias outside the blob", i);
            VQ_REQUIRE(L.cout <= 65535 * FC_COLS, "layer %d: InnerProduct with more than %d outputs", i, 65535 * FC_COLS);
            macs += (double)L.cin * L.cout;
        } else {
            return host_fail(VQ_E_INVALID, "layer %d: unknown op %d", i, L.op);
        }
    }
    plan->input = *input;
    plan->tensors.assign(tensors, tensors + n_tensors);
    plan->layers.assign(layers, layers + n_layers);
    plan->segments.clear();
    if (n_segments > 0) plan->segments.assign(segments, segments + n_segments);
    plan->D = tensors[feature_slot].c;
    plan->flops_per_crop = 2.0 * macs;
    plan->consensus_layer = -1;
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].op == VQ_OP_GLOBAL_AVGPOOL && layers[i].dst == feature_slot && layers[i].dst_coff == 0 && layers[i].cout == plan->D)
            plan->consensus_layer = i;
    return VQ_OK;
}

namespace {
// Channel range of one slot that a layer reads or writes.
struct SlotRange {
    int slot, c0, c1;
};
bool overlaps(const std::vector<SlotRange>& x, const std::vector<SlotRange>& y) {
    for (const SlotRange& p : x)
        for (const SlotRange& q : y)
            if (p.slot == q.slot && p.c0 < q.c1 && q.c0 < p.c1) return true;
    return false;
}

// The launch sequence.  Layer i depends on an earlier layer j when i reads what j wrote, overwrites what j read, or
// writes the same channels (slots are never recycled, so in a valid plan only the first kind occurs, but all three are
// honoured).  Layers are levelled (level = 1 + deepest dependency) and launched level by level, which is a topological
// order; inside a level every layer is independent of every other, so the level's Winograd convolutions -- the 3x3 and
// the first double-3x3 arm of an inception module -- share ONE launch (vq_wino.hip).
}  // namespace

void build_items(TsnPlan& plan, bool group_wino, bool group_pool) {
    const int n = (int)plan.layers.size();
    std::vector<std::vector<SlotRange>> rd(n), wr(n);
    for (int i = 0; i < n; ++i) {
        const vq_layer_desc& L = plan.layers[i];
        const bool whole = L.op == VQ_OP_CONV && L.cin % KPAD != 0;
        rd[i].push_back(whole ? SlotRange{L.src, 0, plan.tensors[L.src].c} : SlotRange{L.src, L.src_coff, L.src_coff + L.cin});
        if (L.op == VQ_OP_CONV && L.seg_count > 0)
            for (int q = 0; q < L.seg_count; ++q) {
                const vq_conv_segment& sg = plan.segments[L.seg_first + q];
                wr[i].push_back(SlotRange{sg.dst, sg.dst_coff, sg.dst_coff + sg.cout});
            }
        else
            wr[i].push_back(SlotRange{L.dst, L.dst_coff, L.dst_coff + L.cout});
    }
    std::vector<int> level(n, 0), floor_level(n, 0);
    int n_levels = 0;
    auto levelise = [&]() {
        n_levels = 0;
        for (int i = 0; i < n; ++i) {
            level[i] = floor_level[i];
            for (int j = 0; j < i; ++j)
                if (overlaps(wr[j], rd[i]) || overlaps(rd[j], wr[i]) || overlaps(wr[j], wr[i])) level[i] = std::max(level[i], level[j] + 1);
            n_levels = std::max(n_levels, level[i] + 1);
        }
    };
    levelise();
    // A pooling layer that reads a module's input is ready one level before the module's Winograd convolutions (it sits
    // beside the 1x1 reductions).  Nothing needs it that early: hold it back one level so it can ride in their launch.
    if (group_wino && group_pool) {
        for (int i = 0; i < n; ++i) {
            const int op = plan.layers[i].op;
            if (op != VQ_OP_MAXPOOL && op != VQ_OP_AVGPOOL) continue;
            bool here = false, next = false;
            for (int j = 0; j < n; ++j)
                if (is_wino(plan.layers[j].op)) {
                    here |= level[j] == level[i];
                    next |= level[j] == level[i] + 1;
                }
            if (!here && next) floor_level[i] = level[i] + 1;
        }
        levelise();
    }
    auto slot_bytes_per_crop = [&](int slot) {
        const vq_tensor_desc& t = plan.tensors[slot];
        return (size_t)t.h * t.w * t.c * sizeof(float);
    };
    auto item_limit = [&](const std::vector<int>& members) {
        size_t worst = 1;
        for (int li : members) {
            const vq_layer_desc& L = plan.layers[li];
            worst = std::max(worst, slot_bytes_per_crop(L.src));
            if (L.op == VQ_OP_CONV && L.seg_count > 0)
                for (int q = 0; q < L.seg_count; ++q) worst = std::max(worst, slot_bytes_per_crop(plan.segments[L.seg_first + q].dst));
            else
                worst = std::max(worst, slot_bytes_per_crop(L.dst));
        }
        size_t limit = std::max<size_t>(1, (size_t)0x7FFFFFF0u / worst);
        // the Winograd kernel multiplies pixel indices of a slot on 24 bits (vq_wino.hip: launch_t requires crops x H x W < 2^23 for the
        // source AND the destination): with >= 64 channels per pixel the byte limit above implies it, a narrower slot at a large batch
        // needs the cap itself (the launch then covers the batch in several crop ranges, like any other item)
        for (int li : members) {
            const vq_layer_desc& L = plan.layers[li];
            if (!is_wino(L.op)) continue;
            for (int slot : {L.src, L.dst}) {
                const vq_tensor_desc& t = plan.tensors[slot];
                limit = std::min(limit, std::max<size_t>(1, ((size_t)(1u << 23) - 1) / ((size_t)t.h * t.w)));
            }
            // ... and decodes a workgroup's first tile with a multiply-high division that is exact while (tiles + 32) x tiles per image < 2^32
            const vq_tensor_desc& ts = plan.tensors[L.src];
            const size_t tpi = (size_t)((ts.h + 1) / 2) * ((ts.w + 1) / 2);
            if ((1ull << 32) / tpi > 64) limit = std::min(limit, std::max<size_t>(1, ((size_t)((1ull << 32) / tpi) - 64) / tpi));
        }
        return (int)limit;
    };
    plan.items.clear();
    plan.item_of_layer.assign(n, -1);
    for (int lv = 0; lv < n_levels; ++lv) {
        std::vector<int> wino, pools;
        for (int i = 0; i < n; ++i)
            if (level[i] == lv && is_wino(plan.layers[i].op) && group_wino) wino.push_back(i);
        for (int i = 0; i < n; ++i) {
            if (level[i] != lv || (is_wino(plan.layers[i].op) && group_wino)) continue;
            const int op = plan.layers[i].op;
            // the level's pooling rides in its Winograd launch (few short workgroups that fill the tail)
            if (!wino.empty() && (op == VQ_OP_MAXPOOL || op == VQ_OP_AVGPOOL) && (int)pools.size() < kWinoMaxPools && group_pool) {
                pools.push_back(i);
                continue;
            }
            LaunchItem it;
            it.kind = 0;
            it.layers = {i};
            it.max_crops = item_limit(it.layers);
            plan.item_of_layer[i] = (int)plan.items.size();
            plan.items.push_back(it);
        }
        // longest K loop first: the hardware hands out workgroups in index order, so the short ones fill the tail
        // (a launch carries layers of one filter layout: the 32-tile form first, then the 16-tile form; a level of BN-Inception has one)
        std::stable_sort(wino.begin(), wino.end(), [&](int x, int y) {
            if (plan.layers[x].op != plan.layers[y].op) return plan.layers[x].op < plan.layers[y].op;
            return plan.layers[x].cin > plan.layers[y].cin;
        });
        for (size_t q = 0; q < wino.size();) {
            size_t end = q;
            while (end < wino.size() && end - q < (size_t)kWinoMaxJobs && plan.layers[wino[end]].op == plan.layers[wino[q]].op) ++end;
            LaunchItem it;
            it.kind = 1;
            it.layers.assign(wino.begin() + q, wino.begin() + end);
            const bool first = q == 0;
            q = end;
            if (first) it.layers.insert(it.layers.end(), pools.begin(), pools.end());
            it.max_crops = item_limit(it.layers);
            for (int m : it.layers) plan.item_of_layer[m] = (int)plan.items.size();
            plan.items.push_back(it);
        }
    }
}

// Which direct convolutions run split over K: single-destination layers with aligned channels on maps of at most
// 7 x 7 (M = 49 x crops: at any usual batch fewer output tiles than the chip has room for, each a long serial K chain
// on one wave per SIMD), cut into slices of at least 16 K-steps of 32 -- at most 4 slices.  On the 14 x 14 maps the
// same cut LOSES (3c/3x3 0.058 -> 0.076 ms at 96 crops: enough tiles already, the scratch round trip costs more).
// A function of the layer alone -- never of the batch actually run -- so a crop's features do not depend on the batch
// it travels in.  VQ_TSN_SPLITK=0 turns it off (A/B measurements).
void choose_ksplit(TsnPlan& plan, bool enabled) {
    const int n_layers = (int)plan.layers.size();
    plan.ksplit.assign(n_layers, 1);
    size_t scratch = 0;
    int max_cout = 4;
    for (int i = 0; i < n_layers && enabled; ++i) {
        const vq_layer_desc& L = plan.layers[i];
        const vq_tensor_desc& td = plan.tensors[L.dst];
        if (L.op != VQ_OP_CONV || L.seg_count > 0 || L.pre_pool_k > 0 || L.cin % KPAD != 0 || td.h * td.w > 49) continue;
        const int steps = L.k * L.k * L.cin / KPAD;
        int ks = std::min(4, steps / 16);
        while (ks > 1 && steps % ks != 0) --ks;
        if (ks <= 1) continue;
        plan.ksplit[i] = ks;
        scratch = std::max(scratch, (size_t)td.h * td.w * L.cout);
        max_cout = std::max(max_cout, L.cout);
    }
    plan.max_cout = max_cout;
    plan.split_crop_floats = scratch > 0 ? scratch + (size_t)max_cout : 0;
}

BatchCut cut_batch(const TsnPlan& plan, int n_crops, int T, const std::vector<int>& split_parts, int parts_sum, bool one_stream) {
    const int n_split = (!one_stream && split_parts.size() > 1 && n_crops % parts_sum == 0) ? (int)split_parts.size() : 1;
    BatchCut cut;
    cut.sub.assign(n_split, n_crops);
    cut.sub_off.assign(n_split, 0);
    if (n_split > 1) {
        for (int sb = 0, o = 0; sb < n_split; ++sb) {
            cut.sub[sb] = n_crops / parts_sum * split_parts[sb];
            cut.sub_off[sb] = o;
            o += cut.sub[sb];
        }
    }
    // the consensus rides in the global-pool launch when every launch of that layer covers whole clips
    bool whole = plan.consensus_layer >= 0 && T <= kMaxFusedT;
    if (whole) {
        const int cap = plan.items[plan.item_of_layer[plan.consensus_layer]].max_crops;
        for (int sb = 0; sb < n_split; ++sb)
            if (cut.sub[sb] % T != 0 || cut.sub_off[sb] % T != 0 || (cut.sub[sb] > cap && cap % T != 0)) whole = false;
    }
    cut.fused_consensus = whole;
    return cut;
}

TsnOptions parse_tsn_options(const char* autotune, const char* group, const char* group_pool, const char* poison, const char* tile,
                             const char* split, const char* splitk) {
    TsnOptions o;
    if (autotune) o.autotune = atoi(autotune) != 0;
    if (group) o.group_wino = atoi(group) != 0;
    if (group_pool) o.group_pool = atoi(group_pool) != 0;
    if (poison) o.poison = atoi(poison) != 0;
    if (splitk) o.splitk = atoi(splitk) != 0;
    if (tile) o.tile_set = sscanf(tile, "%dx%dx%dx%d", &o.tile[0], &o.tile[1], &o.tile[2], &o.tile[3]) >= 2;
    if (split && strchr(split, ',')) {
        o.split_parts.clear();
        for (const char* q = split; *q;) {
            o.split_parts.push_back(std::max(atoi(q), 1));
            q = strchr(q, ',');
            if (!q) break;
            ++q;
        }
        o.n_split = std::min<int>((int)o.split_parts.size(), 8);
        o.split_parts.resize(o.n_split);
    } else {
        o.n_split = std::min(std::max(split ? atoi(split) : 2, 1), 8);
        o.split_parts.assign(o.n_split, 1);
    }
    return o;
}

TsnOptions tsn_options_from_env() {
    return parse_tsn_options(getenv("VQ_TSN_AUTOTUNE"), getenv("VQ_TSN_GROUP"), getenv("VQ_TSN_GROUP_POOL"), getenv("VQ_TSN_POISON"),
                             getenv("VQ_TSN_TILE"), getenv("VQ_TSN_SPLIT"), getenv("VQ_TSN_SPLITK"));
}

int nearest_size(const std::vector<int>& sizes, int n_crops) {
    int nearest = 0;
    for (int size : sizes) {
        if (10 * std::max(size, n_crops) > 16 * std::min(size, n_crops)) continue;            // further than 1.6x away
        if (nearest == 0 || std::abs(size - n_crops) < std::abs(nearest - n_crops)) nearest = size;
    }
    return nearest;
}

}  // namespace vq
