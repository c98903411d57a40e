// The handle of a resident feature database (vq_db_*): what csrc/vq_sim.hip keeps per database, shared with the device loader of
// feature CSV files (csrc/vq_csv.hip), which stores into the handle's block under the handle's lock.
#pragma once
#include <mutex>
#include <vector>

#include "vq_common.h"

struct vq_db {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int S = 0, E = 0, D = 0, dtype = VQ_F32;
    int cus = 256;
    void* feats = nullptr;
    bool owns_feats = true;
    // VQ_LAYOUT_ROWS: [N][S][E][D].  VQ_LAYOUT_TILED (fp32, own memory): [tile of 16 clips][S*E][D/4][clip][4] in the SAME block (a
    // tile's 16 rows and its tiled form cover the same bytes; the block is allocated for whole tiles) -- vq_db_set_layout
    int layout = VQ_LAYOUT_ROWS;
    bool feats_exposed = false;      // adopted memory, or the raw pointer was handed out: the library no longer controls the layout
    uint8_t* present = nullptr;
    double* t = nullptr;        // [S*E*D]
    bool have_query = false, have_avg = false, have_scores = false, have_sims = false;
    double* w = nullptr;        // [8]
    double* sims = nullptr;     // lazily [N][S][E]
    double* avg = nullptr;      // [N][S]
    int32_t* ne = nullptr;      // [N][S]
    double* scores = nullptr;   // [N]
    // avg | ne | scores | sel_result | match prefix | near prefix are ONE device allocation (round_dev), in the order of the host
    // block of vq_db_query_round: a round's results go back in one copy
    char* round_dev = nullptr;
    int64_t round_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // byte offsets of avg, ne, scores, result, matchp, nearp; [6] = total
    int64_t* matchp = nullptr;       // first kRoundPrefix rows of the last selection's match list
    int64_t* nearp = nullptr;
    // selection scratch
    int nblk = 0;
    int2* blk_cnt = nullptr;
    double* blk_max = nullptr;
    int64_t* blk_arg = nullptr;
    int64_t* sel_result = nullptr;   // [3] device
    int64_t* rows0 = nullptr;        // [N]
    int64_t* rows1 = nullptr;        // [N]
    int64_t last_n0 = 0, last_n1 = 0;
    uint64_t* tk_state = nullptr;    // [2]
    unsigned int* tk_hist = nullptr; // [256]
    double* batch_buf = nullptr;     // batched scan: queries [Q][NV][D] | weights [Q][S] | (two-kernel form: sims [NV][Q][N]) | scores [Q][N]
    double* batch_scores = nullptr;  // where the scores of the last batched scan start inside batch_buf
    int64_t batch_cap = 0;           // doubles
    int batch_q = 0;                 // queries of the last batched scan
    // Batched rounds (vq_db_query_round_batch, include/vq_amd_rounds.h): ONE lazy allocation that starts with the image of the host
    // block (queries | weights | bands | n_e | avg | scores | results | prefixes: what comes and goes in one copy each way) followed by
    // the full match / near lists [Q][N] each and the per-block scratch of the three-pass selection.
    char* bround_dev = nullptr;
    int64_t bround_cap = 0;          // bytes
    int bround_q = 0;                // queries of the last batched round (0: none, or its lists are gone)
    int64_t bround_rows0 = 0, bround_rows1 = 0;      // byte offsets of the full lists of the last round
    int64_t bround_n0[16] = {0}, bround_n1[16] = {0};  // its counts per query (-1: that round did not partition)
    hipEvent_t bround_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // flag 8: start | pass done | selection done | copies done
    bool bround_timed = false;
    int64_t bround_qoff[16] = {0};   // where query q's full lists start inside the two list arrays (entries): q N, or a view round's start[q]
    // The layout of the last batched round, for the calls of include/vq_amd_round_fit.h that work on its device data: the offsets of
    // its block, the rows per query (bround_qoff[q] is also where query q's avg / scores entries start), whether it was a view
    // round, and where the scratch of the three-pass selection sits (query q's blocks start at bround_bstart[q]; none for a piece
    // of at most kSelSmallN rows).
    int64_t bround_off[12] = {0};
    int64_t bround_m[16] = {0};
    bool bround_views = false;
    int64_t bround_cnt = 0, bround_max = 0, bround_arg = 0;     // byte offsets of blk_cnt, blk_max, blk_arg
    int32_t bround_bstart[17] = {0};
    // View rounds (vq_db_query_round_views, include/vq_amd_round_views.h): the plan's device block, allocated on the first one --
    // inv [16][stride] i32 | union rows [stride + 16] i32 | touched tiles [stride / 16] i32 | counts [2] i64 | start [17] i64 | the
    // per-block counts of the compaction [tiles / 256] int2 -- and what the last one covered
    char* vround_plan = nullptr;
    bool vround_have = false;
    int64_t vround_union = 0, vround_tiles = 0;
    double* grid_buf = nullptr;      // scratch for grid / gathers
    int64_t grid_cap = 0;
    // Batched targets (vq_db_batch_targets, include/vq_amd_round_targets.h; csrc/vq_round_targets.hip): the image of the call's block |
    // the pools' Gram matrices | the coefficients of every draw | a status per (draw, slot), and the scratch area of the draws whose
    // systems do not fit into local memory.  Both grow on demand and go with the handle.
    char* targets_buf = nullptr;
    int64_t targets_cap = 0;         // bytes
    double* targets_ws = nullptr;
    int64_t targets_ws_cap = 0;      // bytes
    // Batched top-k (vq_db_batch_round_topk, include/vq_amd_round_topk.h; csrc/vq_round_topk.hip): the image of the call's block | the
    // survivors of the long pieces | the state and the histograms of the eight radix passes | the block counts of the compaction.
    // Allocated by the first call, grows on demand, goes with the handle.
    char* btopk_buf = nullptr;
    int64_t btopk_cap = 0;           // bytes
    // Row views (vq_db_rows_define): resident index lists, one device block each.  `active` is the view the one-query path runs over
    // (-1: the whole database) and `na` the number of clips it then covers -- M, or N: what every result-side entry point counts with.
    struct RowView {
        bool defined = false;
        int64_t m = 0;               // rows in the view
        int64_t ntiles = 0;          // tiles of 16 clips it touches (fp32 databases of a tiled-capable shape; else no tile tables)
        int64_t* rows = nullptr;     // [m] | tiles [ntiles] | pos [ntiles][16]: ONE allocation, rows first
        int64_t* tiles = nullptr;
        int64_t* pos = nullptr;
    };
    std::vector<RowView> views;
    int active = -1;
    int64_t na = 0;
    size_t elem() const { return dtype == VQ_F64 ? 8 : dtype == VQ_F16 ? 2 : 4; }
};

namespace vq {

// csrc/vq_sim.hip: rows (by number) -> a dense row-major [L][S][E][D] block in the handle's gather scratch, whatever the layout; the
// caller holds the handle's lock and has its device current.  rows_dev: the same L row numbers already on the device (ordered on the
// handle's stream) -- they are then read there and nothing is uploaded.  Shared with csrc/vq_round_targets.hip.
int gather_rows_device(vq_db* db, const int64_t* rows_host, int L, const void** dense, const int64_t* rows_dev = nullptr);

}  // namespace vq
