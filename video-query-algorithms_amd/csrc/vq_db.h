// The handle of a resident feature database (vq_db_*): what csrc/vq_db.hip keeps per database, shared with the scans
// (csrc/vq_sim.hip, csrc/vq_sim_batch.hip), the ranking (csrc/vq_rank.hip), the device loader of feature CSV files (csrc/vq_csv.hip),
// which stores into the handle's block under the handle's lock, and the units of the batched rounds (csrc/vq_rounds.hip,
// csrc/vq_round_targets.hip, csrc/vq_round_topk.hip).  Every device block is held by an owner (vq_common.h): the handle has no free
// function and is deleted with its device current.  The plain pointers next to the owners point INTO one of them.
#pragma once
#include <mutex>
#include <type_traits>
#include <vector>

#include "vq_common.h"
#include "vq_tile_index.h"

constexpr int kBatchSlots = 16;            // queries of a batched scan or round
constexpr int64_t kRoundPrefix = 1024;     // rows of each list that a round copies back next to the counts

// The pieces of a batched round, for every kind of round: what a round is laid out by and what the handle remembers of the last one.
// Query q's avg / scores / list entries are start[q] .. start[q + 1] of the concatenated pieces (a whole-database round: q N on);
// the entries behind the last query repeat its end.  A piece of more than kSelSmallN entries has blocks bstart[q] .. bstart[q + 1] of the three-pass
// selection's scratch, a shorter one has none.
struct BatchRound {
    int q = 0;                       // queries (0 on the handle: no round yet, or its lists are gone)
    bool views = false, timed = false;
    int64_t off[12] = {0};           // the host block: include/vq_amd_rounds.h, include/vq_amd_round_views.h
    int64_t start[17] = {0};
    int32_t bstart[17] = {0};
    int64_t n0[16] = {0}, n1[16] = {0};      // the counts of the last partition per query (-1: that round did not partition)
    int64_t rows0 = 0, rows1 = 0;    // byte offsets behind the image of the host block: the full match and near lists ...
    int64_t cnt = 0, max = 0, arg = 0;       // ... and blk_cnt | blk_max | blk_arg
    int64_t need = 0;                // bytes of the device block
    int64_t m(int i) const { return start[i + 1] - start[i]; }
};

// The arguments of the 16-query passes (batch_fused_kernel, batch_view_kernel: csrc/vq_sim_batch.hip).
struct BatchFusedArgs {
    const void* feats;
    const double* t;          // [Q][NV][D]
    const double* w;          // [Q][S]
    const uint8_t* present;   // [n][S][E] or null
    double* scores;           // [Q][n]
    int64_t n;
    int32_t Q, S, E, D;
    double* avg;              // ROUND only: [Q][n][S]
};

// A round over the UNION of up to 16 row views (vq_db_query_round_views, include/vq_amd_round_views.h): n stays the database's N, the
// tiles the pass walks are those of `items`, and query q's avg / scores are compact pieces that start at entry start[q].
struct BatchViewArgs : BatchFusedArgs {
    const int32_t* items;     // rows: the union's database rows, ascending, padded to a multiple of 16 with its last row | tiled: the tiles
                              // the union touches, ascending | null: the whole database (a view of the round is -1)
    const int64_t* counts;    // device, written by the plan: [0] rows of the union, [1] tiles it touches (read only with items)
    const int32_t* inv;       // [16][inv_stride]: the position of a database row in query q's view, -1 = not a member (unused for a whole query)
    int64_t inv_stride;
    const int64_t* start;     // device [17]: the first entry of query q's piece
    uint32_t whole;           // bit q: query q covers the whole database (position = row)
    uint32_t members;         // bit q: query q's row list is in inv; a query with neither bit (an empty view) stores nothing
};

struct vq_db {
    std::mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int S = 0, E = 0, D = 0, dtype = VQ_F32;
    // include/vq_amd_dim.h: d = the logical length of a vector, D = the stored pitch (d rounded up to a multiple of 4; the pads d..D-1
    // of every stored vector and of the query are +0.0).  d == D on every handle created without VQ_DIM_PADDED.  short_rows: the handle
    // was created with VQ_DIM_SHORT_ROWS (scan_short_kernel at D <= 128)
    int d = 0;
    bool short_rows = false;
    int cus = 256;
    void* feats = nullptr;           // the one block that may be adopted (vq_db_adopt_device): raw, released by release_feats alone
    bool owns_feats = true;
    void release_feats() {
        if (owns_feats && feats) (void)hipFree(feats);
        feats = nullptr;
    }
    ~vq_db() { release_feats(); }
    // VQ_LAYOUT_ROWS: [N][S][E][D].  VQ_LAYOUT_TILED (fp32, own memory): [tile of 16 clips][S*E][D/4][clip][4] in the SAME block (a
    // tile's 16 rows and its tiled form cover the same bytes; the block is allocated for whole tiles) -- vq_db_set_layout.
    // VQ_LAYOUT_TILED64 (fp64): the same with the 16-byte unit of doubles, [tile][S*E][D/2][clip][2] (csrc/vq_tile_index.h);
    // VQ_LAYOUT_TILED16 (fp16): with the unit of halves, [tile][S*E][D/8][clip][8]
    int layout = VQ_LAYOUT_ROWS;
    bool tiled() const { return layout != VQ_LAYOUT_ROWS; }
    int unit() const { return tiled() ? vq::tile_unit_of((int)elem()) : 0; }      // elements per 16-byte unit of the layout; 0: rows
    int tiled_layout() const { return dtype == VQ_F32 ? VQ_LAYOUT_TILED : dtype == VQ_F64 ? VQ_LAYOUT_TILED64 : VQ_LAYOUT_TILED16; }   // the tiled layout of the storage type
    bool feats_exposed = false;      // adopted memory, or the raw pointer was handed out: the library no longer controls the layout
    vq::DeviceMem<uint8_t> present;
    vq::DeviceMem<double> t;    // [S*E*D] | w
    bool have_query = false, have_avg = false, have_scores = false, have_sims = false;
    void stale() { have_avg = have_scores = have_sims = false; }      // what the handle holds was computed from other inputs
    double* w = nullptr;        // [8], inside t
    vq::DeviceMem<double> sims; // lazily [N][S][E]
    double* avg = nullptr;      // [N][S]
    int32_t* ne = nullptr;      // [N][S]
    double* scores = nullptr;   // [N]
    // avg | ne | scores | sel_result | match prefix | near prefix are ONE device allocation (round_dev), in the order of the host
    // block of vq_db_query_round: a round's results go back in one copy
    vq::DeviceMem<char> round_dev;
    int64_t round_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // byte offsets of avg, ne, scores, result, matchp, nearp; [6] = total
    int64_t* matchp = nullptr;       // first kRoundPrefix rows of the last selection's match list
    int64_t* nearp = nullptr;
    // selection scratch
    vq::DeviceMem<int2> blk_cnt;
    vq::DeviceMem<double> blk_max;
    vq::DeviceMem<int64_t> blk_arg;
    int64_t* sel_result = nullptr;   // [3] device
    vq::DeviceMem<int64_t> rows0, rows1;     // [N] each
    int64_t last_n0 = 0, last_n1 = 0;
    vq::DeviceMem<uint64_t> tk_state;        // [2]
    vq::DeviceMem<unsigned int> tk_hist;     // [256]
    vq::DeviceMem<double> batch_buf; // batched scan: queries [Q][NV][D] | weights [Q][S] | (two-kernel form: sims [NV][Q][N]) | scores [Q][N]
    double* batch_scores = nullptr;  // where the scores of the last batched pass start, inside batch_buf or bround_dev
    int batch_q = 0;                 // queries of the last batched scan
    // Batched rounds (csrc/vq_rounds.hip; include/vq_amd_rounds.h, vq_amd_round_views.h, vq_amd_round_fit.h): ONE lazy allocation that
    // starts with the image of the host block (queries | weights | bands | n_e | avg | scores | results | prefixes: what comes and goes
    // in one copy each way) followed by the full match / near lists and the per-block scratch of the three-pass selection; `round` says
    // where each of these sits for the last round.
    vq::DeviceMem<char> bround_dev;
    vq::Event bround_ev[4];          // flag 8: start | pass done | selection done | copies done
    BatchRound round;
    // View rounds (vq_db_query_round_views, include/vq_amd_round_views.h): the plan's device block, allocated on the first one --
    // inv [16][stride] i32 | union rows [stride + 16] i32 | touched tiles [stride / 16] i32 | counts [2] i64 | start [17] i64 | the
    // per-block counts of the compaction [tiles / 256] int2 -- and what the last one covered
    vq::DeviceMem<char> vround_plan;
    bool vround_have = false;
    int64_t vround_union = 0, vround_tiles = 0;
    vq::DeviceMem<char> grid_buf;    // scratch for grid / gathers
    // Batched targets (vq_db_batch_targets, include/vq_amd_round_targets.h; csrc/vq_round_targets.hip): the image of the call's block |
    // the pools' Gram matrices | the coefficients of every draw | a status per (draw, slot), and the scratch area of the draws whose
    // systems do not fit into local memory.  Both grow on demand and go with the handle.
    vq::DeviceMem<char> targets_buf;
    vq::DeviceMem<double> targets_ws;
    // Batched top-k (vq_db_batch_round_topk, include/vq_amd_round_topk.h; csrc/vq_round_topk.hip): the image of the call's block | the
    // survivors of the long pieces | the state and the histograms of the eight radix passes | the block counts of the compaction.
    // Allocated by the first call, grows on demand, goes with the handle.
    vq::DeviceMem<char> btopk_buf;
    // Row views (vq_db_rows_define): resident index lists, one device block each.  `active` is the view the one-query path runs over
    // (-1: the whole database) and `na` the number of clips it then covers -- M, or N: what every result-side entry point counts with.
    struct RowView {
        bool defined = false;
        int64_t m = 0;               // rows in the view
        int64_t ntiles = 0;          // tiles of 16 clips it touches (databases of a tiled-capable shape, whichever the storage type; else no tile tables)
        vq::DeviceMem<int64_t> rows; // [m] | tiles [ntiles] | pos [ntiles][16]: ONE allocation, rows first
        int64_t* tiles = nullptr;
        int64_t* pos = nullptr;
    };
    std::vector<RowView> views;
    int active = -1;
    int64_t na = 0;
    size_t elem() const { return dtype == VQ_F64 ? 8 : dtype == VQ_F16 ? 2 : 4; }
};

namespace vq {

// The one dispatch on the storage type: f(T{}) with T = __half, float or double, the element type of the handle's feature block.
template <typename F>
int with_dtype(const vq_db* db, F&& f) {
    switch (db->dtype) {
        case VQ_F16: return f(__half{});
        case VQ_F32: return f(float{});
        case VQ_F64: return f(double{});
    }
    return fail(VQ_E_STATE, "internal: database of unknown dtype %d", db->dtype);
}
// ... and on the 256-element chunks of a vector, D / 256 in {1, 2, 3, 4}: f(std::integral_constant<int, CH>{}); the caller has checked D
template <typename F>
int with_chunks(const vq_db* db, F&& f) {
    switch (db->D / 256) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 2: return f(std::integral_constant<int, 2>{});
    }
    return f(std::integral_constant<int, 1>{});
}

// csrc/vq_db.hip: rows (by number) -> a dense row-major [L][S][E][D] block in the handle's gather scratch, whatever the layout; the
// caller holds the handle's lock and has its device current.  rows_dev: the same L row numbers already on the device (ordered on the
// handle's stream) -- they are then read there and nothing is uploaded.  Shared with csrc/vq_round_targets.hip.
int gather_rows_device(vq_db* db, const int64_t* rows_host, int L, const void** dense, const int64_t* rows_dev = nullptr);

// csrc/vq_sim.hip: the one-query scan over the row view in use (none: the whole database) on the handle's stream, from the handle's
// query into its avg / ne and, with_scores, under the handle's weights into its scores; keep_sims: the per-split similarities too
// (the handle's sims block exists).  The caller holds the handle's lock and has its device current, here and below.
int launch_scan(vq_db* db, bool with_scores, bool keep_sims);

// csrc/vq_rank.hip: the handle's scores again from its avg under its weights; the stable partition of the scores by a threshold and
// a lower bound (res = n_match, n_near, near_argmax copied back and waited for, or null: they stay on the device; with_prefix: the
// first kRoundPrefix rows of both lists next to them, for vq_db_query_round).
int launch_rescore(vq_db* db);
int select_threshold(vq_db* db, double threshold, double lower, int64_t res[3], bool with_prefix = false);

// csrc/vq_sim_batch.hip, for the rounds of csrc/vq_rounds.hip; the caller has checked the shape (D in {256,512,768,1024}, S <= 8).
// The 16-query pass of a round over the whole database: d_t [Q][NV][D], d_w [Q][8] -> d_scores [Q][n], d_avg [Q][n][S].  The pass
// over the union of a round's views; max_tiles bounds the tiles its plan can hold.
int launch_round_pass(vq_db* db, int Q, const double* d_t, const double* d_w, double* d_scores, double* d_avg);
int launch_view_pass(vq_db* db, BatchViewArgs f, int64_t max_tiles);

}  // namespace vq
