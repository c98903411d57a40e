// Where element k of vector (row, slice v) of a feature block sits, for every layout of a resident database (vq_db_set_layout): the
// ONE statement of the rule, shared by csrc/vq_db.hip, csrc/vq_csv.hip and the host-only test of the rule (no HIP include: plain C++).
//
//   rows (unit 0):  [N][NV][D]
//   tiled (unit U): [tile of 16 clips][NV][D / U][clip][U] -- U elements = the 16 bytes a lane loads: 4 floats (VQ_LAYOUT_TILED),
//                   2 doubles (VQ_LAYOUT_TILED64) or 8 halves (VQ_LAYOUT_TILED16).  A (tile, slice) is 16 D elements whichever the order, so a tile's 16 rows and its
//                   tiled form cover the same bytes, and 64 consecutive units are 1 KB: 4 k-groups of 16 clips.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VQ_TILE_HD __host__ __device__
#else
#define VQ_TILE_HD
#endif

namespace vq {

// elements per 16-byte unit of the tiled layout of a storage type (elem = its size in bytes)
VQ_TILE_HD constexpr int tile_unit_of(int elem) { return 16 / elem; }

// element (row, v, k) of a tiled block with units of U elements, in elements from the start of the block
VQ_TILE_HD inline int64_t tiled_index(int U, int64_t row, int NV, int v, int D, int k) {
    return (((row >> 4) * NV + v) * (int64_t)(D / U) + k / U) * (16 * U) + (row & 15) * U + k % U;
}

// the same for any layout: unit 0 = row-major
VQ_TILE_HD inline int64_t feat_index(int unit, int64_t row, int NV, int v, int D, int k) {
    return unit ? tiled_index(unit, row, NV, v, D, k) : (row * NV + v) * (int64_t)D + k;
}

}  // namespace vq
