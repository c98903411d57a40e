// The element-address rule of the tiled layouts (video-query-algorithms_amd/csrc/vq_tile_index.h) for the unit of float16 storage --
// U = 8 halves, VQ_LAYOUT_TILED16 -- in a stand-alone host program, built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_tiled16_host.py.
//
//   tile16_driver                  every check below; prints "tile16: ok"
//   tile16_driver U row NV v D k   the index of one element (unit U, 0 = rows), for the test's own comparison
//
// Per (n, NV, D): the rule maps the elements of the whole tiles of a block of n clips ONE TO ONE onto [0, tiles * 16 * NV * D) (the marks
// live in a vector of exactly that size: an index outside it is a sanitizer finding), a tile's 16 rows land inside the tile's own
// elements, a lane's 8 halves are adjacent, and 64 consecutive units (1 KB: one wave instruction) are 4 k-groups of 16 clips -- lane l
// of load i of scan_tiled_kernel<__half> holds clip l % 16, k = 32 i + 8 (l / 16) + 0..7 at i * 512 + l * 8 halves of the slice, which is
// also load m' = i % 4 of chunk i / 4 of ChunkP<__half, 8>::load_tiled (lane offset kk * 128 + col * 8, chunk step 2048).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vq_tile_index.h"

static int check(int64_t n, int NV, int D) {
    const int U = 8;
    const int64_t tiles = (n + 15) / 16, tile_elems = (int64_t)16 * NV * D, total = tiles * tile_elems;
    std::vector<unsigned char> seen((size_t)total, 0);
    for (int64_t row = 0; row < tiles * 16; ++row)
        for (int v = 0; v < NV; ++v)
            for (int k = 0; k < D; ++k) {
                const int64_t i = vq::tiled_index(U, row, NV, v, D, k);
                if (i < (row >> 4) * tile_elems || i >= ((row >> 4) + 1) * tile_elems) return printf("(%lld, %d, %d) leaves its tile\n", (long long)row, v, k);
                if (seen[(size_t)i]++) return printf("element %lld hit twice\n", (long long)i);
                if (i != vq::feat_index(U, row, NV, v, D, k)) return printf("feat_index differs from tiled_index\n");
                if (k % U && i != vq::tiled_index(U, row, NV, v, D, k - 1) + 1) return printf("a unit is not contiguous\n");
                const int64_t in_slice = i - ((row >> 4) * NV + v) * (int64_t)16 * D;
                if (in_slice / U != (int64_t)(k / U) * 16 + (row & 15)) return printf("unit order\n");
                // the wave's view: 64 consecutive units = one load; lane = unit % 64 = (clip, k-group), load = unit / 64
                const int64_t unit = in_slice / U, load = unit / 64, lane = unit % 64;
                if (lane % 16 != (row & 15) || k != 32 * load + 8 * (lane / 16) + k % U) return printf("1 KB is not 4 k-groups of 16 clips\n");
                if (in_slice != load * 512 + lane * 8 + k % U) return printf("a lane's load is not at i * 512 + l * 8\n");
                // the 16-query pass: chunk c = load / 4 (128 elements), load m' = load % 4, lane offset kk * 128 + col * 8
                if (in_slice != (load / 4) * 2048 + (load % 4) * 512 + (lane / 16) * 128 + (lane % 16) * 8 + k % U) return printf("chunk addressing\n");
                if (k != 128 * (load / 4) + 32 * (load % 4) + 8 * (lane / 16) + k % U) return printf("chunk elements\n");
            }
    for (unsigned char s : seen)
        if (s != 1) return printf("not onto\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7) {
        printf("%lld\n", (long long)vq::feat_index(atoi(argv[1]), atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])));
        return 0;
    }
    if (vq::tile_unit_of(2) != 8) return printf("tile_unit_of(2)\n"), 1;
    const int64_t ns[] = {1, 16, 17, 37};                    // one clip, a whole tile, ragged last tiles
    for (int64_t n : ns) {
        if (check(n, 3, 64) || check(n, 1, 8)) return 1;
    }
    if (check(21, 10, 1024)) return 1;                        // the largest shape the layout takes: S E = 10, D = 1024
    printf("tile16: ok\n");
    return 0;
}
