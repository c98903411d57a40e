// The element-address rule of the tiled layouts (video-query-algorithms_amd/csrc/vq_tile_index.h) in a stand-alone host program, built
// under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_tiled64_host.py.
//
//   tile_index_driver            every check below; prints "tile_index: ok"
//   tile_index_driver U row NV v D k   the index of one element (unit U, 0 = rows), for the test's own comparison
//
// Per (unit, n, NV, D): the rule maps the elements of the whole tiles of a block of n clips ONE TO ONE onto [0, tiles * 16 * NV * D)
// (the marks live in a vector of exactly that size: an index outside it is a sanitizer finding), a tile's 16 rows land inside the
// tile's own bytes, a lane's U elements are adjacent, 64 consecutive units are 4 k-groups of 16 clips, unit 4 agrees with the fp32
// formula as vq_sim.hip and vq_csv.hip wrote it before this header, and unit 0 is row-major.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vq_tile_index.h"

static int64_t fp32_rule(int64_t row, int NV, int v, int D, int k) {      // as written in the feature database's unit (feat_index) before
    return (((row >> 4) * NV + v) * (int64_t)(D / 4) + (k >> 2)) * 64 + (row & 15) * 4 + (k & 3);
}

static int check(int U, int64_t n, int NV, int D) {
    const int64_t tiles = (n + 15) / 16, tile_elems = (int64_t)16 * NV * D, total = tiles * tile_elems;
    std::vector<unsigned char> seen((size_t)total, 0);
    for (int64_t row = 0; row < tiles * 16; ++row)
        for (int v = 0; v < NV; ++v)
            for (int k = 0; k < D; ++k) {
                const int64_t i = vq::tiled_index(U, row, NV, v, D, k);
                if (i < (row >> 4) * tile_elems || i >= ((row >> 4) + 1) * tile_elems) return printf("U %d: (%lld, %d, %d) leaves its tile\n", U, (long long)row, v, k);
                if (seen[(size_t)i]++) return printf("U %d: element %lld hit twice\n", U, (long long)i);
                if (i != vq::feat_index(U, row, NV, v, D, k)) return printf("feat_index differs from tiled_index\n");
                if (k % U && i != vq::tiled_index(U, row, NV, v, D, k - 1) + 1) return printf("U %d: a unit is not contiguous\n", U);
                // unit g of the slice sits at g * 16 + clip: 64 consecutive units = k-groups 4 j .. 4 j + 3 of the 16 clips = 1 KB
                const int64_t unit = (i - ((row >> 4) * NV + v) * (int64_t)16 * D) / U;
                if (unit != (int64_t)(k / U) * 16 + (row & 15)) return printf("U %d: unit order\n", U);
                if (U == 4 && i != fp32_rule(row, NV, v, D, k)) return printf("unit 4 is not the fp32 rule\n");
                if (vq::feat_index(0, row, NV, v, D, k) != (row * NV + v) * (int64_t)D + k) return printf("unit 0 is not row-major\n");
            }
    for (unsigned char s : seen)
        if (s != 1) return printf("U %d: not onto\n", U);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7) {
        printf("%lld\n", (long long)vq::feat_index(atoi(argv[1]), atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])));
        return 0;
    }
    if (vq::tile_unit_of(4) != 4 || vq::tile_unit_of(8) != 2) return printf("tile_unit_of\n"), 1;
    const int64_t ns[] = {1, 16, 17, 37};                    // one clip, a whole tile, ragged last tiles
    for (int U : {2, 4})
        for (int64_t n : ns) {
            if (check(U, n, 3, 64) || check(U, n, 1, 8)) return 1;
        }
    if (check(2, 21, 10, 1024) || check(4, 21, 10, 1024)) return 1;      // the largest shape the layouts take: S E = 10, D = 1024
    printf("tile_index: ok\n");
    return 0;
}
