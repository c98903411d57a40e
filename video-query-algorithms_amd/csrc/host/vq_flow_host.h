// The host arithmetic of the flow handle (csrc/vq_flow.hip) that touches no device: pyramid sizes, the tile cut of a level, the
// launch chunks of an inner loop, the fp64 homography algebra and the layout of the two scratch blocks.  Host-only, sanitizer-built.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vq {

struct Level {
    int h, w;
    size_t off;          // float offset of this level inside a per-plane pyramid buffer of max_pairs pairs: [level][pair][h][w]
};
// level sizes, finest first: round(previous * scale_step), stop before 16 pixels (oracle.pyramid_sizes)
std::vector<Level> pyramid_levels(int h, int w, int nscales, float scale_step, int max_pairs);

// The cut of a w x h level into nx x ny tiles of ceil(w / nx) x ceil(h / ny) own pixels (ew x eh cells with a halo of `halo` on every
// side, at most max_cells of them) that costs `pairs` pairs the least on `slots` workgroup slots: a workgroup's time goes with its cells
// (halo included) in whole waves, a launch's with its rounds.
struct TileCut {
    int nx, ny, tw, th, ew, eh;
};
TileCut fit_tiles(int w, int h, int pairs, int slots, int halo, int max_cells);

// Launches of an inner loop of at most `iterations` iterations in blocks of `block`: a pair needs at most ceil(iterations / block)
// blocks, one replay and one closing launch.  They are queued in chunks (2 launches while fewer than 4 are out, then 4, clipped to
// what is left); the host looks at the live flag between chunks.
inline int max_launches(int iterations, int block) { return (iterations + block - 1) / block + 2; }
inline int launch_chunk(int l0, int max_launches) {
    const int chunk = l0 < 4 ? 2 : 4;
    return max_launches - l0 < chunk ? max_launches - l0 : chunk;
}

// 3x3 inverse by cofactors (fp64), as numpy.linalg.inv does to rounding; false (out untouched) unless |det| > 1e-300
bool invert3x3(const double m[9], double out[9]);
bool solve_dense(std::vector<double>& A, std::vector<double>& b, int n);   // Gaussian elimination, partial pivoting; b <- solution
// Least-squares homography (h33 = 1 in normalised coordinates) over the points with mask[i] != 0: Hartley normalisation of both point
// sets, normal equations of the 2k x 8 system in fp64, de-normalised and scaled to H[8] = 1.  false: fewer than 4 points, or degenerate.
bool refit_homography(const float* src, const float* dst, const uint8_t* mask, int n, double* H);
// dense_flow's guards: H becomes the identity unless there are more than 50 matches, more than 25 inliers and H can be inverted.
// Returns true when H was replaced.
bool guard_homography(int matches, int inliers, double H[9]);

// Byte offsets inside the RANSAC scratch block of n pairs of at most max_points matches (8-byte aligned things first) ...
struct RansacScratch {
    size_t h, src, dst, counts, best, winner, mask, total;     // double [n][9], float [n][max_points][2] x 2, int [n] x 3, uint8 [n][max_points]
    size_t points_bytes;                                       // bytes of src (= of dst)
};
RansacScratch ransac_scratch(int n, int max_points);
// ... and inside the scratch block of vq_flow_warped: corners, moved corners (float [n][max_corners][2] each), counts (int [n])
struct WarpScratch {
    size_t corners, moved, counts, total;
    size_t corners_bytes;
};
WarpScratch warp_scratch(int n, int max_corners);

}  // namespace vq
