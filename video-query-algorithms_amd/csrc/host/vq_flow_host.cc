// Host arithmetic of the flow handle: see vq_flow_host.h.  No HIP include; plain C++17.
#include "vq_flow_host.h"

#include <cmath>
#include <cstring>
#include <utility>

namespace vq {

std::vector<Level> pyramid_levels(int h, int w, int nscales, float scale_step, int max_pairs) {
    std::vector<Level> levels;
    size_t off = 0;
    int lh = h, lw = w;
    for (int s = 0; s < nscales; ++s) {
        if (s > 0) {
            const int nh = (int)std::nearbyint((double)lh * (double)scale_step), nw = (int)std::nearbyint((double)lw * (double)scale_step);
            if (nh < 16 || nw < 16) break;
            lh = nh;
            lw = nw;
        }
        levels.push_back(Level{lh, lw, off});
        off += (size_t)max_pairs * lh * lw;
    }
    return levels;
}

TileCut fit_tiles(int w, int h, int pairs, int slots, int halo, int max_cells) {
    TileCut best{0, 0, 0, 0, 0, 0};
    long long best_cost = -1;
    for (int nx = 1; nx <= (w + 7) / 8; ++nx) {
        const int tw = (w + nx - 1) / nx, ew = tw + 2 * halo;
        for (int ny = 1; ny <= (h + 7) / 8; ++ny) {
            const int th = (h + ny - 1) / ny, eh = th + 2 * halo;
            if ((long long)ew * eh > max_cells) continue;
            const long long waves = ((long long)ew * eh + 63) / 64;
            const long long rounds = ((long long)nx * ny * pairs + slots - 1) / slots;
            const long long cost = rounds * waves;
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = TileCut{nx, ny, tw, th, ew, eh};
            }
        }
    }
    return best;
}

static double det3x3(const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

bool invert3x3(const double m[9], double o[9]) {
    const double det = det3x3(m);
    if (!(std::fabs(det) > 1e-300)) return false;
    o[0] = (m[4] * m[8] - m[5] * m[7]) / det;
    o[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = (m[5] * m[6] - m[3] * m[8]) / det;
    o[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = (m[3] * m[7] - m[4] * m[6]) / det;
    o[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}

bool guard_homography(int matches, int inliers, double H[9]) {
    constexpr int kMinMatches = 50, kMinInliers = 25;
    if (matches > kMinMatches && inliers > kMinInliers && std::fabs(det3x3(H)) > 1e-300) return false;
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(H, eye, sizeof eye);
    return true;
}

bool solve_dense(std::vector<double>& A, std::vector<double>& b, int n) {
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
        if (std::fabs(A[(size_t)piv * n + c]) < 1e-300) return false;
        if (piv != c) {
            for (int q = 0; q < n; ++q) std::swap(A[(size_t)c * n + q], A[(size_t)piv * n + q]);
            std::swap(b[c], b[piv]);
        }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[(size_t)r * n + c] / A[(size_t)c * n + c];
            for (int q = c; q < n; ++q) A[(size_t)r * n + q] -= f * A[(size_t)c * n + q];
            b[r] -= f * b[c];
        }
    }
    for (int c = n - 1; c >= 0; --c) {
        double v = b[c];
        for (int q = c + 1; q < n; ++q) v -= A[(size_t)c * n + q] * b[q];
        b[c] = v / A[(size_t)c * n + c];
    }
    return true;
}

bool refit_homography(const float* src, const float* dst, const uint8_t* mask, int n, double* H) {
    int k = 0;
    double cs[2] = {0, 0}, cd[2] = {0, 0};
    for (int i = 0; i < n; ++i)
        if (mask[i]) {
            cs[0] += src[2 * i];
            cs[1] += src[2 * i + 1];
            cd[0] += dst[2 * i];
            cd[1] += dst[2 * i + 1];
            ++k;
        }
    if (k < 4) return false;
    for (int q = 0; q < 2; ++q) {
        cs[q] /= k;
        cd[q] /= k;
    }
    double ms = 0, md = 0;
    for (int i = 0; i < n; ++i)
        if (mask[i]) {
            ms += std::sqrt((src[2 * i] - cs[0]) * (src[2 * i] - cs[0]) + (src[2 * i + 1] - cs[1]) * (src[2 * i + 1] - cs[1]));
            md += std::sqrt((dst[2 * i] - cd[0]) * (dst[2 * i] - cd[0]) + (dst[2 * i + 1] - cd[1]) * (dst[2 * i + 1] - cd[1]));
        }
    if (ms <= 0 || md <= 0) return false;
    const double ss = std::sqrt(2.0) * k / ms, sd = std::sqrt(2.0) * k / md;
    std::vector<double> N(64, 0.0), r(8, 0.0);
    for (int i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        const double x = (src[2 * i] - cs[0]) * ss, y = (src[2 * i + 1] - cs[1]) * ss;
        const double u = (dst[2 * i] - cd[0]) * sd, v = (dst[2 * i + 1] - cd[1]) * sd;
        const double r0[8] = {x, y, 1, 0, 0, 0, -u * x, -u * y}, r1[8] = {0, 0, 0, x, y, 1, -v * x, -v * y};
        for (int a = 0; a < 8; ++a) {
            for (int b = 0; b < 8; ++b) N[a * 8 + b] += r0[a] * r0[b] + r1[a] * r1[b];
            r[a] += r0[a] * u + r1[a] * v;
        }
    }
    if (!solve_dense(N, r, 8)) return false;
    const double Hn[9] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], 1.0};
    // H = Td^-1 Hn Ts with Ts = [ss 0 -ss cs0; 0 ss -ss cs1; 0 0 1], Td^-1 = [1/sd 0 cd0; 0 1/sd cd1; 0 0 1]
    double M[9];
    for (int a = 0; a < 3; ++a) {
        M[a * 3] = Hn[a * 3] * ss;
        M[a * 3 + 1] = Hn[a * 3 + 1] * ss;
        M[a * 3 + 2] = -Hn[a * 3] * ss * cs[0] - Hn[a * 3 + 1] * ss * cs[1] + Hn[a * 3 + 2];
    }
    double G[9];
    for (int q = 0; q < 3; ++q) {
        G[q] = M[q] / sd + cd[0] * M[6 + q];
        G[3 + q] = M[3 + q] / sd + cd[1] * M[6 + q];
        G[6 + q] = M[6 + q];
    }
    if (std::fabs(G[8]) < 1e-300) return false;
    for (int q = 0; q < 9; ++q) H[q] = G[q] / G[8];
    return true;
}

RansacScratch ransac_scratch(int n, int max_points) {
    RansacScratch s;
    s.points_bytes = (size_t)n * max_points * 2 * sizeof(float);
    s.h = 0;
    s.src = (size_t)n * 9 * sizeof(double);
    s.dst = s.src + s.points_bytes;
    s.counts = s.dst + s.points_bytes;
    s.best = s.counts + (size_t)n * sizeof(int);
    s.winner = s.best + (size_t)n * sizeof(int);
    s.mask = s.winner + (size_t)n * sizeof(int);
    s.total = s.mask + (size_t)n * max_points + 64;
    return s;
}

WarpScratch warp_scratch(int n, int max_corners) {
    WarpScratch s;
    s.corners_bytes = (size_t)n * max_corners * 2 * sizeof(float);
    s.corners = 0;
    s.moved = s.corners_bytes;
    s.counts = 2 * s.corners_bytes;
    s.total = s.counts + (size_t)n * sizeof(int);
    return s;
}

}  // namespace vq
