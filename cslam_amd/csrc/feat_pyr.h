// feat_pyr.h -- the integer rules of the scale pyramid of the keyframe features (feat_pyr_level_kernel and
// feat_pyr_merge_kernel in feat.hip), shared by the kernels and the host tests (compiled for the host with __host__ /
// __device__ defined away, as feat.h is).  Integer arithmetic up to the final coordinates, which are one float64 division
// and one subtraction, so the GPU, this header on the host and tests/feat_pyramid_reference.py agree bit for bit.
//
//   levels      L = 1 .. 8, the scale per level 6 / 5; level l of an n-pixel axis has (n 5^l + 6^l / 2) / 6^l pixels
//   taps        level l from level l - 1, per axis and output index x: u = ((2 x + 1) n_prev 1024) / (2 n_l) - 512 in
//               int64, clamped to [0, (n_prev - 1) 1024]; i0 = u >> 10, a = u & 1023, i1 = min(i0 + 1, n_prev - 1)
//   blend       ((g00 (1024 - a) + g01 a) (1024 - b) + (g10 (1024 - a) + g11 a) b + 2^19) >> 20, in 0 .. 255
//   base pixel  the level-0 pixel under level pixel x: ((2 x + 1) n_0) / (2 n_l), always inside the image
//   base coord  the level-0 coordinate of level pixel x: (double)((2 x + 1) n_0) / (double)(2 n_l) - 0.5; x at level 0
//   budgets     w_l = 5^l 6^(L - 1 - l); level l gets max_features w_l / sum w, the remainder goes to level 0
//   point       X = ((kx - cx) Z) / fx, Y = ((ky - cy) Z) / fy on the base coordinates; an invalid Z gives a NaN row
//   sub-pixel   per axis, from the int32 responses m, c, p of the level's map at the keypoint's two neighbours along the axis
//               and at the keypoint: den = m - 2 c + p and num = m - p in int64; den >= 0 (a plateau, or no maximum along the
//               axis) or a neighbour outside the image: off = 0; else off = (double)num / (double)(2 den), one division,
//               clamped to [-0.5, 0.5].  Level-0 coordinate: ((double)(2 x + 1) + 2 off) (double)n_0 / (double)(2 n_l) - 0.5
//               in this order; no product feeds an addition, so contraction changes no bit, and off = 0 gives base coord.
#pragma once
#include "feat.h"

#define FEAT_PYR_MAX_LEVELS 8
#define FEAT_PYR_MAX_SIDE (1 << 20)       // (2 x + 1) n 1024 stays far inside int64
#define FEAT_PYR_ONE 1024

FEAT_HD int64_t feat_pyr_pow(int base, int e) {
    int64_t p = 1;
    for (int i = 0; i < e; ++i) p *= base;
    return p;
}

FEAT_HD int feat_pyr_size(int n, int l) {
    const int64_t den = feat_pyr_pow(6, l);
    return (int)(((int64_t)n * feat_pyr_pow(5, l) + den / 2) / den);
}

FEAT_HD void feat_pyr_tap(int x, int n_l, int n_prev, int *i0, int *i1, int *a) {
    int64_t u = ((int64_t)(2 * x + 1) * n_prev * FEAT_PYR_ONE) / (2 * (int64_t)n_l) - FEAT_PYR_ONE / 2;
    const int64_t top = (int64_t)(n_prev - 1) * FEAT_PYR_ONE;
    u = u < 0 ? 0 : (u > top ? top : u);
    *i0 = (int)(u >> 10);
    *a = (int)(u & (FEAT_PYR_ONE - 1));
    *i1 = *i0 + 1 < n_prev ? *i0 + 1 : n_prev - 1;
}

// at most 255 * 2^20 + 2^19 < 2^31
FEAT_HD int feat_pyr_blend(int g00, int g01, int g10, int g11, int a, int b) {
    return ((g00 * (FEAT_PYR_ONE - a) + g01 * a) * (FEAT_PYR_ONE - b) + (g10 * (FEAT_PYR_ONE - a) + g11 * a) * b + (1 << 19)) >> 20;
}

FEAT_HD int feat_pyr_base_pixel(int x, int n_0, int n_l) { return (int)(((int64_t)(2 * x + 1) * n_0) / (2 * (int64_t)n_l)); }

FEAT_HD double feat_pyr_base_coord(int x, int n_0, int n_l) {
    return (double)((int64_t)(2 * x + 1) * n_0) / (double)(2 * (int64_t)n_l) - 0.5;
}

// the offset of a maximum along one axis from the responses before, at and after it
FEAT_HD double feat_pyr_subpix_offset(int32_t m, int32_t c, int32_t p) {
    const int64_t den = (int64_t)m - 2 * (int64_t)c + (int64_t)p, num = (int64_t)m - (int64_t)p;
    if (den >= 0) return 0.0;
    const double off = (double)num / (double)(2 * den);
    return off < -0.5 ? -0.5 : (off > 0.5 ? 0.5 : off);
}

// both offsets of the keypoint (x, y) of an H x W response map R; an axis whose neighbour lies outside the image gives 0
FEAT_HD void feat_pyr_subpix(const int32_t *R, int H, int W, int x, int y, double *off) {
    off[0] = off[1] = 0.0;
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    const int32_t *r = R + (int64_t)y * W + x;
    if (x >= 1 && x + 1 < W) off[0] = feat_pyr_subpix_offset(r[-1], r[0], r[1]);
    if (y >= 1 && y + 1 < H) off[1] = feat_pyr_subpix_offset(r[-(int64_t)W], r[0], r[W]);
}

FEAT_HD double feat_pyr_subpix_coord(int x, double off, int n_0, int n_l) {
    return ((double)(2 * (int64_t)x + 1) + 2.0 * off) * (double)n_0 / (double)(2 * (int64_t)n_l) - 0.5;
}

FEAT_HD void feat_pyr_budgets(int max_features, int levels, int *budget) {
    int64_t sum = 0;
    for (int l = 0; l < levels; ++l) sum += feat_pyr_pow(5, l) * feat_pyr_pow(6, levels - 1 - l);
    int given = 0;
    for (int l = 0; l < levels; ++l) {
        budget[l] = (int)(((int64_t)max_features * feat_pyr_pow(5, l) * feat_pyr_pow(6, levels - 1 - l)) / sum);
        given += budget[l];
    }
    budget[0] += max_features - given;
}

// the operation order of feat_points_kernel; p = a NaN row unless Z is finite and > 0
FEAT_HD void feat_pyr_point(double kx, double ky, double Z, double fx, double fy, double cx, double cy, double *p) {
    p[0] = p[1] = p[2] = NAN;
    if (!(Z > 0.0 && Z <= 1.7976931348623157e308)) return;
    p[0] = ((kx - cx) * Z) / fx;
    p[1] = ((ky - cy) * Z) / fy;
    p[2] = Z;
}
