// stereo.h -- the constants and the small rules of the sparse stereo correspondence (feat_stereo_kernel in feat.hip), shared
// by the kernel and the host tests (compiled for the host with __host__ / __device__ defined away, as feat.h is).  Integer
// arithmetic up to one float64 division in the parabola and the triangulation, whose expressions hold no a * b + c, so the
// GPU, this header on the host and tests/stereo_reference.py agree bit for bit.
//
//   window      15 x 3 around the keypoint; cost C(d) = the sum of squared differences, <= 45 * 255^2 = 2926125 < 2^22
//   key         (C << 9) | d, 0 <= d <= 256: 31 bits; the minimum key is the best cost and among equals the lowest d
//   range       D_lo = min_disparity - 1, D_hi = min(max_disparity + 1, u - 7); searched when D_hi - D_lo >= 2
//   uniqueness  with S the lowest cost at |d - d*| >= 2: not unique iff S * 100 <= C(d*) * (100 + uniqueness) in int64
//   parabola    d* + (a - c) / (2 (a - 2 b + c)) on a = C(d* - 1), b = C(d*), c = C(d* + 1): one division, one addition
//   point       Z = (baseline fx) / disparity, X = ((u - cx) Z) / fx, Y = ((v - cy) Z) / fy
#pragma once
#include <stdint.h>

#ifndef STEREO_HD
#define STEREO_HD __host__ __device__ static inline
#endif

#define STEREO_HALF_W 7            // rtabmap's 15 x 3 window
#define STEREO_HALF_H 1
#define STEREO_WIN_W (2 * STEREO_HALF_W + 1)
#define STEREO_WIN_H (2 * STEREO_HALF_H + 1)
#define STEREO_MAX_DISPARITY 255
#define STEREO_MAX_RANGE (STEREO_MAX_DISPARITY + 2)                    // disparities 0 .. 256
#define STEREO_STRIP_W (STEREO_MAX_RANGE - 1 + STEREO_WIN_W)           // 271 columns hold every window of a range
#define STEREO_COST_MAX (STEREO_WIN_W * STEREO_WIN_H * 255 * 255)      // 2926125
#define STEREO_KEY_SHIFT 9

enum { STEREO_ACCEPTED = 0, STEREO_OUTSIDE = 1, STEREO_NO_RANGE = 2, STEREO_EDGE = 3, STEREO_NOT_UNIQUE = 4, STEREO_LEFT_RIGHT = 5 };

STEREO_HD int32_t stereo_key(int32_t cost, int d) { return (int32_t)(((uint32_t)cost << STEREO_KEY_SHIFT) | (uint32_t)d); }
STEREO_HD int32_t stereo_key_cost(int32_t key) { return key >> STEREO_KEY_SHIFT; }
STEREO_HD int stereo_key_d(int32_t key) { return key & ((1 << STEREO_KEY_SHIFT) - 1); }

// the window around (u, v) lies in the H x W image
STEREO_HD bool stereo_inside(int u, int v, int H, int W) {
    return u >= STEREO_HALF_W && u <= W - 1 - STEREO_HALF_W && v >= STEREO_HALF_H && v <= H - 1 - STEREO_HALF_H;
}

// the disparities searched for a left keypoint at column u; false: fewer than three, nothing to search
STEREO_HD bool stereo_range(int u, int min_disparity, int max_disparity, int *d_lo, int *d_hi) {
    const int room = u - STEREO_HALF_W;
    *d_lo = min_disparity - 1;
    *d_hi = max_disparity + 1 < room ? max_disparity + 1 : room;
    return *d_hi - *d_lo >= 2;
}

// the upper end of the range searched back from the right column ur into the left image of width W
STEREO_HD int stereo_range_back(int ur, int W, int max_disparity) {
    const int room = W - 1 - STEREO_HALF_W - ur;
    return max_disparity + 1 < room ? max_disparity + 1 : room;
}

STEREO_HD bool stereo_not_unique(int32_t second, int32_t best, int uniqueness) {
    return (int64_t)second * 100 <= (int64_t)best * (100 + uniqueness);
}

// a > b (the tie rule) and c >= b, so the denominator is positive and the offset lies in [-0.5, 0.5]
STEREO_HD double stereo_parabola(int d, int32_t a, int32_t b, int32_t c) {
    const int32_t den = a - 2 * b + c;
    return (double)d + (double)(a - c) / (double)(2 * den);
}

STEREO_HD void stereo_point(int u, int v, double disparity, double fx, double fy, double cx, double cy, double baseline, double *p) {
    const double Z = (baseline * fx) / disparity;
    p[0] = (((double)u - cx) * Z) / fx;
    p[1] = (((double)v - cy) * Z) / fy;
    p[2] = Z;
}
