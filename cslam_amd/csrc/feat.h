// feat.h -- the constants, the sampling pattern and the small integer rules of the keyframe features (feat.hip), shared by
// the kernels and the host tests (compiled for the host with __host__ / __device__ defined away, as pnp.h is).  Everything
// here is integer arithmetic, so the GPU, this header on the host and tests/feat_reference.py agree bit for bit.
//
//   grey        (1868 B + 9617 G + 4899 R + 8192) >> 14
//   isqrt       the exact floor square root of 0 <= D < 2^62: sqrt in double, then integer compares move it into place
//   response    R = (a + c) - isqrt((a - c)^2 + 4 b^2) on the 3 x 3 box sums a, b, c of Ix^2, Ix Iy, Iy^2
//   bins        32 directions; (C_k, S_k) for k < 8 are the literals below, bins 8 .. 31 exact quarter turns (c, s) -> (-s, c);
//               the bin of moments (m10, m01) is the k with the largest m10 C_k + m01 S_k in int64, the lowest k on ties
//   generator   draw n = splitmix64(FEAT_SEED + n): x = (low 32 bits) mod 27 - 13, y = (high 32 bits) mod 27 - 13, kept when
//               x^2 + y^2 <= 13^2, otherwise the next draw.  Pair i = the next two kept points (p, q); when q = p the pair is
//               dropped and drawn again from the draw after it.
//   rotation    of (x, y) into bin k: by (C, S) of k mod 8 as ((x C - y S), (x S + y C)) / 16384 rounded half away from zero
//               in integers, then k / 8 quarter turns (x, y) -> (-y, x).  No floating point.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef FEAT_HD
#define FEAT_HD __host__ __device__ static inline
#endif

#define FEAT_PATCH_RADIUS 15       // moments over x^2 + y^2 <= 15^2; every rotated pattern point lies within it
#define FEAT_BLUR_RADIUS 3         // [1, 6, 15, 20, 15, 6, 1] in both directions, unnormalised
#define FEAT_MIN_BORDER (FEAT_PATCH_RADIUS + FEAT_BLUR_RADIUS)
#define FEAT_PATTERN_RADIUS 13
#define FEAT_PAIRS 256
#define FEAT_DESC_BYTES (FEAT_PAIRS / 8)
#define FEAT_BINS 32
#define FEAT_SEED 0x0BADC0FFEE0DDF00ull
#define FEAT_R_MAX 18727200        // 2 * 9 * 1020^2: no response exceeds it

FEAT_HD int feat_gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

FEAT_HD int64_t feat_isqrt(int64_t d) {
    int64_t s = (int64_t)sqrt((double)d);
    while (s * s > d) --s;
    while ((s + 1) * (s + 1) <= d) ++s;
    return s;
}

FEAT_HD int32_t feat_response(int64_t a, int64_t b, int64_t c) {
    return (int32_t)((a + c) - feat_isqrt((a - c) * (a - c) + 4 * b * b));
}

FEAT_HD void feat_direction(int k, int *c, int *s) {
    const int C[8] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196};
    const int S[8] = {0, 3196, 6270, 9102, 11585, 13623, 15137, 16069};
    int x = C[k & 7], y = S[k & 7];
    for (int q = (k >> 3) & 3; q > 0; --q) { const int t = x; x = -y; y = t; }
    *c = x;
    *s = y;
}

FEAT_HD int feat_bin(int64_t m10, int64_t m01) {
    int best = 0;
    int64_t best_v = 0;
    for (int k = 0; k < FEAT_BINS; ++k) {
        int c, s;
        feat_direction(k, &c, &s);
        const int64_t v = m10 * c + m01 * s;
        if (k == 0 || v > best_v) { best = k; best_v = v; }
    }
    return best;
}

FEAT_HD int feat_round14(int v) { return v >= 0 ? (v + 8192) >> 14 : -((-v + 8192) >> 14); }

FEAT_HD void feat_rotate(int x, int y, int k, int *xr, int *yr) {
    int c, s;
    feat_direction(k & 7, &c, &s);
    int u = feat_round14(x * c - y * s), v = feat_round14(x * s + y * c);
    for (int q = (k >> 3) & 3; q > 0; --q) { const int t = u; u = -v; v = t; }
    *xr = u;
    *yr = v;
}

static constexpr uint64_t feat_mix64(uint64_t z) {         // splitmix64's output function after its increment
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct FeatPattern { int8_t v[FEAT_PAIRS][4]; };           // px, py, qx, qy

static constexpr FeatPattern feat_make_pattern() {
    FeatPattern pat = {};
    uint64_t n = 0;
    for (int i = 0; i < FEAT_PAIRS;) {
        int pt[4] = {0, 0, 0, 0};
        for (int j = 0; j < 2;) {
            const uint64_t v = feat_mix64(FEAT_SEED + n++);
            const int x = (int)((v & 0xffffffffull) % 27) - 13, y = (int)((v >> 32) % 27) - 13;
            if (x * x + y * y <= FEAT_PATTERN_RADIUS * FEAT_PATTERN_RADIUS) { pt[2 * j] = x; pt[2 * j + 1] = y; ++j; }
        }
        if (pt[0] == pt[2] && pt[1] == pt[3]) continue;
        for (int e = 0; e < 4; ++e) pat.v[i][e] = (int8_t)pt[e];
        ++i;
    }
    return pat;
}
