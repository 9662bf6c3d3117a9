// rectify.h -- from a raw camera's frame to the "pinhole, rectified, no distortion" image every visual stage starts from: the
// rule of image_proc's rectify (OpenCV initUndistortRectifyMap + remap), written once for the kernels of rectify.hip, the
// host tests and a stand-alone sanitizer program (compiled for the host with __host__ / __device__ defined away, as
// stereo.h is).  tests/rectify_reference.py restates it in numpy, operation for operation.
//
//   camera    26 float64: K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3, k4, k5, k6) (plumb-bob with the rational terms),
//             R row-major 3 x 3, P = (fx', fy', cx', cy') and P[0][3] = Tx fx' of the 3 x 4 projection, which the map does not
//             use (-P[0][3] / fx' is a right camera's baseline); the destination size (H, W) comes with the map
//   map       destination pixel (u, v) -> source position, float64, every product and sum rounded on its own (the
//             translation units that include this are built with -ffp-contract=off):
//               x = (u - cx') / fx', y = (v - cy') / fy', (X, Y, Wd) = R^T (x, y, 1); outside unless Wd > 0
//               xn = X / Wd, yn = Y / Wd, r2 = xn xn + yn yn, r4 = r2 r2, r6 = r4 r2
//               rad = (1 + k1 r2 + k2 r4 + k3 r6) / (1 + k4 r2 + k5 r4 + k6 r6)
//               xd = xn rad + 2 p1 xn yn + p2 (r2 + 2 xn xn), yd = yn rad + p1 (r2 + 2 yn yn) + 2 p2 xn yn
//               mx = fx xd + cx, my = fy yd + cy
//   quantised q = floor(m 32 + 0.5), 1/32 pixel, an int32 pair (qx, qy); both INT32_MIN when the pixel is outside, m is
//             not finite or |q| >= 2^26
//   bilinear  uint8, per channel: x0 = qx >> 5, ax = qx & 31 (arithmetic shift: negative coordinates floor), the weights
//             (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay, ax ay; a tap outside the source contributes 0;
//             value = (sum + 512) >> 10; valid iff every tap of non-zero weight lies inside
//   nearest   depth is never interpolated: xs = (qx + 16) >> 5, ys = (qy + 16) >> 5, the source element's bits, 0 outside
//
// The per-thread functions at the end are the kernels' bodies: a kernel is its index arithmetic and one call.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#ifndef RECTIFY_HD
#define RECTIFY_HD __host__ __device__ static inline
#endif

#define RECTIFY_CAM 26                     // float64 per camera
#define RECTIFY_SHIFT 5                    // 1/32 pixel
#define RECTIFY_ONE (1 << RECTIFY_SHIFT)
#define RECTIFY_Q_LIMIT 67108864.0         // 2^26
#define RECTIFY_NONE INT32_MIN
#define RECTIFY_RUN 4                      // destination pixels of one row per thread of the remap
#define RECTIFY_BLOCK 256

// ---- the map -------------------------------------------------------------------------------------------------------
RECTIFY_HD void rectify_map_pixel(const double *cam, int u, int v, int32_t *qx, int32_t *qy) {
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const double k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7], k3 = cam[8], k4 = cam[9], k5 = cam[10], k6 = cam[11];
    const double *R = cam + 12;
    const double pfx = cam[21], pfy = cam[22], pcx = cam[23], pcy = cam[24];         // cam[25], Tx fx', is the stereo pair's
    *qx = *qy = RECTIFY_NONE;
    const double x = ((double)u - pcx) / pfx, y = ((double)v - pcy) / pfy;
    const double X = R[0] * x + R[3] * y + R[6];
    const double Y = R[1] * x + R[4] * y + R[7];
    const double Wd = R[2] * x + R[5] * y + R[8];
    if (!(Wd > 0.0)) return;
    const double xn = X / Wd, yn = Y / Wd;
    const double r2 = xn * xn + yn * yn, r4 = r2 * r2, r6 = r4 * r2;
    const double rad = (1.0 + k1 * r2 + k2 * r4 + k3 * r6) / (1.0 + k4 * r2 + k5 * r4 + k6 * r6);
    const double xd = xn * rad + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn);
    const double yd = yn * rad + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn;
    const double mx = fx * xd + cx, my = fy * yd + cy;
    const double fqx = floor(mx * 32.0 + 0.5), fqy = floor(my * 32.0 + 0.5);
    if (!(fabs(fqx) < RECTIFY_Q_LIMIT && fabs(fqy) < RECTIFY_Q_LIMIT)) return;        // a NaN or an infinity fails too
    *qx = (int32_t)fqx;
    *qy = (int32_t)fqy;
}

// ---- the two samplers ----------------------------------------------------------------------------------------------
// One tap of C interleaved channels into the sums; returns whether it lay inside or had no weight.  Without a branch: the
// load is from the clamped position and a tap outside gets the weight 0, so a thread's loads are all issued before the
// first is waited for.
template <int C> RECTIFY_HD bool rectify_tap(const uint8_t *src, int Hs, int Ws, int x, int y, int w, int32_t *sum) {
    const bool inside = x >= 0 && x < Ws && y >= 0 && y < Hs;
    const int xc = x < 0 ? 0 : (x >= Ws ? Ws - 1 : x), yc = y < 0 ? 0 : (y >= Hs ? Hs - 1 : y);
    const uint8_t *p = src + ((int64_t)yc * Ws + xc) * C;
    const int32_t wi = inside ? w : 0;
    for (int ch = 0; ch < C; ++ch) sum[ch] += wi * (int32_t)p[ch];
    return inside || w == 0;
}

// the C values of one destination pixel; returns valid (0 or 1).  A sentinel needs no case of its own (x0 = -2^26: every tap
// is outside, the first with a weight of 1024), it has one for the reader.
template <int C> RECTIFY_HD uint32_t rectify_bilinear(const uint8_t *src, int Hs, int Ws, int32_t qx, int32_t qy, uint8_t *out) {
    const bool none = qx == RECTIFY_NONE || qy == RECTIFY_NONE;
    const int x0 = qx >> RECTIFY_SHIFT, y0 = qy >> RECTIFY_SHIFT;
    const int ax = qx & (RECTIFY_ONE - 1), ay = qy & (RECTIFY_ONE - 1), bx = RECTIFY_ONE - ax, by = RECTIFY_ONE - ay;
    int32_t sum[C];
    for (int ch = 0; ch < C; ++ch) sum[ch] = 0;
    bool ok = rectify_tap<C>(src, Hs, Ws, x0, y0, bx * by, sum);
    ok = rectify_tap<C>(src, Hs, Ws, x0 + 1, y0, ax * by, sum) && ok;
    ok = rectify_tap<C>(src, Hs, Ws, x0, y0 + 1, bx * ay, sum) && ok;
    ok = rectify_tap<C>(src, Hs, Ws, x0 + 1, y0 + 1, ax * ay, sum) && ok;
    for (int ch = 0; ch < C; ++ch) out[ch] = none ? (uint8_t)0 : (uint8_t)((sum[ch] + 512) >> 10);
    return ok && !none ? 1u : 0u;
}

// the index of the nearest source element, -1 when outside
RECTIFY_HD int64_t rectify_nearest_index(int Hs, int Ws, int32_t qx, int32_t qy) {
    if (qx == RECTIFY_NONE || qy == RECTIFY_NONE) return -1;
    const int64_t xs = ((int64_t)qx + RECTIFY_ONE / 2) >> RECTIFY_SHIFT, ys = ((int64_t)qy + RECTIFY_ONE / 2) >> RECTIFY_SHIFT;
    if (xs < 0 || xs >= Ws || ys < 0 || ys >= Hs) return -1;
    return ys * Ws + xs;
}

// ---- the kernels' bodies -------------------------------------------------------------------------------------------
// rectify_map_kernel: thread i of camera c, one destination pixel
RECTIFY_HD void rectify_map_thread(const double *cams, const int64_t *off, const int32_t *hw, int c, int64_t i, int32_t *map) {
    const int64_t n = off[c + 1] - off[c];
    if (i >= n) return;
    const int W = hw[2 * c + 1];
    int32_t qx, qy;
    rectify_map_pixel(cams + RECTIFY_CAM * c, (int)(i % W), (int)(i / W), &qx, &qy);
    map[2 * (off[c] + i)] = qx;
    map[2 * (off[c] + i) + 1] = qy;
}

// A ragged batch of frames and the maps they go through: frame c is H x W = hw[c] destination pixels at off[c], uses map
// map_index[c] (of the same H x W, at map_off[.] pixels), and reads a source of src_hw[c] at src_off[c] elements.
struct RectifyFrames {
    const int32_t *map;
    const int64_t *map_off;
    const int32_t *map_index;
    const int64_t *off;
    const int32_t *hw;
    const int64_t *src_off;
    const int32_t *src_hw;
    const int64_t *dst_off;                // bilinear: bytes, C times the pixels; nearest: unused, the elements are the pixels
};

// The first `bytes` bytes of WORDS little-endian words: whole dwords where the run is full and the address allows, as it
// does for every run of an image whose width is a multiple of 4.  Every index into w is a constant once the loops are
// unrolled, so the words stay in registers.
template <int WORDS> RECTIFY_HD void rectify_store(uint8_t *p, const uint32_t *w, int bytes) {
    if (bytes == 4 * WORDS && ((uintptr_t)p & 3) == 0) {
        uint8_t *p4 = (uint8_t *)__builtin_assume_aligned(p, 4);
#pragma unroll
        for (int k = 0; k < WORDS; ++k) memcpy(p4 + 4 * k, &w[k], 4);
    } else {
#pragma unroll
        for (int j = 0; j < 4 * WORDS; ++j)
            if (j < bytes) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

template <int C> RECTIFY_HD void rectify_remap_run(const uint8_t *src, int Hs, int Ws, const int32_t *m, int count, uint8_t *dst, uint8_t *valid) {
    uint32_t px[C], ok = 0;                // RECTIFY_RUN pixels of C bytes are C words, their validity one
    for (int k = 0; k < C; ++k) px[k] = 0;
#pragma unroll
    for (int k = 0; k < RECTIFY_RUN; ++k)
        if (k < count) {
            uint8_t v[C];
            ok |= rectify_bilinear<C>(src, Hs, Ws, m[2 * k], m[2 * k + 1], v) << (8 * k);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) px[(C * k + ch) >> 2] |= (uint32_t)v[ch] << (8 * ((C * k + ch) & 3));
        }
    rectify_store<C>(dst, px, count * C);
    rectify_store<1>(valid, &ok, count);
}

// rectify_remap_kernel: thread `run` of frame c, RECTIFY_RUN consecutive destination pixels of one row
RECTIFY_HD void rectify_remap_thread(const RectifyFrames *f, const uint8_t *src, int c, int64_t run, uint8_t *dst, uint8_t *valid) {
    const int H = f->hw[2 * c], W = f->hw[2 * c + 1], per_row = (W + RECTIFY_RUN - 1) / RECTIFY_RUN;
    if (run >= (int64_t)H * per_row) return;
    const int v = (int)(run / per_row), u0 = RECTIFY_RUN * (int)(run % per_row), count = W - u0 < RECTIFY_RUN ? W - u0 : RECTIFY_RUN;
    const int64_t px = (int64_t)v * W + u0, dst_bytes = f->dst_off[c + 1] - f->dst_off[c];
    const int32_t *m = f->map + 2 * (f->map_off[f->map_index[c]] + px);
    const uint8_t *s = src + f->src_off[c];
    const int Hs = f->src_hw[2 * c], Ws = f->src_hw[2 * c + 1];
    if (dst_bytes == f->off[c + 1] - f->off[c]) rectify_remap_run<1>(s, Hs, Ws, m, count, dst + f->dst_off[c] + px, valid + f->off[c] + px);
    else rectify_remap_run<3>(s, Hs, Ws, m, count, dst + f->dst_off[c] + 3 * px, valid + f->off[c] + px);
}

// rectify_nearest_kernel: thread i of frame c, one destination pixel; `mask` may be null, where it is 0 the output is 0
template <typename T> RECTIFY_HD void rectify_nearest_thread(const RectifyFrames *f, const T *src, const uint8_t *mask, int c, int64_t i, T *dst) {
    const int64_t n = f->off[c + 1] - f->off[c];
    if (i >= n) return;
    const int32_t *m = f->map + 2 * (f->map_off[f->map_index[c]] + i);
    const int64_t at = rectify_nearest_index(f->src_hw[2 * c], f->src_hw[2 * c + 1], m[0], m[1]);
    T out;
    memset(&out, 0, sizeof(T));
    if (at >= 0 && (!mask || mask[f->off[c] + i])) out = src[f->src_off[c] + at];
    dst[f->off[c] + i] = out;
}
