// stereo_dense.h -- the dense stereo kernel (stereo_dense.hip) as what ONE thread does in each of its phases, written over
// plain arrays: the kernel calls these with its LDS between barriers, the host tests call them thread after thread with
// arrays of the same sizes (compiled for the host with __host__ / __device__ defined away, as stereo.h is), so the tile plan
// and every index below run on the CPU, under the host compiler's sanitizers.  The rule itself (window, key, range,
// uniqueness, parabola, point) is stereo.h's; nothing of it is restated here.
//
//   tiles       a workgroup of STEREO_DENSE_T threads walks one image row in tiles of STEREO_DENSE_T columns and, inside a
//               column tile, the range D_lo .. max_disparity + 1 in tiles of STEREO_DENSE_TD disparities, ascending
//   words       rows v - 1 .. v + 1 of a column are the three low bytes of one word, 0 outside the image; the product of two
//               columns is one dot4
//   costs       C(u, d) = SA(u) + SB(u - d) - 2 P(u, d): SA, SB the sums of squares of the left and the right window, P the
//               sum of products; thread (d, segment) walks STEREO_DENSE_WALK columns, adds the column that enters the window
//               and takes off the one that leaves (a ring of 15 products), and writes STEREO_DENSE_SEG costs to the slab
//   book        what a left pixel keeps in registers while its costs go by in ascending d: the four smallest keys, sorted
//               (m[0] is the best), the cost before the best and the cost after it
//   rival       the lowest cost at |d - d*| >= 2 is the first of m[1 .. 3] that is a key and lies that far from d*: d* - 1 and
//               d* + 1 are the only ones left out, so one of the three qualifies whenever the range holds four disparities
//   back span   the disparities e of one disparity tile whose cost C(ur + e, e) lies in one column tile: the share of the
//               right pixel ur's search that this (column tile, disparity tile) holds
#pragma once
#include <math.h>
#include "stereo.h"

#define STEREO_DENSE_T 256         // columns per tile = threads per workgroup
#define STEREO_DENSE_TD 32         // disparities per tile
#define STEREO_DENSE_SEG 32        // columns one thread sums along for one disparity
#define STEREO_DENSE_NO_KEY 0x7fffffff
#define STEREO_DENSE_STRIDE (STEREO_DENSE_T + 1)                            // words per disparity of the cost slab
#define STEREO_DENSE_LW (STEREO_DENSE_T + 2 * STEREO_HALF_W)                // left columns staged for a tile
#define STEREO_DENSE_RW (STEREO_DENSE_LW + STEREO_MAX_RANGE - 1)            // right columns: up to 256 disparities further left
#define STEREO_DENSE_SBW (STEREO_DENSE_RW - 2 * STEREO_HALF_W)              // right columns with a whole window staged
#define STEREO_DENSE_WALK (STEREO_DENSE_SEG + 2 * STEREO_HALF_W)            // 46 columns give the 32 windows of a segment
#define STEREO_DENSE_SLAB (STEREO_DENSE_TD * STEREO_DENSE_STRIDE)

// one image row of one frame and the parameters
struct StereoDenseRow { const uint8_t *L, *R; int H, W, v, min_disparity, max_disparity, uniqueness, lr_tolerance; };
// the arrays of a workgroup: l [LW], r [RW], sa [T], sb [SBW], slab [SLAB]
struct StereoDenseTile { uint32_t *l, *r, *sa, *sb; int32_t *slab; };
struct StereoDenseBook { int32_t m[4]; int32_t prev, ca, cc; };
// what a pixel gets; await = d* while the left-right check is still to come, otherwise -1
struct StereoDensePixel { int status, ds, await; int32_t ca, cb, cc; float disparity, depth; };

// the sum of the products of the three rows of two columns
STEREO_HD uint32_t stereo_dense_dot(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
    return (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u);
#endif
}

STEREO_HD uint32_t stereo_dense_column(const uint8_t *img, int W, int v, int x) {
    if (x < 0 || x >= W) return 0u;
    const uint8_t *p = img + (int64_t)(v - STEREO_HALF_H) * W + x;
    return (uint32_t)p[0] | (uint32_t)p[W] << 8 | (uint32_t)p[2 * (int64_t)W] << 16;
}

// rows 1 .. H - 2 of an image wide enough for one window are searched; every pixel of another row is outside
STEREO_HD bool stereo_dense_row_searched(int v, int H, int W) {
    return v >= STEREO_HALF_H && v <= H - 1 - STEREO_HALF_H && W >= STEREO_WIN_W;
}

// disparity tiles that cover D_lo .. max_disparity + 1
STEREO_HD int stereo_dense_d_tiles(int min_disparity, int max_disparity) {
    return (max_disparity + 1 - (min_disparity - 1)) / STEREO_DENSE_TD + 1;
}

// the right column of r[0] for the column tile at u0; r holds STEREO_DENSE_LW + D_hi - D_lo columns from there
STEREO_HD int stereo_dense_r_base(const StereoDenseRow *q, int u0) { return u0 - STEREO_HALF_W - (q->max_disparity + 1); }
STEREO_HD int stereo_dense_r_width(const StereoDenseRow *q) { return STEREO_DENSE_LW + q->max_disparity + 1 - (q->min_disparity - 1); }

// ---- phase: stage.  l[i] = left column u0 - 7 + i, r[i] = right column r_base + i
STEREO_HD void stereo_dense_stage(const StereoDenseRow *q, const StereoDenseTile *s, int u0, int t) {
    const int rw = stereo_dense_r_width(q), r_base = stereo_dense_r_base(q, u0);
    for (int i = t; i < STEREO_DENSE_LW; i += STEREO_DENSE_T) s->l[i] = stereo_dense_column(q->L, q->W, q->v, u0 - STEREO_HALF_W + i);
    for (int i = t; i < rw; i += STEREO_DENSE_T) s->r[i] = stereo_dense_column(q->R, q->W, q->v, r_base + i);
}

// ---- phase: squares.  sa[j] = SA of left column u0 + j, sb[i] = SB of right column r_base + 7 + i
STEREO_HD void stereo_dense_squares(const StereoDenseRow *q, const StereoDenseTile *s, int t) {
    const int n = stereo_dense_r_width(q) - 2 * STEREO_HALF_W;
    uint32_t a = 0;
    for (int k = 0; k < STEREO_WIN_W; ++k) a += stereo_dense_dot(s->l[t + k], s->l[t + k]);
    s->sa[t] = a;
    for (int i = t; i < n; i += STEREO_DENSE_T) {
        uint32_t b = 0;
        for (int k = 0; k < STEREO_WIN_W; ++k) b += stereo_dense_dot(s->r[i + k], s->r[i + k]);
        s->sb[i] = b;
    }
}

// ---- phase: costs.  slab[d - e0][j] = C(u0 + j, d) for this thread's d and segment; nothing for a disparity past
// max_disparity + 1 or a segment past the last column that has a window (no later phase reads those)
STEREO_HD void stereo_dense_costs(const StereoDenseRow *q, const StereoDenseTile *s, int u0, int e0, int t) {
    const int dd = t % STEREO_DENSE_TD, js = (t / STEREO_DENSE_TD) * STEREO_DENSE_SEG, d = e0 + dd, d_max = q->max_disparity + 1;
    if (d > d_max || u0 + js > q->W - 1 - STEREO_HALF_W) return;
    const uint32_t *pl = s->l + js, *pr = s->r + js + d_max - d, *sa = s->sa + js, *sb = s->sb + js + d_max - d;
    int32_t *out = s->slab + dd * STEREO_DENSE_STRIDE + js;
    uint32_t ring[STEREO_WIN_W], p = 0;
#pragma unroll
    for (int i = 0; i < STEREO_DENSE_WALK; ++i) {
        const uint32_t x = stereo_dense_dot(pl[i], pr[i]);
        if (i >= STEREO_WIN_W) p -= ring[i % STEREO_WIN_W];
        ring[i % STEREO_WIN_W] = x;
        p += x;
        if (i >= STEREO_WIN_W - 1) {
            const int j = i - (STEREO_WIN_W - 1);
            out[j] = (int32_t)(sa[j] + sb[j] - 2u * p);
        }
    }
}

// ---- phase: left.  the book of left column u0 + t takes its costs of this disparity tile
STEREO_HD void stereo_dense_book_init(StereoDenseBook *b) {
    for (int i = 0; i < 4; ++i) b->m[i] = STEREO_DENSE_NO_KEY;
    b->prev = b->ca = b->cc = -1;
}

// the cost of the next disparity d (ascending, without gaps)
STEREO_HD void stereo_dense_book_take(StereoDenseBook *b, int32_t cost, int d) {
    int32_t key = stereo_key(cost, d);
    if (key < b->m[0]) {                                   // a new best: its left neighbour is known, its right one not yet
        b->ca = b->prev;
        b->cc = -1;
    } else if (d == stereo_key_d(b->m[0]) + 1) {
        b->cc = cost;
    }
    b->prev = cost;
    for (int i = 0; i < 4; ++i) {                          // sorted insertion; the largest of the five falls out
        const int32_t lo = key < b->m[i] ? key : b->m[i];
        key = key < b->m[i] ? b->m[i] : key;
        b->m[i] = lo;
    }
}

STEREO_HD void stereo_dense_left(const StereoDenseRow *q, const StereoDenseTile *s, int u0, int e0, int t, StereoDenseBook *b) {
    int d_lo, d_hi;
    const int u = u0 + t;
    if (!stereo_inside(u, q->v, q->H, q->W) || !stereo_range(u, q->min_disparity, q->max_disparity, &d_lo, &d_hi)) return;
    const int last = d_hi - e0 < STEREO_DENSE_TD - 1 ? d_hi - e0 : STEREO_DENSE_TD - 1;
    for (int dd = 0; dd <= last; ++dd) stereo_dense_book_take(b, s->slab[dd * STEREO_DENSE_STRIDE + t], e0 + dd);
}

// ---- phase: right.  e_lo .. e_hi (empty when e_lo > e_hi): the disparities e of the tile e0 .. e0 + TD - 1 that the right
// pixel ur searches and whose left column ur + e lies in the column tile u0 .. u0 + T - 1
STEREO_HD void stereo_dense_back_span(int ur, int W, int min_disparity, int max_disparity, int u0, int e0, int *e_lo, int *e_hi) {
    int lo = min_disparity - 1, hi = stereo_range_back(ur, W, max_disparity);
    if (lo < e0) lo = e0;
    if (lo < u0 - ur) lo = u0 - ur;
    if (hi > e0 + STEREO_DENSE_TD - 1) hi = e0 + STEREO_DENSE_TD - 1;
    if (hi > u0 + STEREO_DENSE_T - 1 - ur) hi = u0 + STEREO_DENSE_T - 1 - ur;
    *e_lo = lo;
    *e_hi = hi;
}

// rkey [W]: the lowest key of every right pixel of the row so far.  The T + TD - 1 right pixels whose diagonal crosses this
// pair of tiles belong to one thread each.
STEREO_HD void stereo_dense_right(const StereoDenseRow *q, const StereoDenseTile *s, int u0, int e0, int t, int32_t *rkey) {
    for (int k = t; k < STEREO_DENSE_T + STEREO_DENSE_TD - 1; k += STEREO_DENSE_T) {
        const int ur = u0 - e0 - (STEREO_DENSE_TD - 1) + k;
        if (ur < STEREO_HALF_W || ur > q->W - 1 - STEREO_HALF_W) continue;
        int e_lo, e_hi;
        stereo_dense_back_span(ur, q->W, q->min_disparity, q->max_disparity, u0, e0, &e_lo, &e_hi);
        if (e_lo > e_hi) continue;
        int32_t low = rkey[ur];
        for (int e = e_lo; e <= e_hi; ++e) {
            const int32_t key = stereo_key(s->slab[(e - e0) * STEREO_DENSE_STRIDE + ur + e - u0], e);
            low = key < low ? key : low;
        }
        rkey[ur] = low;
    }
}

// ---- after the last disparity tile of a column tile: the pixel but for the left-right check
// the lowest cost at |d - d*| >= 2, or STEREO_DENSE_NO_KEY when the range holds none
STEREO_HD int32_t stereo_dense_rival(const StereoDenseBook *b) {
    const int ds = stereo_key_d(b->m[0]);
    int32_t second = STEREO_DENSE_NO_KEY;
    for (int i = 3; i >= 1; --i) {
        const int dd = stereo_key_d(b->m[i]) - ds;
        if (b->m[i] != STEREO_DENSE_NO_KEY && (dd >= 2 || dd <= -2)) second = stereo_key_cost(b->m[i]);
    }
    return second;
}

STEREO_HD StereoDensePixel stereo_dense_pixel(const StereoDenseRow *q, const StereoDenseBook *b, int u, const double *cam) {
    StereoDensePixel r = {STEREO_OUTSIDE, -1, -1, -1, -1, -1, NAN, NAN};
    int d_lo, d_hi;
    if (!stereo_inside(u, q->v, q->H, q->W)) return r;
    r.status = STEREO_NO_RANGE;
    if (!stereo_range(u, q->min_disparity, q->max_disparity, &d_lo, &d_hi)) return r;
    r.ds = stereo_key_d(b->m[0]);
    r.ca = b->ca;
    r.cb = stereo_key_cost(b->m[0]);
    r.cc = b->cc;
    const int32_t second = stereo_dense_rival(b);
    if (r.ds == d_lo || r.ds == d_hi) r.status = STEREO_EDGE;
    else if (second != STEREO_DENSE_NO_KEY && stereo_not_unique(second, r.cb, q->uniqueness)) r.status = STEREO_NOT_UNIQUE;
    else {
        double p[3];
        const double d = stereo_parabola(r.ds, r.ca, r.cb, r.cc);
        stereo_point(u, q->v, d, cam[0], cam[1], cam[2], cam[3], cam[4], p);
        r.status = STEREO_ACCEPTED;
        r.disparity = (float)d;
        r.depth = (float)p[2];
        if (q->lr_tolerance >= 0) r.await = r.ds;
    }
    return r;
}

// ---- after the last column tile: every right pixel of the row is complete.  ds = the pixel's awaiting d* >= 0
STEREO_HD bool stereo_dense_left_right_fails(const StereoDenseRow *q, const int32_t *rkey, int u, int ds) {
    const int es = stereo_key_d(rkey[u - ds]);             // u - ds >= 8: ds < D_hi <= u - 7
    return (es > ds ? es - ds : ds - es) > q->lr_tolerance;
}
