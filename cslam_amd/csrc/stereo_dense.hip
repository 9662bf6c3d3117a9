// stereo_dense.hip -- the stereo rule of stereo.h at EVERY pixel of a rectified pair, and the keyframe cloud made from it
// (gfx950).  The reference sends no cloud for a stereo frame (stereo_handler.cpp has no send_visualization_pointcloud of its
// own depth); this gives a swarm of stereo robots the map the RGB-D ones get from cloud.hip.
//
// A pixel's status, disparity and best are the bits feat_stereo_kernel (feat.hip) gives for a keypoint at that pixel: the
// rule is integer arithmetic up to one float64 division, so the order of the sums is free.  What the dense form shares:
//
//   products   C(u, d) = SA(u) + SB(u - d) - 2 P(u, d): SA, SB the 15 x 3 sums of squares of the left and the right window,
//              once per column; P the 15 x 3 sum of products.  A column's three rows are the three bytes of one word, so a
//              column's share of P is one v_dot4_u32_u8, and P runs along the columns: add the column that enters, take
//              off the one that leaves (its product waits in a ring of 15 registers, the walk is unrolled).
//   back search  the right pixel ur searches C(ur + e, e) over e, whichever left pixel asks: every cost is read once more
//              along its diagonal, and the lowest key of ur is kept in rkey (int32 per pixel).
//
// stereo_dense_kernel: one workgroup of 256 threads per image row.  The row is walked in tiles of T = 256 columns and, inside
// one, the disparities in tiles of TD = 32, ascending.  Every phase is a function of one thread over plain arrays in
// stereo_dense.h, which the host tests run in this schedule on the CPU; the kernel below is the schedule: the barriers, the
// registers that live across them, and the stores.  Per (column tile, disparity tile):
//   costs   thread (d, segment of 32 columns) walks its segment (14 columns of run-in, 46 products for 32 costs) and writes
//           the costs to an LDS slab [TD][T + 1] (33 KB; the odd stride spreads the 32 disparities of a wave over the banks).
//   left    thread u reads its column of the slab in ascending d into its book (stereo_dense.h): registers only.
//   right   thread ur reads its diagonal of the slab and lowers rkey[ur].  A right pixel belongs to one thread per tile pair,
//           and a barrier separates the pairs: no atomics.
// After a column tile the book gives status, best, disparity and depth but for the left-right check, and d* of the pixels
// that still await it goes to dstar (int16 per pixel).  After the last tile every right pixel of the row is complete (the
// costs it needs lie up to max_disparity + 1 columns to its right, so no order of the tiles would have it earlier) and one
// more pass over the row marks the left-right failures.
// Left pixels without a range (u - 7 - D_lo < 2) have costs all the same: the slab is uniform in u, the back search of the
// right pixels 7, 8, ... needs them.  Columns outside the image are staged as zeros and their costs are never read.
// rkey and dstar (6 bytes per pixel) are written and read back by the one workgroup that owns the row; rkey is read and
// rewritten once per pair of tiles (T + TD - 1 keys), 66 bytes per pixel at 640 columns and 130 disparities, which a row's
// 2.5 KB keep in L2.  The window of T + max_disparity + 1 live keys would fit in LDS; the finished ones would still have to
// leave the chip for the pass after the row.
//
// LDS 38 KB per workgroup: four workgroups, 16 waves per CU.  Nothing depends on another row or frame: a frame gives the
// same bytes alone or in any batch.
#include "common.h"
// before stereo.h and stereo_dense.h: their float64 expressions (parabola, point) hold no a * b + c, and none may appear
#pragma clang fp contract(off)
#include "feat_args.h"
#include "stereo_dense.h"
#define CLOUD_HD __host__ __device__
#include "cloud.h"                 // CLOUD_DEPTH_F32

#define SD_T STEREO_DENSE_T

__global__ __launch_bounds__(SD_T) void stereo_dense_kernel(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right,
                                                            const int64_t *__restrict__ off, const int32_t *__restrict__ hw,
                                                            const double *__restrict__ cams, StereoParams P, float *__restrict__ disparity,
                                                            uint8_t *__restrict__ status, float *__restrict__ depth,
                                                            int32_t *__restrict__ best, int32_t *rkey, int16_t *dstar) {
    __shared__ int32_t s_slab[STEREO_DENSE_SLAB];
    __shared__ uint32_t s_l[STEREO_DENSE_LW], s_r[STEREO_DENSE_RW], s_sa[SD_T], s_sb[STEREO_DENSE_SBW];
    const int c = blockIdx.y, v = blockIdx.x, t = threadIdx.x;
    const int64_t base = off[c];
    const int H = hw[2 * c], W = hw[2 * c + 1];
    if (v >= H) return;                                    // the whole workgroup leaves
    const int64_t row = base + (int64_t)v * W;
    if (!stereo_dense_row_searched(v, H, W)) {
        for (int u = t; u < W; u += SD_T) {
            status[row + u] = STEREO_OUTSIDE;
            disparity[row + u] = NAN;
            depth[row + u] = NAN;
            if (best) for (int k = 0; k < 4; ++k) best[4 * (row + u) + k] = -1;
        }
        return;
    }
    const StereoDenseRow q = {left + base, right + base, H, W, v, P.min_disparity, P.max_disparity, P.uniqueness, P.lr_tolerance};
    const StereoDenseTile s = {s_l, s_r, s_sa, s_sb, s_slab};
    const int n_dt = stereo_dense_d_tiles(P.min_disparity, P.max_disparity), d_lo = P.min_disparity - 1;
    for (int u = t; u < W; u += SD_T) rkey[row + u] = STEREO_DENSE_NO_KEY;
    for (int u0 = 0; u0 < W; u0 += SD_T) {
        __syncthreads();                                   // the tile before is done with the LDS; rkey's start values are in place
        stereo_dense_stage(&q, &s, u0, t);
        __syncthreads();
        stereo_dense_squares(&q, &s, t);
        StereoDenseBook bk;
        stereo_dense_book_init(&bk);
        for (int dt = 0; dt < n_dt; ++dt) {
            const int e0 = d_lo + dt * STEREO_DENSE_TD;
            __syncthreads();                               // SA, SB are written; the slab has been read
            stereo_dense_costs(&q, &s, u0, e0, t);
            __syncthreads();
            stereo_dense_left(&q, &s, u0, e0, t, &bk);
            stereo_dense_right(&q, &s, u0, e0, t, rkey + row);
        }
        const int u = u0 + t;
        if (u < W) {
            const StereoDensePixel r = stereo_dense_pixel(&q, &bk, u, cams + 5 * c);
            status[row + u] = (uint8_t)r.status;
            disparity[row + u] = r.disparity;
            depth[row + u] = r.depth;
            dstar[row + u] = (int16_t)r.await;
            if (best) { best[4 * (row + u)] = r.ds; best[4 * (row + u) + 1] = r.ca; best[4 * (row + u) + 2] = r.cb; best[4 * (row + u) + 3] = r.cc; }
        }
    }
    __syncthreads();                                       // every right pixel of the row is complete
    for (int u = t; u < W; u += SD_T) {                    // u's own thread wrote dstar[u]
        const int ds = dstar[row + u];
        if (ds >= 0 && stereo_dense_left_right_fails(&q, rkey + row, u, ds)) {
            status[row + u] = STEREO_LEFT_RIGHT;
            disparity[row + u] = NAN;
            depth[row + u] = NAN;
        }
    }
}

// the (fx, fy, cx, cy) of the stereo cameras, as the cloud kernels take them
__global__ void stereo_dense_cam4_kernel(const double *__restrict__ cam5, int n, double *__restrict__ cam4) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * n) cam4[i] = cam5[5 * (i / 4) + i % 4];
}

// ---- host side -----------------------------------------------------------------------------------------------------
static StreamScratch g_dense_scratch, g_dense_chain_scratch;

static int dense_launch(const uint8_t *left, const uint8_t *right, const int64_t *off, const int32_t *hw, int n, const FeatShape &sh,
                        const double *cams, const StereoParams &P, float *disparity, uint8_t *status, float *depth, int32_t *best,
                        hipStream_t st) {
    int32_t *rkey;
    int16_t *dstar;
    auto layout = [&](Carver &cv) {
        rkey = cv.take<int32_t>((size_t)sh.px.total);
        dstar = cv.take<int16_t>((size_t)sh.px.total);
    };
    SCRATCH_CARVE(g_dense_scratch, st, (size_t)1 << 20, layout);
    hipLaunchKernelGGL(stereo_dense_kernel, dim3((unsigned)sh.max_h, (unsigned)n), dim3(STEREO_DENSE_T), 0, st, left, right, off, hw, cams, P, disparity,
                       status, depth, best, rkey, dstar);
    return CSLAM_OK;
}

CSLAM_API int cslam_stereo_dense_dev(const uint8_t *d_left, const uint8_t *d_right, const int64_t *d_off, const int32_t *d_hw, int n,
                                     const double *d_cameras, int min_disparity, int max_disparity, int uniqueness, int lr_tolerance,
                                     float *d_disparity, uint8_t *d_status, float *d_depth, int32_t *d_best, const int64_t *h_off,
                                     const int32_t *h_hw, const double *h_cameras, void *stream) {
    FeatShape sh;
    const StereoParams P = {min_disparity, max_disparity, uniqueness, lr_tolerance};
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_stereo_checks(P, h_cameras, n))) return rc;
    ARG_CHECK(d_left && d_right && d_off && d_hw && d_cameras && d_disparity && d_status && d_depth, "NULL argument");
    PTR_DEVICE(d_left);
    if ((rc = dense_launch(d_left, d_right, d_off, d_hw, n, sh, d_cameras, P, d_disparity, d_status, d_depth, d_best, (hipStream_t)stream)))
        return rc;
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_cloud_keyframes_stereo_dev(const uint8_t *d_left, const int64_t *d_left_off, int channels, const uint8_t *d_right,
                                               const int64_t *d_right_off, const int64_t *d_off, const int32_t *d_hw,
                                               const double *d_cameras, int n, int min_disparity, int max_disparity, int uniqueness,
                                               int lr_tolerance, double leaf, double max_range, float *d_out, uint32_t *d_out_rgb,
                                               int32_t *d_counts, int64_t *d_out_offsets, int32_t *d_status, const int64_t *h_left_off,
                                               const int64_t *h_right_off, const int64_t *h_off, const int32_t *h_hw,
                                               const double *h_cameras, void *stream) {
    FeatShape sh;
    const StereoParams P = {min_disparity, max_disparity, uniqueness, lr_tolerance};
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = feat_src_check(h_left_off, h_off, n))) return rc;
    if ((rc = feat_src_check(h_right_off, h_off, n))) return rc;
    if ((rc = feat_stereo_checks(P, h_cameras, n))) return rc;
    ARG_CHECK(leaf > 0.0 && leaf < INFINITY, "voxel must be positive and finite");
    ARG_CHECK(max_range >= 0.0, "max_range must not be negative or NaN");
    ARG_CHECK(channels == 1 || channels == 3, "channels must be 1 or 3");
    for (int c = 0; c < n; ++c)
        ARG_CHECK(h_left_off[c + 1] - h_left_off[c] == channels * (h_off[c + 1] - h_off[c]), "every left image has `channels` channels");
    ARG_CHECK(d_left && d_left_off && d_right && d_right_off && d_off && d_hw && d_cameras && d_out && d_out_rgb && d_counts && d_out_offsets &&
                  d_status,
              "NULL argument");
    PTR_DEVICE(d_left);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *gray_l, *gray_r, *status;
    float *disparity, *depth;
    double *cam4;
    auto layout = [&](Carver &cv) {
        gray_l = cv.take<uint8_t>((size_t)sh.px.total);
        gray_r = cv.take<uint8_t>((size_t)sh.px.total);
        status = cv.take<uint8_t>((size_t)sh.px.total);
        disparity = cv.take<float>((size_t)sh.px.total);
        depth = cv.take<float>((size_t)sh.px.total);
        cam4 = cv.take<double>((size_t)4 * n);
    };
    SCRATCH_CARVE(g_dense_chain_scratch, st, (size_t)1 << 20, layout);
    if ((rc = cslam_feat_gray_dev(d_left, d_left_off, d_off, d_hw, n, gray_l, h_left_off, h_off, h_hw, stream))) return rc;
    if ((rc = cslam_feat_gray_dev(d_right, d_right_off, d_off, d_hw, n, gray_r, h_right_off, h_off, h_hw, stream))) return rc;
    if ((rc = dense_launch(gray_l, gray_r, d_off, d_hw, n, sh, d_cameras, P, disparity, status, depth, nullptr, st))) return rc;
    hipLaunchKernelGGL(stereo_dense_cam4_kernel, dim3((unsigned)ceil_div64(4 * (int64_t)n, 256)), dim3(256), 0, st, d_cameras, n, cam4);
    HIP_TRY(hipGetLastError());
    return cslam_cloud_keyframes_dev(d_left, channels, depth, CLOUD_DEPTH_F32, d_off, d_hw, cam4, n, leaf, max_range, d_out, d_out_rgb,
                                     d_counts, d_out_offsets, d_status, h_off, h_hw, stream);
}
