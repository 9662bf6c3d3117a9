// rectify.hip -- undistort and rectify raw camera frames (gfx950): what image_proc / stereo_image_proc do in front of the
// reference (OpenCV initUndistortRectifyMap + remap; stereo_handler.cpp:120 hard-codes alreadyRectified = true), so that a
// camera driver's frames can enter the visual stages of feat.hip, stereo_dense.hip and cloud.hip without leaving the device.
// The rule is rectify.h's; every kernel here is its index arithmetic and one call of a per-thread function there, which
// the host tests run in the same schedule.
//
//   rectify_map_kernel      a thread per destination pixel of a ragged batch of cameras: float64, one (qx, qy) pair stored,
//                           no atomics.  Made once per camera and kept on the device.
//   rectify_remap_kernel    a ragged batch of frames, each naming its map by an index (many frames share one map), 1 or 3
//                           channels each.  A thread owns RECTIFY_RUN = 4 consecutive destination pixels of one row: 32
//                           bytes of map, and one dword of image per channel and one of validity where the row allows (a
//                           width that is a multiple of 4; otherwise bytes).  The taps are byte loads served by L2: the rule
//                           does not bound the footprint of a tile (a rotation or a strong distortion spreads it), so the
//                           source is not staged in LDS.
//   rectify_nearest_kernel  depth, uint16 or float32, a thread per destination pixel; with a mask (the validity map of the
//                           colour image through the same map) a masked pixel is 0.
//
// Nothing depends on another frame: a frame gives the same bytes alone, in any batch and in any order.
#include "common.h"
// before rectify.h: the map is compared bit for bit with a restatement that rounds every product and sum on its own
#pragma clang fp contract(off)
#include "feat_args.h"
#include "rectify.h"

__global__ __launch_bounds__(RECTIFY_BLOCK) void rectify_map_kernel(const double *__restrict__ cams, const int64_t *__restrict__ off,
                                                                    const int32_t *__restrict__ hw, int32_t *__restrict__ map) {
    rectify_map_thread(cams, off, hw, blockIdx.y, (int64_t)blockIdx.x * RECTIFY_BLOCK + threadIdx.x, map);
}

__global__ __launch_bounds__(RECTIFY_BLOCK) void rectify_remap_kernel(RectifyFrames f, const uint8_t *__restrict__ src,
                                                                      uint8_t *__restrict__ dst, uint8_t *__restrict__ valid) {
    rectify_remap_thread(&f, src, blockIdx.y, (int64_t)blockIdx.x * RECTIFY_BLOCK + threadIdx.x, dst, valid);
}

template <typename T>
__global__ __launch_bounds__(RECTIFY_BLOCK) void rectify_nearest_kernel(RectifyFrames f, const T *__restrict__ src,
                                                                        const uint8_t *__restrict__ mask, T *__restrict__ dst) {
    rectify_nearest_thread<T>(&f, src, mask, blockIdx.y, (int64_t)blockIdx.x * RECTIFY_BLOCK + threadIdx.x, dst);
}

// ---- host side -----------------------------------------------------------------------------------------------------
static int rectify_camera_checks(const double *h_cams, int n) {
    ARG_CHECK(h_cams != nullptr, "h_cameras is required");
    for (int c = 0; c < n; ++c) {
        const double *cam = h_cams + RECTIFY_CAM * c, *R = cam + 12;
        for (int k = 0; k < RECTIFY_CAM; ++k) ARG_CHECK(isfinite(cam[k]), "a raw camera (K, D, R, P) must be finite");
        ARG_CHECK(cam[0] > 0.0 && cam[1] > 0.0 && cam[21] > 0.0 && cam[22] > 0.0, "the focal lengths of K and P must be positive");
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double dot = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2];
                ARG_CHECK(fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9, "R must be orthonormal to 1e-9");
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        ARG_CHECK(det > 0.0, "R must be a rotation (positive determinant)");
    }
    return CSLAM_OK;
}

// the frames' destinations, their maps and their sources: `elems` = admitted source elements per pixel (1, or 1 and 3)
static int rectify_frame_checks(const int64_t *h_off, const int32_t *h_hw, int n, const int64_t *h_map_off, const int32_t *h_map_hw, int n_maps,
                                const int32_t *h_map_index, const int64_t *h_src_off, const int32_t *h_src_hw, bool three, FeatShape *sh) {
    FeatShape maps;
    int rc = feat_shape(h_off, h_hw, n, sh);
    if (rc) return rc;
    BATCH_COUNT_CHECK(n_maps);
    if ((rc = feat_shape(h_map_off, h_map_hw, n_maps, &maps))) return rc;
    ARG_CHECK(h_map_index != nullptr && h_src_off != nullptr && h_src_hw != nullptr, "h_map_index, h_src_off and h_src_hw are required");
    RaggedShape src;
    if ((rc = offsets_check(h_src_off, n, &src))) return rc;
    for (int c = 0; c < n; ++c) {
        const int m = h_map_index[c];
        ARG_CHECK(m >= 0 && m < n_maps, "a map index must name one of the maps");
        ARG_CHECK(h_hw[2 * c] == h_map_hw[2 * m] && h_hw[2 * c + 1] == h_map_hw[2 * m + 1], "a frame's destination has the size of its map");
        const int64_t Hs = h_src_hw[2 * c], Ws = h_src_hw[2 * c + 1], len = h_src_off[c + 1] - h_src_off[c];
        ARG_CHECK(Hs >= 2 && Ws >= 2, "a source image is at least 2 x 2");
        ARG_CHECK(Hs * Ws <= FEAT_MAX_PIXELS, "an image has at most 2^30 pixels");
        ARG_CHECK(len == Hs * Ws || (three && len == 3 * Hs * Ws), three ? "a source image has 1 channel or 3 (BGR)" : "a depth image has 1 channel");
    }
    return CSLAM_OK;
}

CSLAM_API int cslam_rectify_map_dev(const double *d_cameras, const int64_t *d_off, const int32_t *d_hw, int n, int32_t *d_map,
                                    const int64_t *h_off, const int32_t *h_hw, const double *h_cameras, void *stream) {
    FeatShape sh;
    int rc = feat_shape(h_off, h_hw, n, &sh);
    if (rc) return rc;
    if ((rc = rectify_camera_checks(h_cameras, n))) return rc;
    ARG_CHECK(d_cameras && d_off && d_hw && d_map, "NULL argument");
    PTR_DEVICE(d_map);
    hipLaunchKernelGGL(rectify_map_kernel, dim3((unsigned)ceil_div64(sh.px.largest, RECTIFY_BLOCK), (unsigned)n), dim3(RECTIFY_BLOCK), 0,
                       (hipStream_t)stream, d_cameras, d_off, d_hw, d_map);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_rectify_remap_dev(const uint8_t *d_src, const int64_t *d_src_off, const int32_t *d_src_hw, const int32_t *d_map,
                                      const int64_t *d_map_off, const int32_t *d_map_index, int n_maps, const int64_t *d_off,
                                      const int32_t *d_hw, int n, uint8_t *d_dst, const int64_t *d_dst_off, uint8_t *d_valid,
                                      const int64_t *h_src_off, const int32_t *h_src_hw, const int64_t *h_map_off, const int32_t *h_map_hw,
                                      const int32_t *h_map_index, const int64_t *h_off, const int32_t *h_hw, const int64_t *h_dst_off,
                                      void *stream) {
    FeatShape sh;
    int rc = rectify_frame_checks(h_off, h_hw, n, h_map_off, h_map_hw, n_maps, h_map_index, h_src_off, h_src_hw, true, &sh);
    if (rc) return rc;
    ARG_CHECK(h_dst_off != nullptr, "h_dst_off is required");
    RaggedShape dsts;
    if ((rc = offsets_check(h_dst_off, n, &dsts))) return rc;
    int64_t most_runs = 0;
    for (int c = 0; c < n; ++c) {
        const int64_t px = h_off[c + 1] - h_off[c], channels = (h_src_off[c + 1] - h_src_off[c]) / ((int64_t)h_src_hw[2 * c] * h_src_hw[2 * c + 1]);
        ARG_CHECK(h_dst_off[c + 1] - h_dst_off[c] == channels * px, "a rectified image has the channels of its source");
        const int64_t runs = (int64_t)h_hw[2 * c] * ceil_div64(h_hw[2 * c + 1], RECTIFY_RUN);
        if (runs > most_runs) most_runs = runs;
    }
    ARG_CHECK(d_src && d_src_off && d_src_hw && d_map && d_map_off && d_map_index && d_off && d_hw && d_dst && d_dst_off && d_valid,
              "NULL argument");
    PTR_DEVICE(d_src);
    const RectifyFrames f = {d_map, d_map_off, d_map_index, d_off, d_hw, d_src_off, d_src_hw, d_dst_off};
    hipLaunchKernelGGL(rectify_remap_kernel, dim3((unsigned)ceil_div64(most_runs, RECTIFY_BLOCK), (unsigned)n), dim3(RECTIFY_BLOCK), 0,
                       (hipStream_t)stream, f, d_src, d_dst, d_valid);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_rectify_nearest_dev(const void *d_src, int src_type, const int64_t *d_src_off, const int32_t *d_src_hw,
                                        const int32_t *d_map, const int64_t *d_map_off, const int32_t *d_map_index, int n_maps,
                                        const int64_t *d_off, const int32_t *d_hw, int n, const uint8_t *d_mask, void *d_dst,
                                        const int64_t *h_src_off, const int32_t *h_src_hw, const int64_t *h_map_off, const int32_t *h_map_hw,
                                        const int32_t *h_map_index, const int64_t *h_off, const int32_t *h_hw, void *stream) {
    FeatShape sh;
    int rc = rectify_frame_checks(h_off, h_hw, n, h_map_off, h_map_hw, n_maps, h_map_index, h_src_off, h_src_hw, false, &sh);
    if (rc) return rc;
    ARG_CHECK(src_type == CSLAM_RECTIFY_U16 || src_type == CSLAM_RECTIFY_F32, "src_type must be 0 (uint16) or 1 (float32)");
    ARG_CHECK(d_src && d_src_off && d_src_hw && d_map && d_map_off && d_map_index && d_off && d_hw && d_dst, "NULL argument");
    PTR_DEVICE(d_src);
    const RectifyFrames f = {d_map, d_map_off, d_map_index, d_off, d_hw, d_src_off, d_src_hw, nullptr};
    const dim3 grid((unsigned)ceil_div64(sh.px.largest, RECTIFY_BLOCK), (unsigned)n), block(RECTIFY_BLOCK);
    if (src_type == CSLAM_RECTIFY_U16)
        hipLaunchKernelGGL(rectify_nearest_kernel<uint16_t>, grid, block, 0, (hipStream_t)stream, f, (const uint16_t *)d_src, d_mask, (uint16_t *)d_dst);
    else
        hipLaunchKernelGGL(rectify_nearest_kernel<float>, grid, block, 0, (hipStream_t)stream, f, (const float *)d_src, d_mask, (float *)d_dst);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}
