// feat_args.h -- the host-side argument checks of the image entry points, written once for feat.hip (features, sparse
// stereo) and stereo_dense.hip (dense stereo): the shape of a ragged batch of images, the channels of its sources, the
// stereo parameters and cameras.  Included after common.h.
#pragma once
#include "stereo.h"

#define FEAT_TILE 16
#define FEAT_MAX_PIXELS ((int64_t)1 << 30)

struct StereoParams { int min_disparity, max_disparity, uniqueness, lr_tolerance; };

struct FeatShape { RaggedShape px; int max_h, max_w; };

// the host copies are required: they size the launches.  Every image is H x W = its rows of the offsets.
static int feat_shape(const int64_t *h_off, const int32_t *h_hw, int n, FeatShape *s) {
    BATCH_COUNT_CHECK(n);
    ARG_CHECK(h_off != nullptr && h_hw != nullptr, "h_off and h_hw are required");
    int rc = offsets_check(h_off, n, &s->px);
    if (rc) return rc;
    s->max_h = s->max_w = 0;
    for (int c = 0; c < n; ++c) {
        const int64_t H = h_hw[2 * c], W = h_hw[2 * c + 1];
        ARG_CHECK(H >= 2 && W >= 2, "an image is at least 2 x 2");
        ARG_CHECK(H * W == h_off[c + 1] - h_off[c], "the offsets must hold H * W pixels per image");
        if (H > s->max_h) s->max_h = (int)H;
        if (W > s->max_w) s->max_w = (int)W;
    }
    ARG_CHECK(s->px.largest <= FEAT_MAX_PIXELS, "an image has at most 2^30 pixels");
    ARG_CHECK(ceil_div64(s->max_h, FEAT_TILE) <= 65535, "an image has at most 65535 * 16 rows");
    return CSLAM_OK;
}

static int feat_src_check(const int64_t *h_src_off, const int64_t *h_off, int n) {
    ARG_CHECK(h_src_off != nullptr, "h_src_off is required");
    RaggedShape s;
    int rc = offsets_check(h_src_off, n, &s);
    if (rc) return rc;
    for (int c = 0; c < n; ++c) {
        const int64_t bytes = h_src_off[c + 1] - h_src_off[c], px = h_off[c + 1] - h_off[c];
        ARG_CHECK(bytes == px || bytes == 3 * px, "an image has 1 channel or 3 (BGR)");
    }
    return CSLAM_OK;
}

static int feat_stereo_checks(const StereoParams &P, const double *h_cameras, int n) {
    ARG_CHECK(P.min_disparity >= 1 && P.min_disparity <= P.max_disparity && P.max_disparity <= STEREO_MAX_DISPARITY,
              "1 <= min_disparity <= max_disparity <= 255 is required");
    ARG_CHECK(P.uniqueness >= 0 && P.uniqueness <= 100, "uniqueness must be in [0, 100] percent");
    ARG_CHECK(P.lr_tolerance >= -1 && P.lr_tolerance <= 255, "lr_tolerance must be in [-1, 255]");
    ARG_CHECK(h_cameras != nullptr, "h_cameras is required");
    for (int c = 0; c < n; ++c) {
        const double *cam = h_cameras + 5 * c;
        ARG_CHECK(isfinite(cam[0]) && isfinite(cam[1]) && isfinite(cam[2]) && isfinite(cam[3]) && isfinite(cam[4]),
                  "a stereo camera (fx, fy, cx, cy, baseline) must be finite");
        ARG_CHECK(cam[0] > 0.0 && cam[1] > 0.0 && cam[4] > 0.0, "fx, fy and the baseline must be positive");
    }
    return CSLAM_OK;
}
