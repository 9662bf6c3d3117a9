"""Visual keyframes over a scale pyramid, on the GPU (feat_pyr_level_kernel and feat_pyr_merge_kernel in csrc/feat.hip, the
rules in csrc/feat_pyr.h): the corners and steered BRIEF-32 descriptors of visual_features.py, detected and described on
`levels` images per frame, each 5/6 the size of the one below, and merged into rows whose keypoints are level-0
coordinates.  The `Keyframe`s go unchanged into `register_pairs`: two views of a place from different distances share
features between level l of the far view and a higher level of the near one, which the single-scale chain cannot offer.

The rule is the one include/cslam_hip.h states and tests/feat_pyramid_reference.py restates: integers up to the final
coordinates, so the two agree bit for bit.  Level l of an n-pixel axis has (n 5^l + 6^l / 2) / 6^l pixels and is resampled
from level l - 1 with a 2 x 2 footprint; every level is an image of its own to the response, candidate, selection and
describe kernels (its own Rmax, the same quality_level, min_distance and border, in level pixels); level l gets
max_features 5^l 6^(L - 1 - l) / sum of the budget, the remainder goes to level 0, and budget a level does not use is not
passed on.  Rows are ordered level 0 first, within a level in selection order.  `levels=1` is `extract_features`.

With `subpixel=True` the chains refine every keypoint on the response map of its level (feat_pyr_subpix_kernel): per axis
den = m - 2 c + p and num = m - p in int64 from the responses before, at and after the keypoint; den >= 0 or a neighbour
outside the image gives offset 0, otherwise num / (2 den) clamped to [-0.5, 0.5]; the level-0 coordinate is
((2 x + 1) + 2 off) n_0 / (2 n_l) - 0.5.  The integer level-0 pixel under the keypoint, where depth is read and the stereo
rule runs, does not move.  `extract_level_keyframes` returns `LevelKeyframe`s, whose levels `register_level_pairs`
(visual_registration.py) uses for per-level reprojection thresholds and weights.

Out of scope: a scale gate in the matcher (measured on the two-distance scene of the tests: at a factor that is safe against
level quantisation and depth noise, 1.3, it changes nothing: 0.0138 against 0.0133 m; it only pays at 1.1, which rejects
true matches one level off), guided re-matching after the fit, dense stereo, and parity with OpenCV's ORB pyramid and
cornerSubPix (unpinned like the rest of the features).

There is no CPU path: without the library or a GPU the functions raise CslamHipError.
"""
import numpy as np

from .. import _lib
from ..lidar_pr._batch import gpu, host, offsets, stream, to_dev
from .visual_features import FEAT_DESC_BYTES, _Batch, _depth, _image, _inside, _keypoints, _ragged_keypoints, _selection
from .visual_registration import Keyframe, LevelKeyframe, _cameras
from .visual_stereo import _pairs, _parameters, _stereo_cameras, _whole

MAX_LEVELS = 8
LEVEL_RUN = 4                  # bytes a thread of the level kernel stores as one word: level images start on multiples of it
LEVEL_BLOCK = 256              # threads of its workgroup, which covers LEVEL_RUN * LEVEL_BLOCK consecutive bytes
MAX_SIDE = 1 << 20


# ---- the host rules ----------------------------------------------------------------------------------------------------
def _level_count(levels):
    L = _whole(levels, "levels")
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError("levels must be in [1, %d]" % MAX_LEVELS)
    return L


def level_sizes(shape, levels):
    """[(H_l, W_l)] of the `levels` levels of an image of `shape`: n_l = (n 5^l + 6^l / 2) / 6^l by integer division."""
    L = _level_count(levels)
    H, W = int(shape[0]), int(shape[1])
    return [((H * 5 ** l + 6 ** l // 2) // 6 ** l, (W * 5 ** l + 6 ** l // 2) // 6 ** l) for l in range(L)]


def level_budgets(max_features, levels):
    """The features each level may give: max_features w_l / sum w with w_l = 5^l 6^(L - 1 - l), the remainder to level 0."""
    L, mf = _level_count(levels), _whole(max_features, "max_features")
    if not 1 <= mf <= 65535:
        raise ValueError("max_features must be in [1, 65535]")
    w = [5 ** l * 6 ** (L - 1 - l) for l in range(L)]
    b = [mf * x // sum(w) for x in w]
    b[0] += mf - sum(b)
    return b


def _frame_levels(shapes, levels, min_side, what):
    """Level sizes per frame; raises when a frame is too small for its top level."""
    L = _level_count(levels)
    out = []
    for s in shapes:
        if s[0] > MAX_SIDE or s[1] > MAX_SIDE:
            raise ValueError("a pyramid image has at most 2^20 rows and columns, got %s" % (tuple(s[:2]),))
        sizes = level_sizes(s, L)
        if min(sizes[-1]) < min_side:
            raise ValueError("a frame of %s is too small for %d levels: level %d is %s, every level must be at least %s on each side"
                             % (tuple(s[:2]), L, L - 1, sizes[-1], what))
        out.append(sizes)
    return L, out


def _level_major(per_frame):
    """[frame][level] -> the flat order of the level layout: all frames' level 0, then all frames' level 1, ..."""
    return [frame[l] for l in range(len(per_frame[0]) if per_frame else 0) for frame in per_frame]


class _Levels:
    """The level images of a batch as one ragged batch: image l * n + c = level l of frame c, on the host and the device.
    Every image starts on a multiple of LEVEL_RUN pixels."""

    def __init__(self, sizes, dev):
        self.n = len(sizes)
        self.shapes = _level_major(sizes)
        self.hw = np.ascontiguousarray(self.shapes, dtype=np.int32).reshape(len(self.shapes), 2)
        self.off = offsets([(h * w + LEVEL_RUN - 1) // LEVEL_RUN * LEVEL_RUN for h, w in self.shapes])
        self.total = int(self.off[-1])
        self.t_hw, self.t_off = to_dev(self.hw, dev), to_dev(self.off, dev)

    def split(self, flat, L):
        imgs = [flat[self.off[i]:self.off[i] + h * w].reshape(h, w).copy() for i, (h, w) in enumerate(self.shapes)]
        return [imgs[c::self.n] for c in range(self.n)]


# ---- the staged calls --------------------------------------------------------------------------------------------------
def build_pyramid(grays, levels, depths=None, device=0):
    """The level images of a list of grey images in ONE call (`cslam_feat_pyramid_dev`): per image the list of its `levels`
    uint8 images, level 0 being the image itself.  With `depths` (one per image, of its size) per image a pair (images,
    maps): map l is uint8 [H_l, W_l], 1 where the depth at the level-0 pixel under the level pixel is valid.  Every level
    must be at least 2 x 2."""
    imgs = [_image(g, channels_ok=(1,)) for g in grays]
    L, sizes = _frame_levels([i.shape for i in imgs], levels, 2, "2")
    if depths is not None and len(depths) != len(imgs):
        raise ValueError("one depth image per image")
    dps = None if depths is None else [_depth(d, i.shape) for d, i in zip(depths, imgs)]
    with gpu(device) as (lib, dev):
        import torch
        if not imgs:
            return []
        b, lv = _Batch([i.shape for i in imgs], dev), _Levels(sizes, dev)
        t_gray = b.flat(imgs, np.uint8, dev)
        t_depth = None if dps is None else b.flat(dps, np.float32, dev)
        t_lg = torch.zeros(lv.total, dtype=torch.uint8, device=dev)
        t_lv = None if dps is None else torch.zeros(lv.total, dtype=torch.uint8, device=dev)
        _lib.check(lib.cslam_feat_pyramid_dev(t_gray.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, L,
                                              None if dps is None else t_depth.data_ptr(), lv.t_off.data_ptr(), lv.t_hw.data_ptr(),
                                              t_lg.data_ptr(), None if dps is None else t_lv.data_ptr(), host(b.off), host(b.hw),
                                              host(lv.off), host(lv.hw), stream()))
        out = lv.split(t_lg.cpu().numpy(), L)
        if dps is not None:
            out = list(zip(out, lv.split(t_lv.cpu().numpy(), L)))
    return out


def merge_levels(shapes, level_features, cameras, max_features=1000, device=0):
    """The merge of the per-level features into per-frame rows in ONE call (`cslam_feat_pyramid_merge_dev`).  `shapes`: the
    (H, W) of the frames; `level_features`: per frame a list of L dicts with keypoints int32 [k, 2] in level pixels,
    responses, bins int32 [k], descriptors uint8 [k, 32] and z float64 [k], the depth at each keypoint (not finite or
    <= 0: a NaN point).  A level gives at most its budget of `level_budgets(max_features, L)`.  Per frame the dict of
    `extract_features_pyramid`."""
    if len(level_features) != len(shapes):
        raise ValueError("one list of level features per frame")
    L = len(level_features[0]) if len(level_features) else 1
    if any(len(f) != L for f in level_features):
        raise ValueError("every frame has the same number of levels")
    L, sizes = _frame_levels(shapes, L, 2, "2")
    mf = sum(level_budgets(max_features, L))               # the budgets share out max_features, which this also checks
    cam = _cameras(cameras, len(shapes))
    flat = _level_major(level_features)
    for f, (h, w) in zip(flat, _level_major(sizes)):
        kp = _keypoints(f["keypoints"])
        if any(len(f[key]) != len(kp) for key in ("responses", "bins", "descriptors", "z")) or len(kp) > 65535:
            raise ValueError("a level's keypoints, responses, bins, descriptors and z have one row per keypoint, at most 65535")
        _inside(kp, (h, w), 0, "keypoints must lie inside their level image")
    with gpu(device) as (lib, dev):
        import torch
        if not flat:
            return []
        n, stride = len(shapes), max(1, max(len(f["keypoints"]) for f in flat))
        lv = _Levels(sizes, dev)
        hw = np.ascontiguousarray([[s[0], s[1]] for s in shapes], dtype=np.int32)

        def packed(key, dtype, tail):
            a = np.zeros((len(flat), stride) + tail, dtype=dtype)
            for i, f in enumerate(flat):
                a[i, :len(f[key])] = np.asarray(f[key], dtype=dtype).reshape((-1,) + tail)
            return to_dev(a, dev)
        t_cnt_l = to_dev(np.array([len(f["keypoints"]) for f in flat], dtype=np.int32), dev)
        t_kp_l, t_resp_l, t_bins_l = packed("keypoints", np.int32, (2,)), packed("responses", np.int32, ()), packed("bins", np.int32, ())
        t_desc_l, t_z_l = packed("descriptors", np.uint8, (FEAT_DESC_BYTES,)), packed("z", np.float64, ())
        t_hw, t_cam = to_dev(hw, dev), to_dev(cam, dev)
        out = _Rows(n, mf, dev)
        _lib.check(lib.cslam_feat_pyramid_merge_dev(t_cnt_l.data_ptr(), t_kp_l.data_ptr(), t_resp_l.data_ptr(), t_bins_l.data_ptr(),
                                                    t_desc_l.data_ptr(), t_z_l.data_ptr(), stride, t_hw.data_ptr(), lv.t_hw.data_ptr(),
                                                    t_cam.data_ptr(), n, L, mf, *out.pointers(), host(hw), host(lv.off), host(lv.hw), stream()))
        return out.frames()


def subpixel_offsets(responses, keypoints, device=0):
    """The sub-pixel offsets of integer keypoints on their response maps in ONE call (`cslam_feat_subpixel_dev`).
    `responses`: a list of int32 [H, W] maps (a level image is a map of its own); `keypoints`: per map int32 [k, 2] = (x, y).
    Per map float64 [k, 2] = (off x, off y), each in [-0.5, 0.5]; a keypoint outside its map gives (0, 0)."""
    if len(responses) != len(keypoints):
        raise ValueError("one list of keypoints per response map")
    maps = []
    for r in responses:
        r = np.asarray(r)
        if r.ndim != 2 or r.dtype != np.int32 or min(r.shape) < 2:
            raise ValueError("a response map is int32 [H, W] with H, W >= 2, got %s %s" % (r.dtype, r.shape))
        maps.append(np.ascontiguousarray(r))
    kps = [_keypoints(k) for k in keypoints]
    with gpu(device) as (lib, dev):
        import torch
        if not maps:
            return []
        b = _Batch([m.shape for m in maps], dev)
        t_R = b.flat(maps, np.int32, dev)
        kp_off, t_kp, t_ko = _ragged_keypoints(kps, dev)
        t_out = torch.zeros((max(int(kp_off[-1]), 1), 2), dtype=torch.float64, device=dev)
        _lib.check(lib.cslam_feat_subpixel_dev(t_R.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), b.n, t_kp.data_ptr(), t_ko.data_ptr(),
                                               t_out.data_ptr(), host(b.off), host(b.hw), host(kp_off), stream()))
        out = t_out.cpu().numpy()
    return [out[kp_off[c]:kp_off[c + 1]].copy() for c in range(len(maps))]


class _Rows:
    """The per-frame outputs of the merge, [n, max_features, ..] on the device; with `subpixel` also the offsets."""

    def __init__(self, n, mf, dev, subpixel=False):
        import torch
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        self.n = n
        self.count = z(n, torch.int32)
        self.named = dict(keypoints=z((n, mf, 2), torch.float64), level_keypoints=z((n, mf, 2), torch.int32), levels=z((n, mf), torch.int32),
                          responses=z((n, mf), torch.int32), bins=z((n, mf), torch.int32), descriptors=z((n, mf, FEAT_DESC_BYTES), torch.uint8),
                          points=z((n, mf, 3), torch.float64))
        self.offsets = z((n, mf, 2), torch.float64) if subpixel else None

    def pointers(self):
        """count and the named outputs, the arguments every merge takes in this order."""
        return [self.count.data_ptr()] + [t.data_ptr() for t in self.named.values()]

    def more(self):
        """what the sub-pixel chains take after their other outputs."""
        return [] if self.offsets is None else [self.offsets.data_ptr()]

    def frames(self, **more):
        if self.offsets is not None:
            more = dict(more, offsets=self.offsets)
        cnt = self.count.cpu().numpy()
        arrays = {k: t.cpu().numpy() for k, t in list(self.named.items()) + list(more.items())}
        return [{k: a[c, :cnt[c]].copy() for k, a in arrays.items()} for c in range(self.n)]


# ---- the whole chains --------------------------------------------------------------------------------------------------
def extract_features_pyramid(images, depths, cameras, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19,
                             depth_as_mask=True, device=0, subpixel=False):
    """The whole pyramid chain of a list of images in ONE call (`cslam_feat_extract_pyramid_dev`), chained on the device with
    no host wait in between.  Per image the dict of `extract_features` with keypoints float64 [k, 2] in level-0
    coordinates, plus levels int32 [k] and level_keypoints int32 [k, 2], the pixel of the level image.  `subpixel=True`
    (`cslam_feat_extract_pyramid_subpix_dev`): keypoints and points are refined and the key `offsets` float64 [k, 2] holds
    the offsets in level pixels; every other key keeps its bytes."""
    imgs = [_image(i) for i in images]
    if len(depths) != len(imgs):
        raise ValueError("one depth image per image")
    dps = [_depth(d, i.shape[:2]) for d, i in zip(depths, imgs)]
    mf, q, md, bd = _selection(max_features, quality_level, min_distance, border, [i.shape for i in imgs])
    L, sizes = _frame_levels([i.shape for i in imgs], levels, 2 * bd + 1, "2 * border + 1 = %d" % (2 * bd + 1))
    cam = _cameras(cameras, len(imgs))
    with gpu(device) as (lib, dev):
        if not imgs:
            return []
        b, lv = _Batch([i.shape for i in imgs], dev), _Levels(sizes, dev)
        src_off = offsets([i.size for i in imgs])
        t_src, t_so, t_depth, t_cam = b.flat(imgs, np.uint8, dev), to_dev(src_off, dev), b.flat(dps, np.float32, dev), to_dev(cam, dev)
        out = _Rows(b.n, mf, dev, subpixel)
        entry = lib.cslam_feat_extract_pyramid_subpix_dev if subpixel else lib.cslam_feat_extract_pyramid_dev
        _lib.check(entry(t_src.data_ptr(), t_so.data_ptr(), t_depth.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(), t_cam.data_ptr(), b.n, L,
                         lv.t_off.data_ptr(), lv.t_hw.data_ptr(), q, md, bd, mf, 1 if depth_as_mask else 0, *out.pointers(), *out.more(),
                         host(src_off), host(b.off), host(b.hw), host(lv.off), host(lv.hw), stream()))
        return out.frames()


def extract_keyframes_pyramid(images, depths, cameras, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19,
                              depth_as_mask=True, device=0):
    """A `Keyframe` per image from the pyramid chain, ready for `register_pairs`."""
    return [Keyframe(f["keypoints"], f["points"], f["descriptors"])
            for f in extract_features_pyramid(images, depths, cameras, levels, max_features, quality_level, min_distance, border, depth_as_mask,
                                              device)]


def extract_features_stereo_pyramid(lefts, rights, cameras, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19,
                                    min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0, subpixel=False):
    """The pyramid chain of a list of stereo frames in ONE call (`cslam_feat_extract_stereo_pyramid_dev`): the pyramid on the
    left image without a mask, the stereo rule at the level-0 pixel under each keypoint, and the point of the keypoint's
    level-0 coordinates at the Z it gives.  Per frame the dict of `extract_features_pyramid` plus disparity float64 [k] and
    status int32 [k]; a rejected keypoint keeps a NaN point.  `subpixel=True`
    (`cslam_feat_extract_stereo_pyramid_subpix_dev`) as in `extract_features_pyramid`."""
    ls, rs = _pairs(lefts, rights, (1, 3))
    mf, q, md, bd = _selection(max_features, quality_level, min_distance, border, [i.shape for i in ls])
    L, sizes = _frame_levels([i.shape for i in ls], levels, 2 * bd + 1, "2 * border + 1 = %d" % (2 * bd + 1))
    lo, hi, uq, lr = _parameters(min_disparity, max_disparity, uniqueness, lr_tolerance)
    cam = _stereo_cameras(cameras, len(ls))
    with gpu(device) as (lib, dev):
        import torch
        if not ls:
            return []
        b, lv = _Batch([i.shape for i in ls], dev), _Levels(sizes, dev)
        l_off, r_off = offsets([i.size for i in ls]), offsets([i.size for i in rs])
        t_left, t_lo, t_right, t_ro = b.flat(ls, np.uint8, dev), to_dev(l_off, dev), b.flat(rs, np.uint8, dev), to_dev(r_off, dev)
        t_cam = to_dev(cam, dev)
        out = _Rows(b.n, mf, dev, subpixel)
        t_disp = torch.zeros((b.n, mf), dtype=torch.float64, device=dev)
        t_status = torch.zeros((b.n, mf), dtype=torch.int32, device=dev)
        entry = lib.cslam_feat_extract_stereo_pyramid_subpix_dev if subpixel else lib.cslam_feat_extract_stereo_pyramid_dev
        _lib.check(entry(t_left.data_ptr(), t_lo.data_ptr(), t_right.data_ptr(), t_ro.data_ptr(), b.t_off.data_ptr(), b.t_hw.data_ptr(),
                         t_cam.data_ptr(), b.n, L, lv.t_off.data_ptr(), lv.t_hw.data_ptr(), q, md, bd, mf, lo, hi, uq, lr, *out.pointers(),
                         t_disp.data_ptr(), t_status.data_ptr(), *out.more(), host(l_off), host(r_off), host(b.off), host(b.hw),
                         host(lv.off), host(lv.hw), host(cam), stream()))
        return out.frames(disparity=t_disp, status=t_status)


def extract_keyframes_stereo_pyramid(lefts, rights, cameras, levels=4, max_features=1000, quality_level=0.001, min_distance=7, border=19,
                                     min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """A `Keyframe` per stereo frame from the pyramid chain, ready for `register_pairs` with the first four numbers of the
    camera.  Keypoints without a correspondence keep a NaN point."""
    return [Keyframe(f["keypoints"], f["points"], f["descriptors"])
            for f in extract_features_stereo_pyramid(lefts, rights, cameras, levels, max_features, quality_level, min_distance, border,
                                                     min_disparity, max_disparity, uniqueness, lr_tolerance, device)]


def _level_keyframe(f):
    return LevelKeyframe(f["keypoints"], f["points"], f["descriptors"], f["levels"].astype(np.uint8))


def extract_level_keyframes(images, depths, cameras, levels=4, subpixel=True, max_features=1000, quality_level=0.001, min_distance=7,
                            border=19, depth_as_mask=True, device=0):
    """A `LevelKeyframe` per image from the pyramid chain, by default with sub-pixel keypoints: ready for
    `register_level_pairs`, and for `register_pairs`, which reads the fields it knows."""
    return [_level_keyframe(f) for f in extract_features_pyramid(images, depths, cameras, levels, max_features, quality_level, min_distance,
                                                                 border, depth_as_mask, device, subpixel)]


def extract_level_keyframes_stereo(lefts, rights, cameras, levels=4, subpixel=True, max_features=1000, quality_level=0.001, min_distance=7,
                                   border=19, min_disparity=1, max_disparity=128, uniqueness=15, lr_tolerance=1, device=0):
    """A `LevelKeyframe` per stereo frame from the pyramid chain, by default with sub-pixel keypoints."""
    return [_level_keyframe(f) for f in extract_features_stereo_pyramid(lefts, rights, cameras, levels, max_features, quality_level,
                                                                        min_distance, border, min_disparity, max_disparity, uniqueness,
                                                                        lr_tolerance, device, subpixel)]
