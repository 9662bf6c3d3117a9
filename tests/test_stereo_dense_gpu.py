"""GPU: the dense stereo kernel (csrc/stereo_dense.hip through cslam_amd.front_end.stereo_depth) against the sparse kernel
at every pixel, against its numpy restatement (tests/stereo_dense_reference.py), and through the cloud chain into the map.
Everything is compared bit for bit: status, best, and the uint32 views of disparity and depth, NaN pattern included.  Only
the end-to-end test has bounds, and those are derived in its docstring."""
import functools

import numpy as np
import pytest

import feat_reference
import stereo_dense_reference as dref
import stereo_reference as sr
from cslam_amd.back_end.swarm_map import assemble_map
from cslam_amd.front_end import keyframe_clouds as kc
from cslam_amd.front_end import stereo_depth as sd
from cslam_amd.front_end import visual_stereo as vs

pytestmark = pytest.mark.gpu

CAM = dref.CAMERA
T, TD, SEG = dref.TILE               # the kernel's tile of columns, of disparities, and a thread's run of columns
SCENE_IDS = [s[0] for s in dref.SCENES]


def bits(a):
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(a, b):
    """The same bits, any NaN counting as NaN."""
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)]))


def same_as_restatement(got, want):
    assert got["status"].dtype == np.uint8 and np.array_equal(got["status"], want["status"])
    if "best" in got:
        assert got["best"].dtype == np.int32 and np.array_equal(got["best"], want["best"])
    same_floats(got["disparity"], want["disparity32"])
    same_floats(got["depth"], want["depth"])
    assert np.array_equal(np.isnan(got["disparity"]), got["status"] != 0)
    assert np.array_equal(np.isnan(got["depth"]), got["status"] != 0)


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


@functools.lru_cache(maxsize=None)
def restated(k):
    """Scene k and its restatement, computed once and left unchanged."""
    L, R, params, want = dref.scene(k)
    d = dref.dense(L, R, CAM, **params)
    for a in (L, R) + tuple(d.values()):
        a.setflags(write=False)
    return L, R, params, d


@functools.lru_cache(maxsize=None)
def restated_pair(H, W, shift, max_disparity):
    L, R = sr.shifted_pair(H, W, shift)
    d = dref.dense(L, R, CAM, max_disparity=max_disparity)
    for a in (L, R) + tuple(d.values()):
        a.setflags(write=False)
    return L, R, d


@pytest.mark.parametrize("k", range(len(dref.SCENES)), ids=SCENE_IDS)
def test_dense_equals_the_sparse_kernel_at_every_pixel(k):
    L, R, params, _ = restated(k)
    H, W = L.shape
    got = sd.dense_disparity(L, R, CAM, return_best=True, **params)
    sparse = vs.stereo_match(L, R, dref.all_pixels(H, W), CAM, **params)
    assert np.array_equal(got["status"], sparse["status"].reshape(H, W))
    assert np.array_equal(got["best"], sparse["best"].reshape(H, W, 4))
    same_floats(got["disparity"], sparse["disparity"].astype(np.float32).reshape(H, W))
    same_floats(got["depth"], sparse["points"][:, 2].astype(np.float32).reshape(H, W))


@pytest.mark.parametrize("k", range(len(dref.SCENES)), ids=SCENE_IDS)
def test_dense_equals_the_restatement(k):
    L, R, params, want = restated(k)
    got = sd.dense_disparity(L, R, CAM, return_best=True, **params)
    same_as_restatement(got, want)
    assert dref.counts(got["status"]) == dref.SCENES[k][3]


# Widths: T + 13 is the last at which the second column tile holds no searched column, T + 14 has one, T + 15 two, 2 T + 14
# puts one in a third tile; SEG + 13 .. SEG + 15 do the same to a thread's run of SEG columns; 63 .. 65 and 141 .. 143 (128 +
# 14) are the widths around 64 and 128 searched columns.  Ranges: D_lo .. max_disparity + 1 holds max_disparity + 2
# disparities, so TD - 2 fills one disparity tile exactly and TD - 1 spills one disparity into the next; 62 .. 65 do the same
# to two tiles, 126 fills four, 254 fills eight and 255 is the full 257-entry range of nine.
EDGE_WIDTHS = (SEG + 13, SEG + 14, SEG + 15, 63, 64, 65, 141, 142, 143, T + 13, T + 14, T + 15, 2 * T + 14)
EDGE_RANGES = (TD - 2, TD - 1, TD, TD + 1, 62, 63, 64, 65, 126, 254, 255)


@pytest.mark.parametrize("max_disparity", EDGE_RANGES)
def test_tile_edges(max_disparity):
    """Every edge width in one ragged call per range, each frame against the restatement."""
    frames = [restated_pair(3, W, 9, max_disparity) for W in EDGE_WIDTHS]
    got = sd.dense_disparity_batch([f[0] for f in frames], [f[1] for f in frames], CAM, max_disparity=max_disparity, return_best=True)
    for g, f in zip(got, frames):
        same_as_restatement(g, f[2])
    assert any(np.any(g["status"] == 0) for g in got)


@pytest.mark.parametrize("H", [3, 4, 6])
def test_heights(H):
    """One searched row, two, and four: a workgroup owns one row, so every height is one more than a multiple of it; what can go
    wrong is the first and the last row and the row index itself."""
    L, R, want = restated_pair(H, 70, 9, 24)
    got = sd.dense_disparity(L, R, CAM, max_disparity=24, return_best=True)
    same_as_restatement(got, want)
    assert np.all(got["status"][0] == 1) and np.all(got["status"][-1] == 1) and np.any(got["status"][1:-1] == 0)


def test_ragged_batch_equals_the_frames_alone():
    """Scenes 1, 4, 6 and 9 in one call, grey and B = G = R sides mixed (whose grey is the same byte), against the same frames
    one by one and in reversed order: byte for byte.  The parameters are one set for the call."""
    bgr = lambda g: np.ascontiguousarray(np.stack([g, g, g], axis=-1))
    ks = (0, 3, 5, 8)
    lefts = [restated(k)[0] if i % 2 else bgr(restated(k)[0]) for i, k in enumerate(ks)]
    rights = [bgr(restated(k)[1]) if i % 3 == 0 else restated(k)[1] for i, k in enumerate(ks)]
    cams = np.array([CAM, (90.0, 95.0, 10.0, 2.0, 0.1), (120.0, 120.0, 64.0, 1.5, 0.3), CAM])
    kw = dict(max_disparity=40, return_best=True)
    batch = sd.dense_disparity_batch(lefts, rights, cams, **kw)
    assert [b["status"].shape for b in batch] == [restated(k)[0].shape for k in ks]
    for i in range(len(ks)):
        same_bytes(batch[i], sd.dense_disparity(lefts[i], rights[i], cams[i], **kw))
        L, R = restated(ks[i])[:2]
        same_as_restatement(batch[i], dref.dense(L, R, cams[i], max_disparity=40))
    back = sd.dense_disparity_batch(lefts[::-1], rights[::-1], cams[::-1], **kw)
    for a, b in zip(batch, back[::-1]):
        same_bytes(a, b)


def coloured(g):
    """A B, G, R image whose channels differ; its grey is a function of g, the same on both sides of a pair."""
    return np.ascontiguousarray(np.stack([g, g // 2, 255 - g // 4], axis=-1))


@pytest.mark.parametrize("voxel_size", [0.05, 0.0])
def test_chained_equals_staged(voxel_size):
    """`keyframe_clouds_stereo` against `dense_disparity_batch`, then `keyframe_clouds` on its depth: points, colours and counts
    byte for byte.  Disparities 5 and 20 at fx 100 and a baseline of 0.2 are 4 m and 1 m, so max_range 2 clips."""
    (L0, R0), (L1, R1) = dref.scene(0)[:2], dref.scene(2)[:2]
    lefts, rights = [coloured(L0), L1, coloured(L1)], [coloured(R0), np.ascontiguousarray(np.stack([R1, R1, R1], axis=-1)), coloured(R1)]
    cam5 = np.array([(100.0, 100.0, 100.0, 5.0, 0.2), (100.0, 110.0, 32.0, 2.5, 0.2), (80.0, 80.0, 30.0, 2.0, 0.25)])
    kw = dict(max_disparity=32)
    dense = sd.dense_disparity_batch(lefts, rights, cam5, **kw)
    staged = kc.keyframe_clouds(lefts, [f["depth"] for f in dense], cam5[:, :4], voxel_size, 2.0)
    chained = sd.keyframe_clouds_stereo(lefts, rights, cam5, voxel_size, 2.0, **kw)
    assert len(chained) == len(staged) == 3
    for a, b, f in zip(chained, staged, dense):
        assert a.points.dtype == np.float32 and a.colors.dtype == np.uint8 and a.counts.dtype == np.int64
        assert a.points.tobytes() == b.points.tobytes() and a.colors.tobytes() == b.colors.tobytes() and np.array_equal(a.counts, b.counts)
        if voxel_size == 0.0:                              # the organised cloud
            assert len(a.points) == f["status"].size
            assert np.array_equal(np.isnan(a.points).all(axis=1), f["status"].reshape(-1) != 0)
            assert np.array_equal(np.isnan(a.points).any(axis=1), f["status"].reshape(-1) != 0)
        else:
            assert len(a.points) <= int((f["status"] == 0).sum()) and np.all(a.points[:, 2] <= 2.0)
    assert len(chained[0].points) > 0                      # the foreground of the first frame lies at 1 m


def test_stereo_frames_to_the_map():
    """Two stereo views of one block texture 16 columns apart, true disparity 10 = 2 m at fx 100 and a baseline of 0.2 m.
    A pixel accepted at d* = 10 has a parabola offset within +-0.5, so its depth lies in [0.2 * 100 / 10.5, 0.2 * 100 / 9.5] =
    [1.905, 2.105] m: derived, not measured.  A voxel's point is a mean of such depths, in the keyframe cloud and again in the
    map, and the second view's pose is a shift along x, so every z of the map lies in the same interval, widened by half a
    voxel for the float32 sums."""
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    lefts, rights = [cut(0), cut(16)], [cut(10), cut(26)]
    cam = (100.0, 100.0, 80.0, 60.0, 0.2)
    voxel, lo, hi = 0.05, 0.2 * 100.0 / 10.5, 0.2 * 100.0 / 9.5
    dense = sd.dense_disparity_batch(lefts, rights, cam)
    for f, L, R in zip(dense, lefts, rights):
        want = dref.dense(L, R, cam)
        same_as_restatement(f, want)
        ok = f["status"] == 0
        share, want_share = ok.mean(), (want["status"] == 0).mean()
        print("accepted %.4f of the pixels (restatement %.4f), depth %.4f .. %.4f m" % (share, want_share, f["depth"][ok].min(), f["depth"][ok].max()))
        assert share >= want_share
        assert np.all(f["depth"][ok] >= np.float32(lo)) and np.all(f["depth"][ok] <= np.float32(hi))
    clouds = sd.keyframe_clouds_stereo(lefts, rights, cam, voxel, 3.0)
    assert all(len(c.points) > 0 for c in clouds)
    poses = {0: np.eye(4), 1: np.eye(4)}
    poses[1][0, 3] = 16 * 2.0 / 100.0                      # the second camera stands 16 columns = 0.32 m to the right
    m = assemble_map({0: clouds[0], 1: clouds[1]}, poses, voxel)
    assert len(m.points) > 0 and m.counts.sum() == sum(len(c.points) for c in clouds)
    assert np.all(m.points[:, 2] >= lo - voxel / 2) and np.all(m.points[:, 2] <= hi + voxel / 2)
    # the two views overlap: the map has fewer voxels than the two clouds have rows
    assert len(m.points) < sum(len(c.points) for c in clouds)
