"""GPU: csrc/cloud.hip against tests/cloud_reference.py, bit for bit (np.array_equal on equal dtypes everywhere).  What
makes these comparisons able to see a wrong constant or a wrong order of a sum is asserted in tests/test_cloud_cpu.py."""
import numpy as np
import pytest

import cloud_reference as ref

pytestmark = pytest.mark.gpu

F = np.float32
CAM = ref.SCENE_CAMERA
CAM2 = (75.25, 74.5, 30.75, 24.125)                        # non-integer cx, cy


@pytest.fixture(scope="module")
def kc():
    from cslam_amd.front_end import keyframe_clouds
    return keyframe_clouds


@pytest.fixture(scope="module")
def sm():
    from cslam_amd.back_end import swarm_map
    return swarm_map


@pytest.fixture(scope="module")
def T():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils.VOXEL_TILE


def same(got, want):
    """A KeyframeCloud / SwarmMap against the restatement's (points, colors, counts): same dtypes, same bits (NaN = NaN)."""
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f")


def organised(image, depth, cam):
    p, c = ref.back_project(image, depth, cam)
    return p, c, np.ones(len(p), dtype=np.int64)


def frame(H, W, seed, depth_dtype, channels):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3) if channels == 3 else (H, W), dtype=np.uint8)
    d = rng.integers(300, 4000, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < 0.2] = 0
    if depth_dtype == np.float32:
        d = np.where(d == 0, np.nan, d.astype(F) * F(0.001)).astype(F)
    return img, d


# ---- back-projection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (16, 16), (17, 63), (48, 64)])
def test_back_projection(kc, H, W):
    for depth_dtype in (np.uint16, np.float32):
        for channels in (3, 1):
            img, d = frame(H, W, H * W, depth_dtype, channels)
            for cam in (CAM, CAM2):
                got = kc.create_colored_pointcloud(img, d, cam)
                assert got.points.shape == (H * W, 3)
                same(got, organised(img, d, cam))


def test_back_projection_of_the_scene_is_not_metres_first(kc):
    d, img = ref.scene_depth(), ref.scene_image()
    got = kc.create_colored_pointcloud(img, d, CAM)
    same(got, organised(img, d, CAM))
    other = ref.back_project_metres_first(d, CAM)
    assert not np.array_equal(got.points, other, equal_nan=True)


def test_back_projection_all_invalid_and_all_valid(kc):
    img = ref.scene_image(16, 16)
    for d in (np.zeros((16, 16), dtype=np.uint16), np.full((16, 16), np.nan, dtype=F)):
        got = kc.create_colored_pointcloud(img, d, CAM)
        assert np.isnan(got.points).all()
        same(got, organised(img, d, CAM))
    for d in (np.full((16, 16), 1234, dtype=np.uint16), np.full((16, 16), 1.234, dtype=F)):
        got = kc.create_colored_pointcloud(img, d, CAM)
        assert np.isfinite(got.points).all()
        same(got, organised(img, d, CAM))


def test_back_projection_float_depths_of_zero_negative_inf_nan(kc):
    img = ref.scene_image(3, 5)
    d = np.array([[0.0, -0.0, -1.5, np.inf, -np.inf], [np.nan, 2.5, 1e-30, 3e38, -3e38], [1.0, 0.5, 0.25, 65.535, 7.0]], dtype=F)
    got = kc.create_colored_pointcloud(img, d, CAM2)
    with np.errstate(all="ignore"):
        same(got, organised(img, d, CAM2))
    valid = np.isfinite(got.points).all(axis=1).reshape(3, 5)
    assert valid[0, :3].all() and not valid[0, 3:].any() and not valid[1, 0]      # 0 and below are valid, inf and NaN are not


def test_back_projection_ragged_batch_equals_one_by_one(kc):
    shapes = [(2, 2, np.uint16, 3), (17, 63, np.float32, 1), (3, 5, np.uint16, 3), (16, 16, np.uint16, 1), (48, 64, np.float32, 3),
              (5, 3, np.uint16, 3)]
    frames = [frame(H, W, 100 + k, dt, ch) for k, (H, W, dt, ch) in enumerate(shapes)]
    cams = np.array([[60.0 + k, 61.0 + k, 10.5 + k, 7.25 + k] for k in range(len(frames))])
    batch = kc.create_colored_pointclouds([f[0] for f in frames], [f[1] for f in frames], cams)
    for k, (img, d) in enumerate(frames):
        same(batch[k], kc.create_colored_pointcloud(img, d, cams[k]))
        same(batch[k], organised(img, d, cams[k]))


# ---- filter ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return ref.back_project(ref.scene_image(), ref.scene_depth(), CAM)


@pytest.mark.parametrize("leaf", [0.1, 0.05])
def test_filter_scene_forward_and_reversed(kc, scene, leaf):
    p, c = scene
    fwd = kc.voxel_subsample(p, c, leaf, 2.0)
    same(fwd, ref.voxel_filter(p, c, leaf, 2.0))
    rev = kc.voxel_subsample(p[::-1], c[::-1], leaf, 2.0)
    same(rev, ref.voxel_filter(p[::-1], c[::-1], leaf, 2.0))
    assert not np.array_equal(fwd.points, rev.points)      # the order of the sum is visible (test_cloud_cpu.py, fact b)
    unclipped = kc.voxel_subsample(p, c, leaf, 100.0)
    same(unclipped, ref.voxel_filter(p, c, leaf, 100.0))
    assert len(unclipped.points) > len(fwd.points) > 0
    if leaf == 0.1:
        assert len(unclipped.points) == 457 and unclipped.counts.max() == 16


def test_filter_sizes_around_the_tile_with_nan_rows(kc, T):
    rng = np.random.default_rng(11)
    clouds = []
    for k, n in enumerate((1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5)):
        pts = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
        col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        holes = np.sort(rng.choice(n + 1, size=max(1, n // 7), replace=True))      # NaN rows interleaved, also first and last
        pts = np.insert(pts, holes, np.array([np.nan, -np.inf, np.inf], dtype=F)[k % 3], axis=0)
        col = np.insert(col, holes, 255, axis=0)
        assert np.isfinite(pts).all(axis=1).sum() == n
        clouds.append((pts, col))
    got = kc.voxel_subsample_batch(clouds, 0.25, 0.75)
    for (p, c), g in zip(clouds, got):
        same(g, ref.voxel_filter(p, c, 0.25, 0.75))
    same(kc.voxel_subsample(*clouds[-1], 0.25, 0.75), ref.voxel_filter(*clouds[-1], 0.25, 0.75))      # alone = in the batch
    assert len(got[-1].points) > 100


def test_filter_one_voxel_of_5000_points(kc):
    rng = np.random.default_rng(12)
    p = rng.uniform(0.01, 0.04, (5000, 3)).astype(F) + np.array([0.0, 0.0, 1.0], dtype=F)
    c = rng.integers(0, 256, (5000, 3), dtype=np.uint8)
    got = kc.voxel_subsample(p, c, 1.0, 10.0)
    assert len(got.points) == 1 and got.counts.tolist() == [5000]
    same(got, ref.voxel_filter(p, c, 1.0, 10.0))
    rev = kc.voxel_subsample(p[::-1], c[::-1], 1.0, 10.0)
    same(rev, ref.voxel_filter(p[::-1], c[::-1], 1.0, 10.0))
    assert (got.points != rev.points).all() and np.array_equal(got.colors, rev.colors)      # any other order gives other bits


def test_filter_lattice_one_point_per_voxel(kc):
    g = (np.arange(10, dtype=np.float64) + 0.5) * 0.05
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    lattice = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)                # already in ascending (iz, iy, ix)
    col = np.random.default_rng(13).integers(0, 256, (1000, 3), dtype=np.uint8)
    perm = np.random.default_rng(14).permutation(1000)
    got = kc.voxel_subsample(lattice[perm], col[perm], 0.05, 100.0)
    assert np.array_equal(got.points, lattice) and np.array_equal(got.colors, col) and got.counts.tolist() == [1] * 1000
    same(got, ref.voxel_filter(lattice[perm], col[perm], 0.05, 100.0))


def test_filter_points_on_voxel_faces_and_negative_coordinates(kc):
    k = np.arange(-6, 7)
    z, y, x = np.meshgrid(k, k[:5], k[:3], indexing="ij")
    faces = (np.stack([x, y, z], axis=-1).reshape(-1, 3) * 0.25).astype(F)          # every coordinate exactly on a face
    inside = faces + F(0.125)
    both = np.concatenate([inside, faces])[np.random.default_rng(15).permutation(2 * len(faces))]
    got = kc.voxel_subsample(both, None, 0.25, 100.0)
    assert got.colors is None
    clipped = ref.voxel_filter(both, None, 0.25, 100.0)
    same(got, clipped)
    assert got.counts.tolist() == [2] * len(got.counts)    # a point on a face belongs to the voxel above it, below zero too
    assert 0 < len(clipped[0]) < len(ref.voxel_filter(both, None, 0.25, None)[0])      # the voxels with z < 0 are clipped


def test_filter_clip_by_the_centroid(kc):
    # leaf 0.1, max_range 1.95: four voxels at different x whose z cell [1.9, 2.0) straddles the limit, then the exact ends
    rows = [(0.05, 1.91, 1.92), (0.15, 1.96, 1.99), (0.25, 1.91, 1.98), (0.35, 1.93, 1.99)]
    pts = [[x, 0.05, z] for x, z0, z1 in rows for z in (z0, z1)]
    pts += [[0.45, 0.05, float(F(1.95))], [0.55, 0.05, 0.0], [0.65, 0.05, -0.01], [0.75, 0.05, float(np.nextafter(F(1.95), F(3)))]]
    pts = np.array(pts, dtype=F)
    col = np.arange(3 * len(pts), dtype=np.uint8).reshape(-1, 3)
    got = kc.voxel_subsample(pts, col, 0.1, 1.95)
    want = ref.voxel_filter(pts, col, 0.1, 1.95)
    same(got, want)
    xs = sorted(round(float(x), 2) for x in got.points[:, 0])
    assert xs == [0.05, 0.25, 0.45, 0.55]                  # kept by the centroid; z == max_range and z == 0 are kept
    assert len(ref.voxel_filter(pts, col, 0.1, None)[0]) == 8


def test_filter_colours_truncate(kc):
    pts = np.array([[0.01, 0.01, 0.5], [0.02, 0.02, 0.5], [0.03, 0.03, 0.5]], dtype=F)
    col = np.array([[1, 255, 0], [2, 255, 0], [2, 254, 1]], dtype=np.uint8)
    got = kc.voxel_subsample(pts, col, 1.0, 2.0)
    assert got.colors.tolist() == [[1, 254, 0]] and got.counts.tolist() == [3]
    same(got, ref.voxel_filter(pts, col, 1.0, 2.0))


def test_filter_empty_cloud_inside_a_batch(kc, scene):
    p, c = scene
    empty = (np.zeros((0, 3), dtype=F), np.zeros((0, 3), dtype=np.uint8))
    nan_only = (np.full((5, 3), np.nan, dtype=F), np.zeros((5, 3), dtype=np.uint8))
    got = kc.voxel_subsample_batch([(p, c), empty, nan_only, (p[::-1], c[::-1])], 0.1, 2.0)
    same(got[0], ref.voxel_filter(p, c, 0.1, 2.0))
    assert got[1].points.shape == (0, 3) and got[1].colors.shape == (0, 3) and got[1].counts.shape == (0,)
    assert got[2].points.shape == (0, 3)
    same(got[3], ref.voxel_filter(p[::-1], c[::-1], 0.1, 2.0))
    assert kc.voxel_subsample_batch([empty], 0.1, 2.0)[0].points.shape == (0, 3)


def test_filter_status_names_only_the_failing_cloud(kc, scene):
    from cslam_amd.lidar_pr.voxel import VoxelSizeError
    p, c = scene
    wide = np.array([[0.0, 0.0, 1.0], [2.0e5, 0.0, 1.0]], dtype=F)                 # index 4e6 at leaf 0.05
    with pytest.raises(ref.RangeError):
        ref.voxel_filter(wide, None, 0.05, 2.0)
    edge = np.array([[0.0, 0.0, 1.0], [(2 ** 21 - 1) * 0.5, 0.0, 1.0]], dtype=F)
    col2 = np.zeros((2, 3), dtype=np.uint8)
    with pytest.raises(VoxelSizeError) as e:
        kc.voxel_subsample_batch([(p, c), (wide, col2), (p[::-1], c[::-1])], 0.05, 2.0)
    assert e.value.failed == [1] and e.value.clouds[1] is None
    same(e.value.clouds[0], ref.voxel_filter(p, c, 0.05, 2.0))
    same(e.value.clouds[2], ref.voxel_filter(p[::-1], c[::-1], 0.05, 2.0))
    same(kc.voxel_subsample(edge, col2, 0.5, 2.0), ref.voxel_filter(edge, col2, 0.5, 2.0))     # index 2^21 - 1: the last a key holds
    assert len(ref.voxel_filter(edge, col2, 0.5, 2.0)[0]) == 2


def test_filter_voxel_size_zero_returns_the_input(kc, scene):
    p, c = scene
    got = kc.voxel_subsample(p, c, 0.0, 2.0)
    assert np.array_equal(got.points, p, equal_nan=True) and np.array_equal(got.colors, c)


# ---- chain -----------------------------------------------------------------------------------------------------------
def test_chain_equals_the_staged_calls(kc):
    shapes = [(48, 64, np.uint16, 3), (17, 63, np.float32, 1), (16, 16, np.uint16, 3), (3, 5, np.float32, 3), (2, 2, np.uint16, 1)]
    frames = [frame(H, W, 200 + k, dt, ch) for k, (H, W, dt, ch) in enumerate(shapes)]
    frames[0] = (ref.scene_image(), ref.scene_depth())
    imgs, dps = [f[0] for f in frames], [f[1] for f in frames]
    for leaf, max_range in ((0.05, 2.0), (0.1, 3.5)):
        chained = kc.keyframe_clouds(imgs, dps, CAM, leaf, max_range)
        staged = kc.voxel_subsample_batch([(o.points, o.colors) for o in kc.create_colored_pointclouds(imgs, dps, CAM)], leaf, max_range)
        for k in range(len(frames)):
            same(chained[k], staged[k])
            same(chained[k], ref.keyframe_cloud(imgs[k], dps[k], CAM, leaf, max_range))
        assert len(chained[0].points) > 100
    for got, img, d in zip(kc.keyframe_clouds(imgs, dps, CAM, 0.0), imgs, dps):
        same(got, organised(img, d, CAM))                  # voxel_size <= 0: the organised cloud, unfiltered and unclipped


def test_chain_full_frame(kc):
    """480 x 640: 4800 waves of the key kernel, 3 radix passes, 1200 head tiles (the scan block takes two each), voxels of
    more than 256 points."""
    H, W, cam = 480, 640, (525.0, 525.0, 319.5, 239.5)
    rng = np.random.default_rng(31)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = (800 + 2.5 * u + 1.8 * v + rng.integers(0, 40, (H, W))).astype(np.uint16)
    d[rng.random((H, W)) < 0.1] = 0
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = ref.keyframe_cloud(img, d, cam, 0.05, 2.0)
    assert len(want[0]) > 1000 and want[2].max() > 256
    same(kc.keyframe_clouds([img], [d], cam, 0.05, 2.0)[0], want)


# ---- map -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keyframes(kc):
    """The two keyframes of fact c as KeyframeClouds (leaf 0.05, unclipped)."""
    return [kc.KeyframeCloud(*k) for k in ref.scene_keyframes()]


def test_map_scene_forward_and_fully_reversed(sm, kc, keyframes):
    k1, k2 = keyframes
    T1, T2 = ref.scene_poses()
    fwd = sm.assemble_map({0: k1, 1: k2}, {0: T1, 1: T2, 2: np.identity(4)}, 0.1)
    want = ref.assemble_map([k1[:2], k2[:2]], [T1, T2], 0.1)
    same(fwd, want)
    assert fwd.points.dtype == np.float64 and len(fwd.points) == 839 and fwd.counts.max() == 11
    r1, r2 = kc.KeyframeCloud(k1.points[::-1], k1.colors[::-1], None), kc.KeyframeCloud(k2.points[::-1], k2.colors[::-1], None)
    rev = sm.assemble_map({0: r2, 1: r1}, {0: T2, 1: T1}, 0.1)
    same(rev, ref.assemble_map([r2[:2], r1[:2]], [T2, T1], 0.1))
    assert not np.array_equal(fwd.points, rev.points) and np.array_equal(fwd.colors, rev.colors)
    assert fwd.counts.sum() == len(k1.points) + len(k2.points)                     # input rows, not the keyframes' own counts


def test_map_dtypes_colours_and_sensor_to_body(sm, keyframes):
    k1, k2 = keyframes
    T1, T2 = ref.scene_poses()
    p1, p2 = k1.points.astype(np.float64) * 1.0000001, k2.points.astype(np.float64) * 0.9999999      # not float32 values
    got = sm.assemble_map({(0, 5): p1, (1, 2): p2}, {(0, 5): T1, (1, 2): T2}, 0.1)
    assert got.colors is None
    same(got, ref.assemble_map([(p1, None), (p2, None)], [T1, T2], 0.1))
    mixed = sm.assemble_map({0: k1, 1: p2}, {0: T1, 1: T2}, 0.1)                    # a lidar keyframe among them: float64, no colours
    same(mixed, ref.assemble_map([(k1.points, None), (p2, None)], [T1, T2], 0.1))
    ext = np.identity(4)
    ext[:3, :3] = ref.rotation((1.0, -1.0, 1.0), 2.0 * np.pi / 3.0)
    ext[:3, 3] = (0.1, 0.02, -0.03)
    got = sm.assemble_map({0: k1, 1: k2}, {0: T1, 1: T2}, 0.1, sensor_to_body=ext)
    same(got, ref.assemble_map([k1[:2], k2[:2]], [T1, T2], 0.1, sensor_to_body=ext))
    quat = sm.assemble_map({0: k1}, {0: [1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0]}, 0.1)  # a pose as 7 numbers
    Tq = np.identity(4)
    Tq[:3, 3] = (1.0, 2.0, 3.0)
    same(quat, ref.assemble_map([k1[:2]], [Tq], 0.1))


def test_map_nine_keyframes_around_the_tile(sm, T):
    rng = np.random.default_rng(21)
    clouds, poses = {}, {}
    for k, n in enumerate((T - 1, T, T + 1, 1, 63, 0, 65, 2 * T + 3, 64)):
        p = rng.uniform(-0.5, 0.5, (n, 3))
        if n > 10:
            p[rng.choice(n, 3, replace=False), rng.integers(0, 3, 3)] = (np.nan, np.inf, -np.inf)      # such rows do not exist
        clouds[k] = p
        Tk = np.identity(4)
        Tk[:3, :3] = ref.rotation(rng.standard_normal(3), rng.uniform(0, 3))
        Tk[:3, 3] = rng.uniform(-1.0, 1.0, 3) + (50.0, -20.0, 3.0)
        poses[k] = Tk
    got = sm.assemble_map(clouds, poses, 0.3)
    want = ref.assemble_map([(clouds[k], None) for k in range(9)], [poses[k] for k in range(9)], 0.3)
    same(got, want)
    assert got.counts.max() > 64 and got.counts.sum() == sum(np.isfinite(c).all(axis=1).sum() for c in clouds.values())


def test_map_same_bits_alone_or_among_far_keyframes(sm, keyframes):
    k1, k2 = keyframes
    T1, T2 = ref.scene_poses()
    alone = sm.assemble_map({0: k1, 2: k2}, {0: T1, 2: T2}, 0.1)
    far1, far2 = T1.copy(), T2.copy()
    far1[:3, 3] += (-300.0, 77.0, 500.0)
    far2[:3, 3] += (40.0, -900.0, 700.0)
    among = sm.assemble_map({0: k1, 1: k2, 2: k2, 3: k1}, {0: T1, 1: far2, 2: T2, 3: far1}, 0.1)
    near = among.points[:, 2] < 100.0
    assert near.sum() == len(alone.points) and near[:near.sum()].all()             # ascending iz: the near rows come first
    same([a[near] for a in among], alone)


def test_map_identity_pose_is_the_map_rule_not_the_keyframe_filter(sm, kc, scene):
    p, c = scene
    kf = kc.voxel_subsample(p, c, 0.05, 100.0)
    got = sm.assemble_map({0: kf}, {0: np.identity(4)}, 0.1)
    same(got, ref.assemble_map([kf[:2]], [np.identity(4)], 0.1))
    # not the keyframe filter at that size: float64 means of the keyframe's rows, each row weighing the same
    direct = kc.voxel_subsample(p, c, 0.1, 100.0)
    assert len(got.points) == len(direct.points) == 457
    assert (got.points != direct.points.astype(np.float64)).any(axis=1).mean() > 0.5
    assert got.counts.sum() == len(kf.points) < direct.counts.sum()


def test_map_status_raises(sm):
    from cslam_amd.lidar_pr.voxel import VoxelSizeError
    pts = np.array([[0.0, 0.0, 0.0], [2.0 ** 21 * 0.5, 0.0, 0.0]])
    with pytest.raises(VoxelSizeError):
        sm.assemble_map({0: pts}, {0: np.identity(4)}, 0.5)
    pts[1, 0] -= 0.5
    got = sm.assemble_map({0: pts}, {0: np.identity(4)}, 0.5)
    same(got, ref.assemble_map([(pts, None)], [np.identity(4)], 0.5))
    assert len(got.points) == 2


# ---- end to end ------------------------------------------------------------------------------------------------------
QUADRANT = np.array([[[200, 30, 30], [30, 200, 30]], [[30, 30, 200], [220, 220, 40]]], dtype=np.uint8)      # (r, g, b) by (Y >= 0, X >= 0)


def render_plane(T, cam, H=48, W=64):
    """uint16 depth and B, G, R image of the plane z = 2 (world) with the quadrant texture, from the camera-to-world pose T:
    exact ray intersection in float64, depth rounded to millimetres."""
    fx, fy, cx, cy = cam
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)          # z of the camera frame = 1: s is the depth
    dw = d @ T[:3, :3].T
    s = (2.0 - T[2, 3]) / dw[..., 2]
    X, Y = T[0, 3] + s * dw[..., 0], T[1, 3] + s * dw[..., 1]
    rgb = QUADRANT[(Y >= 0).astype(int), (X >= 0).astype(int)]
    return np.ascontiguousarray(rgb[..., ::-1]), np.rint(s * 1000.0).astype(np.uint16)


def test_end_to_end_plane_from_three_poses(kc, sm):
    """Bounds: a depth is off by at most 0.5 mm along its ray, whose world direction has a z component of at most |d| <= 1.06
    for this camera, so a point lies within 0.53 mm of the plane, plus float32 spacing at 2 m (2.4e-4 mm) in the four float32
    operations of the projection; a centroid is a mean of such points: 1 mm holds."""
    cam = (120.0, 120.0, 31.5, 23.5)
    poses = {}
    for k, (angle, t) in enumerate(((-0.1, (-0.1, 0.0, 0.0)), (0.0, (0.0, 0.01, 0.0)), (0.1, (0.1, 0.0, 0.02)))):
        Tk = np.identity(4)
        Tk[:3, :3] = ref.rotation((0.0, 1.0, 0.0), angle)
        Tk[:3, 3] = t
        poses[(0, k)] = Tk
    frames = [render_plane(poses[key], cam) for key in sorted(poses)]
    clouds = kc.keyframe_clouds([f[0] for f in frames], [f[1] for f in frames], cam, 0.02, 3.0)
    assert all(len(c.points) > 500 for c in clouds)
    swarm = sm.assemble_map(dict(zip(sorted(poses), clouds)), poses, 0.05)
    off = np.abs(swarm.points[:, 2] - 2.0).max()
    print("largest distance of a map centroid from the plane: %.4f mm over %d rows" % (off * 1e3, len(swarm.points)))
    assert off <= 1e-3
    # A map voxel (0.05) holds keyframe centroids (of voxels of 0.02, which mix colours where they straddle a texture edge):
    # further than 0.05 + 0.02 (plus the point error) from both edges, every pixel behind a map row is of one quadrant.
    X, Y = swarm.points[:, 0], swarm.points[:, 1]
    interior = (np.abs(X) > 0.072) & (np.abs(Y) > 0.072)
    assert interior.sum() > 100
    assert np.array_equal(swarm.colors[interior], QUADRANT[(Y[interior] >= 0).astype(int), (X[interior] >= 0).astype(int)])
    assert len({tuple(c) for c in swarm.colors[interior]}) == 4
    assert len(swarm.points) < sum(len(c.points) for c in clouds)
    # a pose that was not applied must show: 5 cm along z on one keyframe
    moved = dict(poses)
    moved[(0, 1)] = poses[(0, 1)].copy()
    moved[(0, 1)][2, 3] += 0.05
    wrong = sm.assemble_map(dict(zip(sorted(poses), clouds)), moved, 0.05)
    assert np.abs(wrong.points[:, 2] - 2.0).max() > 1e-3
