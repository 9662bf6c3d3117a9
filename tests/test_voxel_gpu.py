"""GPU: batched voxel down-sampling (csrc/voxel.hip through cslam_amd.lidar_pr.icp_utils.downsample / downsample_clouds and
lidar_pr.keyframes.ingest) against `icp_reference.voxel_average`, the numpy statement of open3d's rule.  The rule fixes
the index arithmetic and the order of every sum, so all comparisons are np.array_equal on float64 arrays: no tolerance.
The sizes sit around T, the keys a workgroup sorts per radix pass, and B, the threads per workgroup of the kernel that
sums a voxel.  tests/test_voxel_cpu.py pins the CPU-side facts used here (the order discrimination, the index values
at the key range's edge)."""
import numpy as np
import pytest

import icp_reference as ref

pytestmark = pytest.mark.gpu

VOXEL = 0.5


@pytest.fixture(scope="module")
def vox():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


def keys_of(cloud, voxel):
    pts = np.asarray(cloud, dtype=np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    return np.floor((pts - (pts.min(axis=0) - voxel / 2.0)) / voxel).astype(np.int64)


def same(got, want):
    return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)


@pytest.fixture(scope="module")
def sized(vox):
    """Uniform clouds in [-1, 1]^3 of the sizes around the sort tile, with their expected results, computed once."""
    T = vox.VOXEL_TILE
    rng = np.random.default_rng(21)
    clouds = [rng.uniform(-1.0, 1.0, (n, 3)) for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5)]
    return clouds, [ref.voxel_average(c, VOXEL) for c in clouds]


def test_sizes_alone_and_batched(vox, sized):
    clouds, want = sized
    single = [vox.downsample(c, VOXEL) for c in clouds]
    for c, g, w in zip(clouds, single, want):
        assert same(g, w), len(c)
    mid = len(clouds) // 2
    batch = vox.downsample_clouds(clouds[:mid] + [np.zeros((0, 3))] + clouds[mid:], VOXEL)
    assert batch[mid].shape == (0, 3) and batch[mid].dtype == np.float64
    del batch[mid]
    for c, g, s, w in zip(clouds, batch, single, want):
        assert same(g, w), len(c)
        assert np.array_equal(g, s), len(c)


def test_sum_is_in_cloud_order(vox):
    pts = np.random.default_rng(5).uniform(-1.0, 1.0, (3000, 3))
    fwd, rev = ref.voxel_average(pts, VOXEL), ref.voxel_average(pts[::-1], VOXEL)
    assert fwd.shape == rev.shape == (125, 3)
    differ = np.mean((fwd != rev).any(axis=1))
    print("voxels whose mean depends on the order of the sum: %.2f" % differ)
    assert differ >= 0.5                                     # the comparison below can see a wrong order
    assert same(vox.downsample(pts, VOXEL), fwd)
    assert same(vox.downsample(pts[::-1], VOXEL), rev)


def test_one_voxel_of_many_points_and_one_point_per_voxel(vox):
    rng = np.random.default_rng(6)
    heavy = rng.uniform(0.0, 0.2, (5000, 3))                 # one voxel: longer than B and than T
    assert 5000 > vox.VOXEL_TILE and 5000 > vox.VOXEL_SEG_BLOCK
    want = ref.voxel_average(heavy, VOXEL)
    assert want.shape == (1, 3)
    got, cnt = vox.downsample_clouds([heavy], VOXEL, counts=True)[0]
    assert same(got, want) and list(cnt) == [5000]
    g = np.arange(10) * VOXEL                                # a 10 x 10 x 10 lattice at voxel-centre spacing
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lattice = lattice[rng.permutation(len(lattice))]
    want = ref.voxel_average(lattice, VOXEL)
    assert want.shape == (1000, 3)
    got, cnt = vox.downsample_clouds([lattice], VOXEL, counts=True)[0]
    assert same(got, want) and np.array_equal(cnt, np.ones(1000, dtype=np.int64))
    both = vox.downsample_clouds([lattice, heavy, lattice], VOXEL)
    assert same(both[0], want) and same(both[2], want) and same(both[1], ref.voxel_average(heavy, VOXEL))


def test_floor_and_boundaries(vox):
    rng = np.random.default_rng(9)
    # negative coordinates, points exactly on voxel faces: with the minimum at -1.75 the faces are the multiples of 0.5
    faces = np.concatenate([[[-1.75, -1.75, -1.75]], rng.integers(-3, 5, (400, 3)) * 0.5])
    k = keys_of(faces, VOXEL)
    assert np.array_equal((faces[1:] + 2.0) / VOXEL, k[1:])                      # exact integers: the points are on faces
    # 0.25 and the double below it, minimum 0: both in index 1 (the sum 0.24999999999999997 + 0.25 rounds to 0.5)
    pair = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.24999999999999997, 0.0, 0.0]])
    assert list(keys_of(pair, VOXEL)[:, 0]) == [0, 1, 1]
    dup = np.repeat(rng.uniform(-3.0, -1.0, (150, 3)), 3, axis=0)[rng.permutation(450)]
    odd = rng.uniform(-1.0, 1.0, (700, 3))
    cases = [(faces, VOXEL), (pair, VOXEL), (dup, VOXEL), (odd, 0.3), (faces, 0.3), (-np.abs(odd) * 40.0, 0.3)]
    for cloud, voxel in cases:
        assert same(vox.downsample(cloud, voxel), ref.voxel_average(cloud, voxel)), voxel
    got = vox.downsample_clouds([c for c, v in cases if v == 0.3], 0.3)
    for g, c in zip(got, [c for c, v in cases if v == 0.3]):
        assert same(g, ref.voxel_average(c, 0.3))


def test_non_finite_rows_do_not_exist(vox):
    rng = np.random.default_rng(10)
    base = rng.uniform(-1.0, 1.0, (300, 3))
    clouds = []
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            row = np.zeros(3)
            row[col] = bad
            low = np.full(3, -5.0)                           # the minimum of the other columns, if the row counted
            low[col] = bad
            clouds += [np.concatenate([[row], base]), np.concatenate([base, [row]]),
                       np.concatenate([base[:100], [low], base[100:]])]
    want = [ref.voxel_average(c, VOXEL) for c in clouds]
    assert all(np.array_equal(w, want[0]) for w in want)     # the reference filters them: the clean cloud's result
    for g, w in zip(vox.downsample_clouds(clouds, VOXEL), want):
        assert same(g, w)
    for k in (0, 13, 26):
        assert same(vox.downsample(clouds[k], VOXEL), want[k])
    many = np.concatenate([base, np.full((70, 3), np.nan)])[rng.permutation(370)]
    got, cnt = vox.downsample_clouds([many], VOXEL, counts=True)[0]
    assert same(got, ref.voxel_average(many, VOXEL)) and cnt.sum() == 300
    # a cloud without a finite row: no rows, no error, alone and in a batch
    nothing = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]])
    assert vox.downsample(nothing, VOXEL).shape == (0, 3)
    got = vox.downsample_clouds([base, nothing, clouds[5]], VOXEL)
    assert same(got[0], want[0]) and got[1].shape == (0, 3) and same(got[2], want[5])


def test_key_range(vox):
    top = (2 ** 21 - 1) * VOXEL
    for axis in range(3):
        pts = np.zeros((2, 3))
        pts[1, axis] = top
        assert list(keys_of(pts, VOXEL)[:, axis]) == [0, 2 ** 21 - 1]
        got = vox.downsample(pts[::-1], VOXEL)
        assert same(got, ref.voxel_average(pts, VOXEL)) and np.array_equal(got, pts)     # two rows, in index order
    # all three axes at their widest: 63 key bits, every radix pass runs
    rng = np.random.default_rng(12)
    wide = np.concatenate([[[0.0, 0.0, 0.0], [top, top, top]], rng.integers(0, 2 ** 21, (500, 3)) * VOXEL])
    wide = np.concatenate([wide, wide[2:200] + 0.125])[rng.permutation(700)]
    assert keys_of(wide, VOXEL).max(axis=0).tolist() == [2 ** 21 - 1] * 3
    small = rng.uniform(-1.0, 1.0, (500, 3))
    got = vox.downsample_clouds([small, wide, small], VOXEL)
    assert same(got[1], ref.voxel_average(wide, VOXEL)) and same(got[0], ref.voxel_average(small, VOXEL))
    assert np.array_equal(got[0], got[2])
    # one index further: the cloud is refused, the other cloud of the batch is not affected
    for axis in range(3):
        over = np.zeros((2, 3))
        over[1, axis] = 2 ** 21 * VOXEL
        assert keys_of(over, VOXEL)[1, axis] == 2 ** 21
        with pytest.raises(ValueError, match="voxel_size is too small") as err:
            vox.downsample_clouds([small, over], VOXEL)
        assert err.value.failed == [1] and err.value.clouds[1] is None
        assert same(err.value.clouds[0], ref.voxel_average(small, VOXEL))
    with pytest.raises(ValueError, match="cloud 0"):
        vox.downsample(over, VOXEL)


class _Cloud:
    def __init__(self, points):
        self.points = points


def test_dtypes_forms_and_counts(vox):
    rng = np.random.default_rng(13)
    f32 = rng.uniform(-4.0, 4.0, (1500, 3)).astype(np.float32)
    want = ref.voxel_average(f32.astype(np.float64), VOXEL)
    assert same(vox.downsample(f32, VOXEL), want)
    assert same(vox.downsample(_Cloud(f32.astype(np.float64)), VOXEL), want)
    wide = np.concatenate([f32.astype(np.float64), rng.uniform(0, 1, (1500, 2))], axis=1)      # [n, 5]: x, y, z + intensity, ring
    wide[::50, 1] = np.nan
    got, cnt = vox.downsample_clouds([wide, f32], VOXEL, counts=True)[0]
    assert same(got, ref.voxel_average(wide[:, :3], VOXEL))
    _, ucnt = np.unique(keys_of(wide[:, :3], VOXEL), axis=0, return_counts=True)
    assert cnt.dtype == np.int64 and cnt.sum() == 1500 - 30 and np.array_equal(cnt, ucnt)
    assert vox.downsample_clouds([], VOXEL) == []
    with pytest.raises(ValueError):
        vox.downsample(np.zeros((4, 2)), VOXEL)


@pytest.fixture(scope="module")
def raw_street():
    """The two raw scans of `street_scene` (9 000 raw points), without its final averaging."""
    keep = ref.voxel_average
    ref.voxel_average = lambda pts, voxel: np.asarray(pts)
    try:
        src, dst, T_true, yaw = ref.street_scene(100, 9000, VOXEL)
    finally:
        ref.voxel_average = keep
    return src, dst, yaw, T_true


def test_keyframes_ingest(vox, raw_street):
    from cslam_amd.lidar_pr import keyframes
    from cslam_amd.lidar_pr.scancontext import ScanContext
    rng = np.random.default_rng(14)
    clouds = [raw_street[0][:3000], raw_street[1][:2500].astype(np.float32), rng.uniform(-20, 20, (700, 3))]
    desc, down = keyframes.ingest(clouds, VOXEL)
    want_desc = ScanContext({}, None).compute_embeddings(clouds)
    assert desc.dtype == np.float64 and desc.shape == want_desc.shape == (3, 1200) and np.array_equal(desc, want_desc)
    assert np.count_nonzero(desc) > 100
    for g, w, c in zip(down, vox.downsample_clouds(clouds, VOXEL), clouds):
        assert same(g, w) and same(g, ref.voxel_average(c, VOXEL))
    on_360 = np.array([[1.0, -1e-300, 0.0], [2.0, 1.0, 0.5]])         # 360 - atan(1e-300) rounds to 360: the reference's IndexError
    with pytest.raises(IndexError) as sc_err:
        ScanContext({}, None).compute_embeddings([on_360])
    with pytest.raises(IndexError) as err:
        keyframes.ingest([clouds[2], on_360], VOXEL)
    assert str(err.value) == str(sc_err.value)


def test_end_to_end_registration_from_raw_scans(vox, raw_street):
    src, dst, yaw, T_true = raw_street
    down = vox.downsample_clouds([src, dst], VOXEL)
    want = [ref.voxel_average(src, VOXEL), ref.voxel_average(dst, VOXEL)]
    assert same(down[0], want[0]) and same(down[1], want[1]) and len(want[0]) < len(src)
    seed = 360.0 - ref.seed_yaw(yaw)
    a = vox.register_pairs([(down[0], down[1])], VOXEL, seed)[0]
    b = vox.register_pairs([(want[0], want[1])], VOXEL, seed)[0]
    assert np.array_equal(a.transformation, b.transformation) and a.iterations == b.iterations
    assert a.fitness == b.fitness and a.correspondences == b.correspondences
    # the scene and the seed of test_icp_cpu.test_staged_restatement_recovers_the_ground_truth (seed 100), and its bounds
    assert ref.rotation_error_deg(a.transformation[:3, :3], T_true[:3, :3]) <= 0.1
    assert np.linalg.norm(a.transformation[:3, 3] - T_true[:3, 3]) <= VOXEL / 5


def test_scratch_is_carved_afresh_for_every_batch(vox):
    """One stream, so one head block and one sort block: a cloud of 29 points (every piece but the histograms shorter than
    256 bytes), then three larger clouds with an empty one among them, then the small cloud again.  Both small results equal,
    byte for byte, the one computed before anything else here, and the reference."""
    import torch
    rng = np.random.default_rng(51)
    small = [rng.uniform(-1.0, 1.0, (29, 3))]
    large = [rng.uniform(-1.0, 1.0, (300, 3)), np.zeros((0, 3)), rng.uniform(-2.0, 2.0, (517, 3))]

    def raw(clouds):
        return b"".join(g.tobytes() + c.tobytes() for g, c in vox.downsample_clouds(clouds, VOXEL, counts=True))

    first = raw(small)
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [raw(small), raw(large), raw(small)]
    assert runs[0] == first and runs[2] == first and runs[1] == raw(large)
    assert first.startswith(ref.voxel_average(small[0], VOXEL).tobytes())


# ---- the lidar call as a caller of the one filter chain (csrc/cloud.hip) ------------------------------------------------
def _raw_call(clouds, voxel, host_offsets=True, device_offsets=None):
    """`cslam_voxel_downsample_dev` through `_lib` directly: (return code, every output as bytes).  `device_offsets`
    replaces the offsets on the device; the host copy is given or not."""
    import ctypes as C
    import torch
    from cslam_amd import _lib
    from cslam_amd.lidar_pr._batch import stream, to_dev, upload
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    cl = upload([np.ascontiguousarray(c, dtype=np.float64) for c in clouds], dev)
    n, total = len(clouds), int(cl.off[-1])
    d_off = cl.d_off if device_offsets is None else to_dev(np.asarray(device_offsets, dtype=np.int64), dev)
    outs = [torch.zeros(max(k, 1), dtype=torch.uint8, device=dev) for k in (24 * total, 8 * (n + 1), 4 * total, 4 * n)]
    rc = lib.cslam_voxel_downsample_dev(cl.rows, d_off if isinstance(d_off, int) else d_off.data_ptr(), n, float(voxel),
                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                        cl.off.ctypes.data_as(C.c_void_p) if host_offsets else None, stream())
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy().tobytes() for o in outs]


def _lattice_cloud(rng, bits):
    """At most 64 rows on the voxel lattice (voxel 0.5, minimum 0: a row's index is its coordinate / 0.5) whose largest
    index on axis a is 2^bits[a] - 1: the origin, the top index on each axis, all three at once, seeded rows and a few
    second rows inside the same voxels."""
    top = np.array([2 ** b - 1 for b in bits])
    idx = rng.integers(0, top + 1, (40, 3))
    for a in range(3):
        idx[a, a] = top[a]
    pts = np.concatenate([[[0, 0, 0], top], idx]).astype(np.float64) * VOXEL
    pts = np.concatenate([pts, pts[5:20] + 0.125])
    return pts[rng.permutation(len(pts))]


def test_key_shifts_at_and_across_32_bits(vox):
    """Keys are packed from 32-bit shifts: per-cloud widths whose shifts (by + bz, bz) sit below, at and beyond 32."""
    rng = np.random.default_rng(77)
    widths = [(3, 21, 10), (3, 21, 11), (3, 12, 21), (3, 21, 21)]
    clouds = [_lattice_cloud(rng, b) for b in widths]
    for c, b in zip(clouds, widths):
        assert len(c) <= 64 and keys_of(c, VOXEL).max(axis=0).tolist() == [2 ** k - 1 for k in b]
    assert [(b[1] + b[2], b[2]) for b in widths] == [(31, 10), (32, 11), (33, 21), (42, 21)]
    want = [ref.voxel_average(c, VOXEL) for c in clouds]
    assert all(len(w) == 42 for w in want)                  # 57 rows, 15 of them second rows of a voxel
    for c, w in zip(clouds, want):
        assert same(vox.downsample(c, VOXEL), w)
    for g, w in zip(vox.downsample_clouds(clouds, VOXEL), want):      # per-cloud widths differ inside one launch
        assert same(g, w)


def test_without_host_offsets(vox):
    """h_offsets == NULL: the bounds pass runs on offsets the host has not seen, which are read back before the one wait
    and checked after it.  Same bytes as with host offsets; decreasing device offsets are refused with the usual message
    after a bounds pass that stayed inside the rows."""
    from cslam_amd import _lib
    rng = np.random.default_rng(78)
    big = rng.uniform(-1.0, 1.0, (vox.VOXEL_TILE + 1, 3))
    big[17] = [0.0, np.nan, 0.0]
    clouds = [np.zeros((0, 3)), rng.uniform(-1.0, 1.0, (1, 3)), big]
    rc_h, with_host = _raw_call(clouds, VOXEL, True)
    rc_d, without = _raw_call(clouds, VOXEL, False)
    assert rc_h == 0 and rc_d == 0
    assert without == with_host
    n_out = np.frombuffer(with_host[1], dtype=np.int64)
    assert n_out[:3].tolist() == [0, 0, 1] and n_out[3] == 1 + len(ref.voxel_average(big, VOXEL))
    got = np.frombuffer(with_host[0], dtype=np.float64).reshape(-1, 3)[1:n_out[3]]
    assert same(got, ref.voxel_average(big, VOXEL))
    total = len(big) + 1
    rc, _ = _raw_call(clouds, VOXEL, False, device_offsets=[0, total, 1, total])      # every row read is a row of the buffer
    assert rc == -1 and _lib.load().cslam_last_error() == b"invalid argument: offsets must not decrease"
    rc, again = _raw_call(clouds, VOXEL, False)                                         # and the next call is not affected
    assert rc == 0 and again == with_host


def _plan_info(n, n_clouds, key_bits):
    T = 2048
    return [-(-key_bits // 8), -(-(n_clouds - 1).bit_length() // 8), key_bits, -(-n // T)]


def test_profiles_of_the_lidar_and_the_cloud_calls_do_not_mix(vox):
    """One profile type, two instances: each read gives the stage times and the plan of the last call of its own family,
    whatever the other family ran in between."""
    import ctypes as C
    from cslam_amd import _lib
    from cslam_amd.front_end import keyframe_clouds as kc
    lib = _lib.load()
    rng = np.random.default_rng(79)
    lidar = _lattice_cloud(rng, (3, 5, 4))[:40]
    lidar = np.concatenate([lidar, rng.integers(0, 8, (vox.VOXEL_TILE + 1 - 40, 3)) * VOXEL])      # two sort tiles, 12 key bits
    assert keys_of(lidar, VOXEL).max(axis=0).tolist() == [7, 31, 15]
    small = (rng.integers(0, 4, (50, 3)) * 0.5).astype(np.float32)                  # one tile; PCL rule, leaf 0.5: 2 bits an axis
    small[:2] = [[0, 0, 0], [1.5, 1.5, 1.5]]

    def read(fn, k):
        ms, info = (C.c_double * k)(), (C.c_int32 * 4)()
        _lib.check(fn(C.byref(ms), C.byref(info)))
        assert all(np.isfinite(t) and t >= 0.0 for t in ms)
        return list(info)

    _lib.check(lib.cslam_voxel_profile(1))
    _lib.check(lib.cslam_cloud_profile(1))
    try:
        want = vox.downsample(lidar, VOXEL)
        kc.voxel_subsample(small, None, 0.5, 10.0)
        assert read(lib.cslam_voxel_profile_read, 6) == _plan_info(len(lidar), 1, 12)
        assert read(lib.cslam_cloud_profile_read, 7) == _plan_info(len(small), 1, 6)
        kc.voxel_subsample(small, None, 0.5, 10.0)
        assert same(vox.downsample(lidar, VOXEL), want)
        assert read(lib.cslam_cloud_profile_read, 7) == _plan_info(len(small), 1, 6)
        assert read(lib.cslam_voxel_profile_read, 6) == _plan_info(len(lidar), 1, 12)
    finally:
        _lib.check(lib.cslam_voxel_profile(0))
        _lib.check(lib.cslam_cloud_profile(0))
    assert same(want, ref.voxel_average(lidar, VOXEL))
    assert lib.cslam_voxel_profile_read(C.byref((C.c_double * 6)()), C.byref((C.c_int32 * 4)())) == -1      # switched off: nothing to read


def test_lidar_and_keyframe_cloud_calls_share_their_scratch(vox):
    """One stream, one pair of scratch blocks for both families: a lidar call of VOXEL_TILE + 1 points, a keyframe-cloud
    call of 8 x 8 pixels, the lidar call again.  All three equal what they give alone, byte for byte."""
    import torch
    import cloud_reference as cref
    from cslam_amd.front_end import keyframe_clouds as kc
    rng = np.random.default_rng(80)
    lidar = [rng.uniform(-1.0, 1.0, (vox.VOXEL_TILE + 1, 3))]
    img, depth = cref.scene_image(8, 8), cref.scene_depth(8, 8)

    def raw_lidar():
        return b"".join(g.tobytes() + c.tobytes() for g, c in vox.downsample_clouds(lidar, VOXEL, counts=True))

    def raw_frame():
        c = kc.keyframe_clouds([img], [depth], cref.SCENE_CAMERA, 0.05, 2.0)[0]
        return c.points.tobytes() + c.colors.tobytes() + c.counts.tobytes()

    alone = [raw_lidar(), raw_frame()]
    assert alone[0].startswith(ref.voxel_average(lidar[0], VOXEL).tobytes())
    want = cref.keyframe_cloud(img, depth, cref.SCENE_CAMERA, 0.05, 2.0)
    assert len(want[0]) > 0 and alone[1].startswith(want[0].tobytes())
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [raw_lidar(), raw_frame(), raw_lidar()]
    assert runs == [alone[0], alone[1], alone[0]]
