"""GPU: FPFH features and mutual matches (csrc/fpfh.hip through cslam_amd.lidar_pr.icp_utils) against the float64
restatement of the rules in tests/fpfh_reference.py.  The shapes are the smallest at which the kernels can still go
wrong: sizes around a wave, the LDS chunks and the candidate buffer.  tests/test_fpfh_cpu.py checks that the decisions
compared here (list order, the sign of a normal, histogram bins away from edge-close pairs) do not hang on the last bits."""
import numpy as np
import pytest

import fpfh_reference as ref
from test_fpfh_cpu import E2E_SEED, E2E_SHARE

pytestmark = pytest.mark.gpu

V = ref.VOXEL


@pytest.fixture(scope="module")
def u():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


@pytest.fixture(scope="module")
def scenes():
    return {s: ref.feature_scene(s) for s in ref.SCENE_SEEDS}


@pytest.fixture(scope="module")
def scene_gpu(u, scenes):
    """Scene 1 through the staged public calls, once: normals, lists, (FPFH, SPFH)."""
    pts = scenes[1]
    normals = u.estimate_normals(pts, 2 * V, 30)
    lists = u.radius_neighbors(pts, 5 * V, 100)
    fpfh, spfh = u.compute_fpfh_feature(pts, normals, 5 * V, 100, return_spfh=True)
    return pts, normals, lists, fpfh, spfh


def check_lists(got, want):
    (idx, d2, count), (w_idx, w_d2, w_count) = got, want
    assert idx.dtype == np.int32 and count.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(count, w_count)
    assert np.array_equal(idx, w_idx)
    np.testing.assert_allclose(d2, w_d2, rtol=1e-15, atol=0.0)       # the padding is +inf in both


# ---- neighbour lists -------------------------------------------------------------------------------------------------
def test_lists_at_sizes_around_a_wave_and_the_chunk(u):
    rng = np.random.default_rng(5)
    ch = u.KNN_CHUNK
    clouds = [rng.standard_normal((n, 3)) for n in (1, 2, 3, 63, 64, 65, ch - 1, ch, ch + 1, 2 * ch + 5)]
    got = u.radius_neighbors_clouds(clouds, 0.7, 30)
    cut = 0
    for pts, g in zip(clouds, got):
        want = ref.radius_neighbors(pts, 0.7, 30)
        check_lists(g, want)
        cut += int((want[2] == 30).sum())
    assert cut > 100 and got[0][0].tolist() == [[0] + [-1] * 29]
    check_lists(u.radius_neighbors(clouds[-1], 0.7, 30), got[-1])                  # alone = in the batch, bit for bit
    assert np.array_equal(u.radius_neighbors(clouds[-1], 0.7, 30)[1], got[-1][1])


def test_isolated_point_and_lists_of_exactly_max_nn(u):
    rng = np.random.default_rng(6)
    max_nn = 12
    ball = 0.1 * rng.standard_normal((max_nn, 3))                   # max_nn points within the radius of each other
    far = np.array([[50.0, 0.0, 0.0]])
    for extra in (0, 1):                                            # exactly max_nn in radius, and max_nn + 1
        pts = np.concatenate([ball, 0.1 * rng.standard_normal((extra, 3)), far])
        got = u.radius_neighbors(pts, 5.0, max_nn)
        check_lists(got, ref.radius_neighbors(pts, 5.0, max_nn))
        assert got[0][-1].tolist() == [len(pts) - 1] + [-1] * (max_nn - 1) and got[2][-1] == 1     # the far point: [self]
        assert (got[2][:-1] == max_nn).all()
    one = u.radius_neighbors(pts, 5.0, 1)                           # max_nn = 1: every list is [self]
    assert one[0].tolist() == [[i] for i in range(len(pts))] and (one[2] == 1).all() and not one[1].any()


@pytest.mark.parametrize("max_nn", (100, 256))
def test_more_in_radius_points_than_the_candidate_buffer(u, max_nn):
    rng = np.random.default_rng(8)
    n = 2 * u.KNN_CAND + 70                                         # the buffer is cut more than once on the way
    pts = np.concatenate([rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(5.0, 6.0, (7, 3))])
    pts = pts[rng.permutation(len(pts))]
    want = ref.radius_neighbors(pts, 1.1, max_nn)
    assert (want[2] == max_nn).sum() == n
    check_lists(u.radius_neighbors(pts, 1.1, max_nn), want)


def test_lattice_with_exact_distances_ties_and_the_radius_itself(u):
    g = np.arange(5) * 0.5
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([1.0, -2.0, 0.5])
    got = u.radius_neighbors(pts, 1.0, 40)
    want = ref.radius_neighbors(pts, 1.0, 40)
    check_lists(got, want)
    assert np.array_equal(got[1], want[1])                          # 0.25, 0.5, 0.75, 1.0: exact
    assert got[2].max() == 33 and (got[1] == 1.0).sum() > 0         # an inner point: 6 + 12 + 8 + 6 others, d2 == r2 included
    inner = int(np.argmax(got[2]))
    assert np.all(np.diff(got[0][inner, 1:7]) > 0)                  # the six at 0.25: by index


def test_duplicates_of_the_query_come_after_it(u):
    rng = np.random.default_rng(9)
    pts = rng.standard_normal((40, 3))
    pts[[3, 17, 30]] = pts[11]
    got = u.radius_neighbors(pts, 0.9, 10)
    check_lists(got, ref.radius_neighbors(pts, 0.9, 10))
    assert got[0][17, :4].tolist() == [17, 3, 11, 30] and got[1][17, :4].tolist() == [0.0] * 4
    assert got[0][3, :4].tolist() == [3, 11, 17, 30]


def test_batch_with_an_empty_cloud_equals_the_singles(u, scenes):
    clouds = [scenes[1][:300], np.zeros((0, 3)), scenes[2][:517], np.array([[np.nan, 0.0, 0.0]])]
    batch = u.radius_neighbors_clouds(clouds, 5 * V, 100)
    for c, b in zip(clouds, batch):
        single = u.radius_neighbors(c, 5 * V, 100)
        assert all(np.array_equal(x, y) for x, y in zip(single, b))
    assert batch[1][0].shape == (0, 100) and batch[3][2].shape == (0,)


# ---- normals ---------------------------------------------------------------------------------------------------------
def test_normals_of_the_scene(u, scenes, scene_gpu):
    pts, normals = scene_gpu[0], scene_gpu[1]
    want = ref.estimate_normals(pts, *ref.radius_neighbors(pts, 2 * V, 30), 2 * V, 30)
    worst = float(ref.angles(normals, want).max())
    print("largest angle to the restatement: %.2e rad" % worst)
    assert worst <= 1e-9
    assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-15
    assert ((normals * -pts).sum(axis=1) > 0).all()
    below = (13.0, 9.5, -30.0)                                      # a viewpoint under the ground turns the ground's normals over
    flipped = u.estimate_normals(pts, 2 * V, 30, viewpoint=below)
    assert float(ref.angles(flipped, ref.estimate_normals(pts, *ref.radius_neighbors(pts, 2 * V, 30), 2 * V, 30, below)).max()) <= 1e-9
    assert ((flipped * (np.array(below) - pts)).sum(axis=1) > 0).all()
    turned = (np.abs(ref.angles(flipped, normals) - np.pi) < 1e-6).mean()
    assert 0.3 < turned < 1.0


def test_fewer_than_three_neighbours_give_the_default_normal(u):
    pts = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [10.3, 0.1, 0.0], [20.0, 5.0, 1.0], [20.2, 5.0, 1.1], [20.1, 5.2, 1.0]])
    normals = u.estimate_normals(pts, 1.0, 30, viewpoint=(0.0, 0.0, -9.0))
    assert np.array_equal(normals[:3], [[0.0, 0.0, -1.0]] * 3)      # (0, 0, 1) exactly, then the sign
    assert np.array_equal(u.estimate_normals(pts, 1.0, 30, viewpoint=(0.0, 0.0, 9.0))[:3], [[0.0, 0.0, 1.0]] * 3)
    assert abs(np.linalg.norm(normals[3]) - 1.0) < 1e-15 and not np.array_equal(np.abs(normals[3]), [0.0, 0.0, 1.0])
    # max_nn = 2 leaves two entries however many are in the radius
    assert np.array_equal(u.estimate_normals(pts, 1.0, 2, viewpoint=(0.0, 0.0, 9.0)), [[0.0, 0.0, 1.0]] * 6)


def test_plane_lattice_and_the_side_of_the_viewpoint(u):
    g = np.arange(6) * 0.5
    plane = np.stack(np.meshgrid(g, g, [-2.0], indexing="ij"), axis=-1).reshape(-1, 3)
    assert np.array_equal(u.estimate_normals(plane, 1.2, 30), np.tile([0.0, 0.0, 1.0], (36, 1)))            # the origin is above
    assert np.array_equal(u.estimate_normals(plane, 1.2, 30, viewpoint=(1.0, 1.0, -7.0)), np.tile([0.0, 0.0, -1.0], (36, 1)))
    # a viewpoint in the plane: the product is exactly 0 and the component of largest magnitude is made positive
    assert np.array_equal(u.estimate_normals(plane, 1.2, 30, viewpoint=(40.0, -3.0, -2.0)), np.tile([0.0, 0.0, 1.0], (36, 1)))


# ---- SPFH and FPFH ---------------------------------------------------------------------------------------------------
def test_spfh_of_the_scene(scene_gpu):
    pts, normals, (idx, d2, count), _, spfh = scene_gpu
    want, n_edge = ref.compute_spfh(pts, normals, idx, count, return_edge=True)     # the GPU's own normals and lists
    clear = n_edge == 0
    share = 1.0 - clear.mean()
    print("edge-close points: %.2f %%" % (100 * share))
    assert share <= 0.05
    np.testing.assert_allclose(spfh[clear], want[clear], rtol=1e-14, atol=0.0)
    unit = 100.0 / (count - 1)
    off_by = np.abs(spfh - want) / unit[:, None]
    assert (off_by.max(axis=1) <= n_edge + 1e-9).all()
    np.testing.assert_allclose(spfh.reshape(len(pts), 3, 11).sum(axis=2), 100.0, rtol=1e-12)


def test_fpfh_of_the_scene(scene_gpu):
    pts, _, (idx, d2, count), fpfh, spfh = scene_gpu
    assert (count == 100).any() and (count < 100).any()
    np.testing.assert_allclose(fpfh, ref.compute_fpfh(spfh, idx, d2, count), rtol=1e-13, atol=0.0)


def test_fpfh_of_lonely_and_coinciding_points(u):
    pts = np.array([[0.0, 0.0, 0.0], [9.0, 0.0, 0.0], [9.0, 0.0, 0.0], [9.5, 0.0, 0.0]])
    normals = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    fpfh, spfh = u.compute_fpfh_feature(pts, normals, 1.0, 100, return_spfh=True)
    lists = u.radius_neighbors(pts, 1.0, 100)
    assert not fpfh[0].any() and not spfh[0].any()                  # k = 1: no histogram
    np.testing.assert_allclose(spfh, ref.compute_spfh(pts, normals, lists[0], lists[2]), rtol=1e-14, atol=0.0)
    np.testing.assert_allclose(fpfh, ref.compute_fpfh(spfh, *lists), rtol=1e-13, atol=0.0)      # d2 == 0 entries are skipped
    # point 1: the coinciding point's pair is the zero vector (bins 5, 5, 5), the other pair has f0 = atan2(0, 0) = 0, f1 = -1, f2 = 0
    assert spfh[1, 5] == 100.0 and spfh[1, 16] == 50.0 and spfh[1, 11] == 50.0 and spfh[1, 27] == 100.0


# ---- extract_fpfh ----------------------------------------------------------------------------------------------------
def test_extract_fpfh_equals_its_stages(u, scenes, scene_gpu):
    assert np.array_equal(u.extract_fpfh(scenes[1], V), scene_gpu[3])               # one search there, two searches here
    shifted = (1.0, -2.0, 3.0)
    staged = u.compute_fpfh_feature(scenes[2], u.estimate_normals(scenes[2], 2 * V, 30, viewpoint=shifted), 5 * V, 100)
    assert np.array_equal(u.extract_fpfh(scenes[2], V, viewpoint=shifted), staged)


def test_extract_fpfh_clouds_equals_the_singles(u, scenes, scene_gpu):
    clouds = [scenes[2], scenes[1][:400], np.zeros((0, 3)), scenes[1]]
    batch = u.extract_fpfh_clouds(clouds, V)
    assert np.array_equal(batch[3], scene_gpu[3]) and batch[2].shape == (0, 33)
    assert np.array_equal(batch[0], u.extract_fpfh(scenes[2], V)) and np.array_equal(batch[1], u.extract_fpfh(scenes[1][:400], V))


# ---- matching --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feature_sets(u):
    rng = np.random.default_rng(12)
    # around the block and the chunk; more chunks than chunk lanes (a lane walks several) in the two largest
    sizes = sorted({1, u.FM_BLOCK - 1, u.FM_BLOCK, u.FM_BLOCK + 1, u.FM_CHUNK - 1, u.FM_CHUNK + 1, 2 * u.FM_CHUNK + 3,
                    u.FM_MAX_LANES * u.FM_CHUNK + 5, 2 * u.FM_MAX_LANES * u.FM_CHUNK + u.FM_CHUNK + 7})
    return {n: rng.standard_normal((n, 33)) for n in sizes}


def test_matching_at_sizes_around_the_block_and_the_chunk(u, feature_sets):
    sizes = list(feature_sets)
    pairs = [(feature_sets[a], feature_sets[b]) for a in sizes for b in sizes if a in (1, sizes[-1]) or b in (1, sizes[-2], sizes[-1])]
    got = u.find_correspondences_pairs(pairs)
    plain = u.find_correspondences_pairs(pairs, mutual_filter=False)
    for (a, b), (i0, i1), (p0, p1) in zip(pairs, got, plain):
        nn01, nn10 = ref.match_argmin(a, b), ref.match_argmin(b, a)
        assert np.array_equal(p1, nn01) and np.array_equal(p0, np.arange(len(a)))
        assert np.array_equal(nn01, ref.match_kdtree(a, b))
        w0, w1 = ref.mutual(nn01, nn10)
        assert np.array_equal(i0, w0) and np.array_equal(i1, w1) and i0.dtype == np.int64
    a, b = pairs[-1]                                                # batched = single
    assert np.array_equal(u.find_knn(a, b), plain[-1][1]) and np.array_equal(u.find_knn(b, a), ref.match_kdtree(b, a))
    single = u.find_correspondences(a, b)
    assert np.array_equal(single[0], got[-1][0]) and np.array_equal(single[1], got[-1][1])
    # the mutual pairs are the reference's logic on the GPU's own two arrays
    w0, w1 = ref.mutual(u.find_knn(a, b), u.find_knn(b, a))
    assert np.array_equal(single[0], w0) and np.array_equal(single[1], w1)


def test_many_small_pairs_in_one_call(u):
    """Enough pairs that the launch needs one chunk lane only (the lanes fill the device when the pairs do not), with
    targets of one, two and three chunks."""
    rng = np.random.default_rng(14)
    sizes = (1, 2, u.FM_CHUNK, u.FM_CHUNK + 1, 2 * u.FM_CHUNK + 1)
    pairs = [(rng.standard_normal((sizes[k % 5], 33)), rng.standard_normal((sizes[(k // 5) % 5], 33))) for k in range(2500)]
    got = u.find_correspondences_pairs(pairs)
    for (a, b), (i0, i1) in list(zip(pairs, got))[::7]:
        w0, w1 = ref.find_correspondences(a, b)
        assert np.array_equal(i0, w0) and np.array_equal(i1, w1)
    for k in (0, 6, 13, 24, 2499):
        single = u.find_correspondences(*pairs[k])
        assert np.array_equal(single[0], got[k][0]) and np.array_equal(single[1], got[k][1])


@pytest.mark.parametrize("dim", (1, 3, 64))
def test_matching_at_other_dimensions(u, dim):
    rng = np.random.default_rng(dim)
    a, b = rng.standard_normal((300, dim)), rng.standard_normal((263, dim))
    assert np.array_equal(u.find_knn(a, b), ref.match_argmin(a, b)) and np.array_equal(u.find_knn(b, a), ref.match_kdtree(b, a))


def test_exact_ties_go_to_the_lower_index(u):
    rng = np.random.default_rng(13)
    a = rng.integers(0, 3, (300, 4)).astype(np.float64)             # 81 distinct rows: every distance is exact and most are tied
    b = rng.integers(0, 3, (290, 4)).astype(np.float64)
    nn01, nn10 = u.find_knn(a, b), u.find_knn(b, a)
    assert np.array_equal(nn01, ref.match_argmin(a, b)) and np.array_equal(nn10, ref.match_argmin(b, a))
    i0, i1 = u.find_correspondences(a, b)
    w0, w1 = ref.mutual(nn01, nn10)
    assert np.array_equal(i0, w0) and np.array_equal(i1, w1) and 0 < len(i0) < 300


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_end_to_end_share_of_true_partners(u, scenes):
    pts = scenes[E2E_SEED]
    copy, T, perm = ref.moved_copy(pts, E2E_SEED)
    f0 = u.extract_fpfh(pts, V)
    f1 = u.extract_fpfh(copy, V, viewpoint=T[:3, 3])
    idx0, idx1 = u.find_correspondences(f0, f1)
    share = ref.true_partner_share(idx0, idx1, perm, len(pts))
    print("true partners: %.5f of %d points, %d mutual matches (restatement: at least %.3f)" % (share, len(pts), len(idx0), E2E_SHARE))
    assert share >= E2E_SHARE - 0.01


def test_match_scratch_is_carved_afresh_for_every_batch(u):
    """One stream, so one scratch block: a pair of a few rows (both pieces shorter than 256 bytes), then three larger pairs
    with a one-row member, then the small pair again.  Both small results equal, byte for byte, the one computed before
    anything else here."""
    import torch
    rng = np.random.default_rng(41)
    small = [(rng.standard_normal((9, 33)), rng.standard_normal((7, 33)))]
    large = [(rng.standard_normal((300, 33)), rng.standard_normal((411, 33))), (rng.standard_normal((1, 33)), rng.standard_normal((1, 33))),
             (rng.standard_normal((257, 33)), rng.standard_normal((500, 33)))]

    def raw(pairs):
        both = u.find_correspondences_pairs(pairs) + u.find_correspondences_pairs(pairs, mutual_filter=False)
        return b"".join(i0.tobytes() + i1.tobytes() for i0, i1 in both)

    first = raw(small)
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [raw(small), raw(large), raw(small)]
    assert runs[0] == first and runs[2] == first and runs[1] == raw(large)
    (i0, i1), (w0, w1) = u.find_correspondences_pairs(small)[0], ref.find_correspondences(*small[0])
    assert np.array_equal(i0, w0) and np.array_equal(i1, w1)
