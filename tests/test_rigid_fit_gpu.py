"""GPU: the rigid fit (csrc/horn.h `icp_rigid_from_sums` behind csrc/icp.hip and csrc/robust.hip) fed directly through the
public API, against the extended-precision centred fit of tests/icp_reference.py, at the origin and far from it; and the
rest of the lidar path (voxel.hip, fpfh.hip, robust.hip, the ICP search) in two frames 2^17 m apart, bit for bit.

Handle 1 is `robust_rotation` on noise-free matches: GNC stops at iteration 0 with unit weights, so the rotation that
comes back is the plain Horn fit of the chain differences.  Handle 2 is `registration_icp(max_iteration=1)` on a pair
whose correspondences are known: the result is U . init with U the fit to them.  tests/test_rigid_fit_cpu.py holds the
cases and the input conditions (that GNC stops at 0, that no correspondence can turn, the singular-value gaps, the
dyadic exactness), and runs the same comparisons on a host build of horn.h.

The bound: moved source points within 256 ulp of the largest coordinate of the reference's (icp_reference.ULP_BOUND).
Worst values measured on the MI355X, in those ulp: handle 1 angles 4.9, planes 1.3, reflections 8.5, scales 3.0; handle 2
at the origin angles 6.3, sizes 4.4, planes 2.3, scales 7.7; far from the origin see test_updates_far_from_the_origin.
"""
import numpy as np
import pytest

import icp_reference as iref
import robust_reference as rref
from test_rigid_fit_cpu import (C_H1, Pair, angle_pairs, check_rotation, check_update, deficient_pairs, far_pairs, handle1_cases,
                                handle1_reference, robust_far_case, scale_pairs, size_pairs, worst)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def u():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


def raw(r):
    return r.transformation.tobytes() + np.array([r.fitness, r.inlier_rmse, r.correspondences, r.iterations], dtype=np.float64).tobytes()


def run_updates(u, pairs):
    """One ICP update of every pair, all pairs of one radius in one batched call; the correspondences are the known ones."""
    out = [None] * len(pairs)
    for radius in sorted({p.radius for p in pairs}):
        mine = [k for k, p in enumerate(pairs) if p.radius == radius]
        got = u.registration_icp_pairs([(pairs[k].src, pairs[k].dst) for k in mine], radius, [pairs[k].init for k in mine], max_iteration=1)
        for k, r in zip(mine, got):
            out[k] = r
    for p, r in zip(pairs, out):
        rows = np.nonzero(p.partner >= 0)[0]
        assert r.iterations == 1 and r.correspondences == len(rows), p.name
        assert np.array_equal(r.correspondence_set, np.stack([rows, p.partner[rows]], axis=1)), p.name
    return out


# ---- A: the fit against the reference, at the origin -----------------------------------------------------------------
def test_rotations_of_noise_free_matches(u):
    cases = handle1_cases()
    got = u.robust_rotation_pairs([(ms, md) for _, ms, md, _ in cases], C_H1)
    figures = []
    for (name, ms, md, unique), (R, w, it) in zip(cases, got):
        a, b, fit = handle1_reference(ms, md)
        assert it == 0 and np.array_equal(w, np.ones(len(a))), name   # the plain Horn fit of the differences
        check_rotation(name, R, a, b, fit, unique, figures)
    print("handle 1, worst moved-point error in ulp of the largest coordinate: angles %.1f, planes %.1f, reflections %.1f, "
          "scales %.1f" % (worst(figures, "angle"), worst(figures, "plane"), worst(figures, "reflection"), worst(figures, "scale")))
    name, ms, md, _ = cases[7]                                       # 180 degrees about z, alone = in the batch
    assert name == "angle-z-180" and u.robust_rotation(ms, md, C_H1)[0].tobytes() == got[7][0].tobytes()


def test_updates_at_every_angle(u):
    pairs = angle_pairs()
    figures = []
    for p, r in zip(pairs, run_updates(u, pairs)):
        check_update(p, r.transformation, figures)
    print("handle 2 at the origin, angles: worst %.1f ulp" % worst(figures))


def test_updates_at_every_sum_size_alone_and_in_one_batch(u):
    pairs = size_pairs()
    batch = run_updates(u, pairs)
    figures = []
    for p, r in zip(pairs, batch):
        check_update(p, r.transformation, figures)
        alone = run_updates(u, [p])[0]
        assert raw(alone) == raw(r), "%s differs between the batch and alone" % p.name
    print("handle 2 at the origin, sizes: worst %.1f ulp" % worst(figures))


def test_updates_of_rank_deficient_sets_and_extremes_of_scale(u):
    pairs = deficient_pairs() + scale_pairs()
    figures = []
    for p, r in zip(pairs, run_updates(u, pairs)):
        check_update(p, r.transformation, figures)
    print("handle 2 at the origin: planes worst %.1f ulp, scales worst %.1f ulp" % (worst(figures, "plane"), worst(figures, "scale")))


# ---- B: far from the origin --------------------------------------------------------------------------------------------
FAR_IDS = ["2^%d" % int(np.log2(c)) for c in iref.FAR_OFFSETS]


@pytest.mark.parametrize("c", iref.FAR_OFFSETS, ids=FAR_IDS)
def test_updates_far_from_the_origin(u, c):
    """Both clouds moved by c . (1, 0.7, 0.01) m, and the offset carried by the init.  Measured on the MI355X, worst ulp
    (sizes / angles): 2^10: 1.1 / 1.6, 2^14: 0.7 / 2.9, 2^17: 0.4 / 1.8, 2^20: 0.5 / 1.6.  With the sums taken about the
    frame origin, as they were before: 2^10: 66 / 133, 2^14: 1.8e3 / 2.8e3, 2^17: 2.3e4 / 1.4e4, 2^20: 4.1e4 / 1.5e5."""
    pairs = far_pairs(c)
    figures = []
    failed = []
    for p, r in zip(pairs, run_updates(u, pairs)):
        try:
            check_update(p, r.transformation, figures)
        except AssertionError as e:
            failed.append(str(e)[:200])
    print("handle 2 at %g m: sizes worst %.1f ulp, angles worst %.1f ulp" % (c, worst(figures, "size"), worst(figures, "angle")))
    assert not failed, failed[:3]


@pytest.fixture(scope="module")
def crop():
    return iref.street_crop()


@pytest.mark.parametrize("by_init", [False, True], ids=["both-moved", "offset-in-init"])
@pytest.mark.parametrize("c", iref.FAR_OFFSETS, ids=FAR_IDS)
def test_registration_of_a_street_crop_far_from_the_origin(u, crop, c, by_init):
    """One 100-iteration registration (15 updates).  Measured on the MI355X: at most 2.2 ulp at every offset; with the sums
    about the frame origin 89 / 94 ulp at 2^10 m, 313 / 2.7e3 at 2^14, 3.0e3 / 1.0e4 at 2^17, 3.8e5 / 2.8e4 at 2^20."""
    src, dst = crop
    off = c * iref.FAR_DIRECTION
    s, init = (src, iref.Rt2T(np.identity(3), off)) if by_init else (src + off, np.identity(4))
    want = iref.registration_icp_ld(s, dst + off, 0.5, init, 100)
    got = u.registration_icp(s, dst + off, 0.5, init, max_iteration=100)
    moved_ref = iref.moved_ld(want.transformation, s)
    ulps = float(np.abs(iref.moved_ld(got.transformation, s) - moved_ref).max()) / iref.coord_ulp(moved_ref.astype(np.float64), dst + off)
    print("street crop at %g m (%s): %d iterations (reference %d), moved points %.1f ulp from the reference's"
          % (c, "offset in init" if by_init else "both moved", got.iterations, want.iterations, ulps))
    assert got.iterations == want.iterations and np.array_equal(got.correspondence_set, want.correspondence_set)
    assert ulps <= iref.ULP_BOUND
    ortho, det = iref.rotation_defects(got.transformation[:3, :3])
    assert ortho <= 1e-14 and det <= 1e-14


# ---- C: the rest of the lidar path does not know where the origin is ------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    pts, view = iref.dyadic_scene()
    return pts, view, pts + iref.FAR_C, view + iref.FAR_C


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_neighbours_normals_and_features_in_two_frames(u, frames):
    near, view, far, view_far = frames
    lists = [u.radius_neighbors(x, 2.5, 100) for x in (near, far)]
    assert lists[0][2].max() > 30 and lists[0][2].min() >= 1
    for a, b in zip(*lists):                                         # indices, d^2, counts
        assert same(a, b)
    normals = [u.estimate_normals(x, 1.0, 30, viewpoint=v) for x, v in ((near, view), (far, view_far))]
    assert same(*normals) and np.abs(np.linalg.norm(normals[0], axis=1) - 1.0).max() <= 1e-12
    feats = [u.compute_fpfh_feature(x, normals[0], 2.5, 100, return_spfh=True) for x in (near, far)]
    assert same(feats[0][0], feats[1][0]) and same(feats[0][1], feats[1][1])
    whole = [u.extract_fpfh_clouds([x[:1000], x[400:]], 0.5, viewpoint=v) for x, v in ((near, view), (far, view_far))]
    assert same(whole[0][0], whole[1][0]) and same(whole[0][1], whole[1][1])
    matches = [u.find_correspondences(f[0], f[1]) for f in whole]
    assert len(matches[0][0]) > 100 and same(matches[0][0], matches[1][0]) and same(matches[0][1], matches[1][1])


def test_nearest_correspondences_in_two_frames(u, frames):
    near, _, far, _ = frames
    got = [u.nearest_correspondences([(x[:1000] + np.array([0.25, -0.125, 0.0625]), x[400:])], 0.3)[0] for x in (near, far)]
    assert 0.2 < np.mean(got[0][0] >= 0) < 0.9
    assert same(got[0][0], got[1][0]) and same(got[0][1], got[1][1])


def test_downsample_in_two_frames(u, frames):
    near, _, far, _ = frames
    (a, ca), (b, cb) = u.downsample_clouds([near, far], 0.5, counts=True)
    assert len(a) > 300 and ca.max() > 3 and ca.sum() == len(near)
    assert same(ca, cb) and len(a) == len(b)                         # the partition, the counts and the order
    origin = near.min(axis=0) - 0.25
    key = np.floor((near - origin) / 0.5).astype(np.int64)
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
    _, first = np.unique(key[order], axis=0, return_index=True)
    exact = np.add.reduceat(near[order].astype(iref.LD), first, axis=0) / ca[:, None]      # the in-voxel sums are exact
    assert np.abs(a.astype(iref.LD) - exact).max() <= np.spacing(np.abs(near).max())
    assert (np.abs(b.astype(iref.LD) - (exact + iref.FAR_C.astype(iref.LD))) <= np.spacing(iref.FAR_C)).all()


def test_robust_stages_in_two_frames(u):
    ms, md, T, inliers, c = robust_far_case()
    fs, fd = ms + iref.FAR_C, md + iref.FAR_C
    assert np.array_equal(fs - iref.FAR_C, ms) and np.array_equal(fd - iref.FAR_C, md)
    graphs = [u.consistency_graph(s, d, c) for s, d in ((ms, md), (fs, fd))]
    assert same(graphs[0][0], graphs[1][0]) and same(graphs[0][1], graphs[1][1])
    cliques = [u.max_clique(g[0]) for g in graphs]
    assert same(*cliques) and cliques[0].tolist() == inliers.tolist()
    rots = [u.robust_rotation(s, d, c, clique=inliers) for s, d in ((ms, md), (fs, fd))]
    assert same(rots[0][0], rots[1][0]) and same(rots[0][1], rots[1][1]) and rots[0][2] == rots[1][2]
    # the translation and the chained fit are not difference-only: equal decisions, and the moved points by the bound
    R = rots[0][0]
    R_ref = rref.gnc_rotation(ms, md, inliers, c)[0]
    trans = [u.robust_translation(s, d, R, c, clique=inliers) for s, d in ((ms, md), (fs, fd))]
    fits = [u.robust_fit_pairs([(s, d)], c)[0] for s, d in ((ms, md), (fs, fd))]
    assert np.array_equal(trans[0][1], trans[1][1])
    assert fits[0].status == fits[1].status == 0 and same(fits[0].clique, fits[1].clique) and fits[0].iterations == fits[1].iterations
    assert fits[0].clique.tolist() == inliers.tolist()
    for s, d, (t, sets), fit in ((ms, md, trans[0], fits[0]), (fs, fd, trans[1], fits[1])):
        p, q = s[inliers].astype(iref.LD), d[inliers].astype(iref.LD)
        ulp = iref.coord_ulp(s[inliers], d[inliers])
        for rot, T_got in ((R, iref.Rt2T(R, t)), (R_ref, fit.transformation)):
            x = q - p @ rot.astype(iref.LD).T                        # the scalars of the per-axis TLS, in extended precision
            sets_ref = np.stack([rref.scalar_tls(x[:, a].astype(np.float64), c)[1] for a in range(3)])
            assert np.array_equal(sets_ref, sets)                    # R and R_ref: the same sets, by the margin of the CPU file
            t_ref = np.array([x[sets_ref[a], a].mean() for a in range(3)], dtype=iref.LD)
            err = float(np.abs(iref.moved_ld(T_got, s[inliers]) - (p @ rot.astype(iref.LD).T + t_ref)).max())
            assert err <= iref.ULP_BOUND * ulp, (err / ulp)
