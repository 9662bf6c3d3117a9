"""GPU: the robust coarse fit (csrc/robust.hip through cslam_amd.lidar_pr.icp_utils) against the float64 restatement of
its rules in tests/robust_reference.py, stage by stage and chained.  The shapes are the smallest at which the kernels can
still go wrong: sizes around a 64-bit word, a wave and the LDS chunk, more than one workgroup.  No graph here has more
than 1000 vertices, so a lane of the clique search holds one word of every set, and on the planted cases the greedy clique
already is the maximum one: the search itself (which clique wins, more than 4096 vertices, widths mixed in a call, one
wave per pair, the depth limit) is compared index for index in tests/test_robust_clique_gpu.py.
tests/test_robust_cpu.py checks that the decisions compared here (edges, weight bands, stopping) do not hang on the last
bits, and that the planted cliques are the only maximum ones."""
import numpy as np
import pytest

import icp_reference as iref
import fpfh_reference as fref
import robust_reference as ref
from test_robust_cpu import (C_PLANTED, CLIQUE_CASES, DENSE_C, E2E_COARSE_DEG, E2E_COARSE_M, E2E_MIN_INLIERS, E2E_REFINED_DEG,
                             E2E_REFINED_M, E2E_SEEDS, UNRELATED)

pytestmark = pytest.mark.gpu

V = 0.5


@pytest.fixture(scope="module")
def u():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


# ---- the graph ------------------------------------------------------------------------------------------------------
def check_graph(got, ms, md, c):
    adj, deg = got
    n = len(ms)
    want = ref.consistency_graph(ms, md, c)
    assert adj.dtype == np.uint64 and adj.shape == (n, (n + 63) // 64) and deg.dtype == np.int32
    assert np.array_equal(adj, ref.to_words(want))                   # the padding bits are zero in to_words
    assert np.array_equal(deg, want.sum(axis=1))
    assert not want.diagonal().any() and np.array_equal(want, want.T)


def test_graph_at_sizes_around_a_word_and_the_chunk(u):
    ch = u.ROBUST_GRAPH_CHUNK
    cases = [ref.planted(n, n, max(n // 3, 1))[:2] for n in (2, 3, 63, 64, 65, 127, 128, 129, ch - 1, ch, ch + 1)]
    got = u.consistency_graph_pairs(cases, C_PLANTED)
    edges = 0
    for (ms, md), g in zip(cases, got):
        check_graph(g, ms, md, C_PLANTED)
        edges += int(g[1].sum())
    assert edges > 1000
    alone = u.consistency_graph(*cases[-1], C_PLANTED)               # alone = in the batch, bit for bit
    assert np.array_equal(alone[0], got[-1][0]) and np.array_equal(alone[1], got[-1][1])


def test_graph_of_a_lattice_with_exact_distances_and_the_bound_itself(u):
    ms, md = ref.lattice_case(70)
    adj, deg = u.consistency_graph(ms, md, 1.0)
    check_graph((adj, deg), ms, md, 1.0)
    bit = lambda i, j: (int(adj[i, j // 64]) >> (j % 64)) & 1
    assert bit(2, 3) == 1 and bit(3, 2) == 1                         # |b - a| == 2 c exactly: an edge
    assert bit(2, 1) == 0 and bit(1, 3) == 1 and bit(65, 67) == 1


# ---- the clique -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_in", CLIQUE_CASES)
def test_planted_clique(u, n, n_in):
    ms, md, _, inliers = ref.planted(n, n, n_in)
    adj = ref.consistency_graph(ms, md, C_PLANTED)
    clique, certified, nodes = u.max_clique(ref.to_words(adj), return_info=True)
    want, unique = ref.max_clique(adj)
    assert unique and certified
    assert clique.tolist() == want and clique.tolist() == inliers.tolist()
    via_gpu_graph = u.max_clique(u.consistency_graph(ms, md, C_PLANTED)[0])
    assert via_gpu_graph.tolist() == want


def test_two_equal_cliques_give_one_of_them_every_time(u):
    ms, md, first, second = ref.two_planted(4, 200, 25)
    adj = ref.consistency_graph(ms, md, C_PLANTED)
    size, cliques = ref.max_cliques(adj)
    assert size == 25 and len(cliques) == 2
    runs = [u.max_clique_graphs([ref.to_words(adj)] * 3) for _ in range(2)]
    one = runs[0][0][0]
    assert len(one) == 25 and ref.is_clique(adj, one) and one.tolist() in cliques
    for run in runs:
        for clique, certified, _ in run:
            assert certified and clique.tobytes() == one.tobytes()


def test_budget(u):
    ms, md = ref.dense_case()
    adj = ref.consistency_graph(ms, md, DENSE_C)
    words = ref.to_words(adj)
    size, _ = ref.max_cliques(adj)
    clique, certified, nodes = u.max_clique(words, return_info=True)
    print("dense case: clique %d, %d nodes of %d, greedy %d" % (len(clique), nodes, u.ROBUST_DEFAULT_NODE_BUDGET, len(ref.greedy_clique(adj))))
    assert certified and len(clique) == size and ref.is_clique(adj, clique) and nodes < u.ROBUST_DEFAULT_NODE_BUDGET
    assert np.all(np.diff(clique) > 0)
    clique, certified, nodes = u.max_clique(words, node_budget=16, return_info=True)
    assert not certified and ref.is_clique(adj, clique) and len(clique) >= len(ref.greedy_clique(adj))


def test_empty_and_complete_graphs_and_a_single_vertex(u):
    empty = np.zeros((70, 2), dtype=np.uint64)
    full = ref.to_words(~np.eye(130, dtype=bool))
    got = u.max_clique_graphs([empty, full, np.zeros((1, 1), dtype=np.uint64), np.zeros((0, 0), dtype=np.uint64)])
    assert got[0][0].tolist() == [0] and got[1][0].tolist() == list(range(130)) and got[2][0].tolist() == [0] and len(got[3][0]) == 0
    assert all(certified for _, certified, _ in got)


# ---- the rotation ---------------------------------------------------------------------------------------------------
def test_rotation(u):
    cases = [ref.rotation_case(m, share, seed) for m, share, seed in ref.ROTATION_CASES]
    c = cases[0][2]
    got = u.robust_rotation_pairs([(ms, md) for ms, md, _ in cases], c)
    for (ms, md, _), (R, w, it), (m, share, _) in zip(cases, got, ref.ROTATION_CASES):
        R_ref, w_ref, it_ref = ref.gnc_rotation(ms, md, np.arange(m + 1), c)
        err = float(np.abs(R - R_ref).max())
        print("rotation m = %d, outliers %.0f %%: %d iterations, |R - R_ref| = %.2e" % (m, 100 * share, it, err))
        assert it == it_ref and len(w) == m
        assert np.array_equal(w == 1.0, w_ref == 1.0) and np.array_equal(w == 0.0, w_ref == 0.0)
        assert err <= 1e-9
        assert np.abs(R @ R.T - np.identity(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
    R, w, it = got[0]                                                # all inliers: stops at it = 0 with unit weights
    assert it == 0 and np.array_equal(w, np.ones(2))
    alone = u.robust_rotation(cases[-1][0], cases[-1][1], c)
    assert alone[0].tobytes() == got[-1][0].tobytes() and alone[1].tobytes() == got[-1][1].tobytes()


def test_rotation_on_a_sublist(u):
    ms, md, _, inliers = ref.planted(300, 300, 30)
    R, w, it = u.robust_rotation(ms, md, C_PLANTED, clique=inliers)
    R_ref, w_ref, it_ref = ref.gnc_rotation(ms, md, inliers, C_PLANTED)
    assert it == it_ref and np.abs(R - R_ref).max() <= 1e-9 and np.array_equal(w == 1.0, w_ref == 1.0)


# ---- the translation ------------------------------------------------------------------------------------------------
def test_translation(u):
    cases = [ref.translation_case(K, K) for K in ref.TRANSLATION_SIZES]
    c = cases[0][3]
    got = u.robust_translation_pairs([(ms, md) for ms, md, _, _ in cases], [R for _, _, R, _ in cases], c)
    for (ms, md, R, _), (t, sets) in zip(cases, got):
        t_ref, sets_ref = ref.tls_translation(ms, md, np.arange(len(ms)), R, c)
        assert np.abs(t - t_ref).max() <= 1e-9 and np.array_equal(sets, sets_ref)
        assert sets.sum() < sets.size or len(ms) == 3                # the planted outliers are outside
    ms, md, T, inliers = ref.planted(300, 300, 30)                   # a real rotation, an index list
    t, sets = u.robust_translation(ms, md, T[:3, :3], C_PLANTED, clique=inliers)
    t_ref, sets_ref = ref.tls_translation(ms, md, inliers, T[:3, :3], C_PLANTED)
    assert np.abs(t - t_ref).max() <= 1e-9 and np.array_equal(sets, sets_ref) and np.abs(t - T[:3, 3]).max() < 0.05


# ---- the whole fit --------------------------------------------------------------------------------------------------
def test_batch_equals_singles_with_every_status(u):
    rng = np.random.default_rng(3)
    big = rng.uniform(-20, 20, (u.ROBUST_MAX_N + 1, 3))
    pairs = [ref.planted(300, 300, 30)[:2], (big, big + 1.0), ref.planted(5, 2, 2)[:2], ref.planted(65, 65, 7)[:2]]
    batch = u.robust_fit_pairs(pairs, C_PLANTED)
    assert [f.status for f in batch] == [0, 2, 1, 0]
    assert np.array_equal(batch[1].transformation, np.identity(4)) and np.array_equal(batch[2].transformation, np.identity(4))
    assert batch[1].clique_size == 0 and batch[2].clique_size == 2 and batch[1].correspondences == u.ROBUST_MAX_N + 1
    for pair, b in zip(pairs, batch):
        one = u.robust_fit_pairs([pair], C_PLANTED)[0]
        assert one.transformation.tobytes() == b.transformation.tobytes() and one.clique.tobytes() == b.clique.tobytes()
        assert (one.status, one.clique_size, one.iterations, one.certified) == (b.status, b.clique_size, b.iterations, b.certified)
    want = ref.robust_fit(*pairs[0], C_PLANTED)
    assert batch[0].clique.tolist() == want.clique and batch[0].iterations == want.iterations
    assert np.abs(batch[0].transformation - want.transformation).max() <= 1e-9


def test_planted_thousand_is_recovered(u):
    ms, md, T, inliers = ref.planted(1000, 1000, 100)
    fit = u.robust_fit_pairs([(ms, md)], C_PLANTED)[0]
    deg, metres = ref.transform_error(fit.transformation, T)
    print("planted(1000, 100): clique %d, %.4f deg, %.4f m, %d nodes" % (fit.clique_size, deg, metres, fit.nodes))
    assert fit.status == 0 and fit.certified and deg <= 0.1 and metres <= 0.02
    by_rows = u.robust_fit_pairs([(ms, md[::-1], np.stack([np.arange(1000), 999 - np.arange(1000)], axis=1))], C_PLANTED)[0]
    assert by_rows.transformation.tobytes() == fit.transformation.tobytes()      # index rows = the matched points themselves


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def street(u):
    scenes = {s: iref.street_scene(s) for s in E2E_SEEDS}
    pairs = [(scenes[s][0], scenes[s][1]) for s in E2E_SEEDS] + [(iref.street_scene(UNRELATED[0])[0], iref.street_scene(UNRELATED[1])[1])]
    return scenes, pairs, u.solve_teaser_pairs(pairs, V, E2E_MIN_INLIERS)


def gpu_matches(u, src, dst):
    f0, f1 = u.extract_fpfh_clouds([src, dst], V)
    return u.find_correspondences(f0, f1)


def test_solve_teaser_on_the_street_scenes(u, street):
    scenes, pairs, results = street
    for s, (valid, t, R) in zip(E2E_SEEDS, results):
        src, dst, T_true, _ = scenes[s]
        coarse = ref.transform_error(valid.coarse, T_true)
        refined = ref.transform_error(iref.Rt2T(R, t), T_true)
        print("street_scene(%d): %d matches, clique %d, %d nodes, coarse %.3f deg %.3f m, refined %.4f deg %.4f m, fitness %.3f"
              % (s, valid.matches, valid.clique_size, valid.nodes, *coarse, *refined, valid.fitness))
        assert valid and valid.certified and valid.status == 0 and valid.clique_size > E2E_MIN_INLIERS
        idx0, idx1 = gpu_matches(u, src, dst)
        assert len(idx0) == valid.matches
        assert ref.is_clique(ref.consistency_graph(src[idx0], dst[idx1], V), valid.clique)
        assert coarse[0] <= E2E_COARSE_DEG and coarse[1] <= E2E_COARSE_M
        assert refined[0] <= E2E_REFINED_DEG and refined[1] <= E2E_REFINED_M


def test_clique_size_on_every_third_match_row(u, street):
    src, dst, _, _ = street[0][2]
    idx0, idx1 = gpu_matches(u, src, dst)
    ms, md = src[idx0[::3]], dst[idx1[::3]]
    assert 300 <= len(ms) <= 500
    adj = ref.consistency_graph(ms, md, V)
    size, _ = ref.max_cliques(adj)
    fit = u.robust_fit_pairs([(ms, md)], V)[0]
    assert fit.certified and fit.clique_size == size and ref.is_clique(adj, fit.clique)


def test_unrelated_scenes_are_not_valid(street):
    valid, t, R = street[2][-1]
    print("unrelated scenes: clique %d of %d matches" % (valid.clique_size, valid.matches))
    assert not valid and valid.clique_size <= E2E_MIN_INLIERS
    assert np.array_equal(iref.Rt2T(R, t), valid.coarse)             # the unrefined fit, as the reference returns it


def test_solve_teaser_pairs_equals_its_stages_bit_for_bit(u, street):
    """The chain on one upload and raw device pointers against the four public stages it is made of, each with its own
    upload and download: the same bits in every field, for the related pairs and for the unrelated one."""
    scenes, pairs, results = street
    for (src, dst), (valid, t, R) in zip(pairs, results):
        f0, f1 = u.extract_fpfh_clouds([src, dst], V)
        rows = u.find_correspondences(f0, f1)
        fit = u.robust_fit_pairs([(src, dst, rows)], V)[0]
        icp = u.registration_icp_pairs([(src, dst)], V, inits=[fit.transformation])[0]
        assert valid.coarse.tobytes() == fit.transformation.tobytes()
        assert np.array_equal(valid.clique, fit.clique) and valid.clique.dtype == fit.clique.dtype
        assert (valid.clique_size, valid.matches, valid.status, valid.certified) == (fit.clique_size, len(rows[0]), fit.status,
                                                                                      fit.certified)
        assert valid.matches == fit.correspondences
        if valid:
            assert valid.transformation.tobytes() == icp.transformation.tobytes()
            assert (valid.fitness, valid.inlier_rmse, valid.correspondences, valid.iterations) == (
                icp.fitness, icp.inlier_rmse, icp.correspondences, icp.iterations)
        else:
            assert valid.transformation.tobytes() == fit.transformation.tobytes()        # the unrefined fit
        assert np.array_equal(iref.Rt2T(R, t), valid.transformation)
    assert [bool(v) for v, _, _ in results] == [True] * len(E2E_SEEDS) + [False]


def test_compute_transform_by_teaser_needs_no_yaw(u, street):
    scenes, pairs, results = street
    src, dst = pairs[0]
    msg, ok = u.compute_transform(src, dst, V, E2E_MIN_INLIERS, coarse="teaser")
    valid, t, R = u.solve_teaser(src, dst, V, E2E_MIN_INLIERS)
    assert ok and valid and ok.clique_size == valid.clique_size == results[0][0].clique_size
    assert ok.transformation.tobytes() == valid.transformation.tobytes() == results[0][0].transformation.tobytes()
    assert (msg.translation.x, msg.translation.y, msg.translation.z) == tuple(float(v) for v in t)
    v2, t2, R2 = u.solve_icp(src, dst, V, E2E_MIN_INLIERS, init_yaw_deg=123.0, coarse="teaser")      # the yaw is not used
    assert np.array_equal(t2, t) and np.array_equal(R2, R)


def test_compute_transform_at_its_defaults_is_unchanged(u):
    src, dst, T_true, yaw = iref.street_scene(1)
    seed = iref.seed_yaw(yaw)
    msg, ok = u.compute_transform(src, dst, V, 50, init_yaw_deg=360.0 - seed)
    staged = u.register_pairs([(src, dst)], V, 360.0 - seed)[0]
    assert ok and not hasattr(ok, "clique_size")
    assert ok.transformation.tobytes() == staged.transformation.tobytes()
    assert (ok.fitness, ok.inlier_rmse, ok.correspondences, ok.iterations) == (staged.fitness, staged.inlier_rmse,
                                                                               staged.correspondences, staged.iterations)
    golden = ref.golden("compute_transform_default_street1.npy")
    assert golden is not None and ok.transformation.tobytes() == golden.tobytes()     # the parent commit's bytes


def test_fit_scratch_is_carved_afresh_for_every_batch(u):
    """One stream, so one scratch block of 23 pieces: a pair of 30 matches (most pieces shorter than 256 bytes), then three
    larger pairs with a minimal member, then the small pair again.  Both small results equal, byte for byte, the one computed
    before anything else here."""
    import torch
    small = [ref.planted(41, 30, 12)[:2]]
    large = [ref.planted(42, 300, 30)[:2], ref.planted(43, 5, 2)[:2], ref.planted(44, 257, 40)[:2]]

    def raw(pairs):
        return b"".join(f.transformation.tobytes() + f.clique.tobytes() + np.array([f.status, f.clique_size, f.iterations, f.certified,
                                                                                    f.nodes]).tobytes() for f in u.robust_fit_pairs(pairs, C_PLANTED))

    first = raw(small)
    with torch.cuda.stream(torch.cuda.Stream()):
        runs = [raw(small), raw(large), raw(small)]
    assert runs[0] == first and runs[2] == first and runs[1] == raw(large)
    assert u.robust_fit_pairs(small, C_PLANTED)[0].status == 0
