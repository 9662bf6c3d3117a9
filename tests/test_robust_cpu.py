"""CPU: what the GPU comparisons of tests/test_robust_gpu.py and tests/test_robust_clique_gpu.py rest on.  The C entry
points of csrc/robust.hip exist and check their arguments before anything touches HIP, the module has no CPU path, the
restatement of tests/robust_reference.py gives what hand-worked cases give, the inputs of the GPU tests stay away from the
decisions that rounding could turn, and the restated clique search returns the maximum clique that the header's rule names
on graphs where that rule decides something."""
import ctypes
import os

import numpy as np
import pytest

import fpfh_reference as fref
import icp_reference as iref
import robust_reference as ref
from conftest import ROOT
from cslam_amd import _lib

SYMBOLS = ("cslam_robust_graph_dev", "cslam_robust_clique_dev", "cslam_robust_rotation_dev", "cslam_robust_translation_dev",
           "cslam_robust_fit_dev")
INVALID = -1                  # CSLAM_E_INVALID
V = 0.5
C_PLANTED = 0.05              # noise bound of the planted cases: 2.5 sigma of their 2 cm noise
CLIQUE_CASES = ((64, 20), (65, 7), (300, 30))
DENSE_C = 0.5
GRAPH_SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)       # around a word and ROBUST_GRAPH_CHUNK
MARGIN = 1e-9
# The end-to-end cases: street_scene(seed) for the fits, and the source of one scene against the target of another.
E2E_SEEDS = (1, 2)
UNRELATED = (1, 3)
E2E_MIN_INLIERS = 50
E2E_COARSE_DEG, E2E_COARSE_M = 3.0, 0.25      # what the one-voxel refinement radius needs, not a measurement
# The refined result: 0.02 deg / 8 mm, the figures DESIGN records for the staged ICP; the restatement's own refined error
# on street_scene(2) is printed by test_end_to_end_restatement and is inside them.
E2E_REFINED_DEG, E2E_REFINED_M = 0.02, 0.008


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cslam_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert "int %s(" % name in header
    for lines in ("icp_utils.py:116-121", "icp_utils.py:68-83", "icp_utils.py:116-118", "icp_utils.py:75-80"):
        assert lines in header                                          # the reference lines they replace


def test_module_constants_are_the_kernels():
    from cslam_amd.lidar_pr import icp_utils as u
    kernel = open(os.path.join(ROOT, "cslam_amd", "csrc", "robust.hip")).read()
    header = open(os.path.join(ROOT, "include", "cslam_hip.h")).read()
    for name, macro in (("ROBUST_MAX_N", "ROBUST_MAX_N"), ("ROBUST_GRAPH_BLOCK", "RB_GRAPH_BLOCK"), ("ROBUST_GRAPH_CHUNK", "RB_GRAPH_CHUNK"),
                        ("ROBUST_STACK_DEPTH", "RB_STACK_DEPTH")):
        assert "#define %s %d " % (macro, getattr(u, name)) in kernel, name
    assert "#define CSLAM_ROBUST_MAX_N %d\n" % u.ROBUST_MAX_N in header
    assert "#define CSLAM_ROBUST_DEFAULT_NODE_BUDGET %d\n" % u.ROBUST_DEFAULT_NODE_BUDGET in header
    assert u.ROBUST_MAX_N >= 8192 and u.ROBUST_MAX_N == ref.MAX_N and u.ROBUST_GRAPH_CHUNK % 64 == 0
    assert "fp contract(off)" in kernel
    assert (u.ROBUST_GRAPH_CHUNK - 1, u.ROBUST_GRAPH_CHUNK, u.ROBUST_GRAPH_CHUNK + 1) == GRAPH_SIZES[-3:]


def _p(n=0x1000):
    return ctypes.c_void_p(n)          # never dereferenced: the argument checks come first


def _arr(dtype, *v):
    a = np.array(v, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    good, h_good = _arr(np.int64, 0, 5)
    cnt, h_cnt = _arr(np.int32, 5)
    graph = lambda c=0.5, n=1, h=h_good, hc=h_cnt: lib.cslam_robust_graph_dev(_p(), _p(), _p(), _p(), n, c, _p(), _p(), _p(), h, hc, None)
    clique = lambda budget=100, n=1, h=h_good, hc=h_cnt: lib.cslam_robust_clique_dev(_p(), _p(), _p(), _p(), _p(), n, budget, _p(), _p(), _p(),
                                                                                    None, h, hc, None)
    rot = lambda c=0.5, n=1, h=h_good: lib.cslam_robust_rotation_dev(_p(), _p(), _p(), _p(), _p(), n, c, _p(), _p(), _p(), h, None)
    tra = lambda c=0.5, n=1, h=h_good: lib.cslam_robust_translation_dev(_p(), _p(), _p(), _p(), _p(), _p(), n, c, _p(), None, h, None)
    fit = lambda c=0.5, budget=100, n=1, h=h_good, hc=h_cnt: lib.cslam_robust_fit_dev(_p(), _p(), _p(), _p(), _p(), _p(), _p(), n, c, budget,
                                                                                     _p(), _p(), None, h, hc, None)
    for c in (0.0, -1.0, float("inf"), float("nan")):
        assert graph(c) == INVALID and rot(c) == INVALID and tra(c) == INVALID and fit(c) == INVALID
    assert b"noise_bound" in lib.cslam_last_error()
    for budget in (0, -5):
        assert clique(budget) == INVALID and fit(0.5, budget) == INVALID
    assert b"node_budget" in lib.cslam_last_error()
    for n in (0, 65536):
        assert graph(n=n) == INVALID and clique(n=n) == INVALID and rot(n=n) == INVALID and tra(n=n) == INVALID and fit(n=n) == INVALID
    for bad in ((1, 5), (0, -1), (3, 2)):
        keep, h_bad = _arr(np.int64, *bad)
        assert graph(h=h_bad) == INVALID and clique(h=h_bad) == INVALID and rot(h=h_bad) == INVALID and tra(h=h_bad) == INVALID
        assert fit(h=h_bad) == INVALID
    for bad in (-1, 6):
        keep, h_bad = _arr(np.int32, bad)
        assert graph(hc=h_bad) == INVALID and clique(hc=h_bad) == INVALID and fit(hc=h_bad) == INVALID
    assert b"count" in lib.cslam_last_error()
    assert lib.cslam_robust_graph_dev(None, _p(), _p(), _p(), 1, 0.5, _p(), _p(), _p(), h_good, h_cnt, None) == INVALID
    assert lib.cslam_robust_fit_dev(_p(), _p(), _p(), _p(), _p(), _p(), _p(), 1, 0.5, 100, None, _p(), None, h_good, h_cnt, None) == INVALID


def _no_gpu():
    n = ctypes.c_int(0)
    return _lib.load().cslam_device_count(ctypes.byref(n)) != 0 or n.value == 0


def test_python_argument_errors_come_first():
    from cslam_amd.lidar_pr import icp_utils as u
    pts = np.zeros((4, 3))
    for call in (lambda: u.consistency_graph(pts, pts, 0.0), lambda: u.robust_rotation(pts, pts, float("nan")),
                 lambda: u.robust_translation(pts, pts, np.identity(3), -1.0), lambda: u.robust_fit_pairs([(pts, pts)], float("inf")),
                 lambda: u.max_clique(np.zeros((1, 1), np.uint64), node_budget=0), lambda: u.solve_teaser(pts, pts, 0.0, 5)):
        with pytest.raises(_lib.CslamHipError, match="invalid argument"):
            call()
    with pytest.raises(ValueError):
        u.consistency_graph(pts, pts[:3], 0.5)
    with pytest.raises(ValueError):
        u.max_clique(np.zeros((3, 2), np.uint64))
    with pytest.raises(ValueError):
        u.compute_transform(pts, pts, 0.5, 5, coarse="svd")


@pytest.mark.skipif(not _no_gpu(), reason="GPU present: covered by the -m gpu suite")
def test_robust_fit_fails_loudly_without_gpu():
    from cslam_amd.lidar_pr import icp_utils as u
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((50, 3)), rng.standard_normal((50, 3))
    words = np.zeros((50, 1), dtype=np.uint64)
    calls = (lambda: u.consistency_graph(a, b, 0.5), lambda: u.consistency_graph_pairs([(a, b)], 0.5), lambda: u.max_clique(words),
             lambda: u.max_clique_graphs([words]), lambda: u.robust_rotation(a, b, 0.5), lambda: u.robust_rotation_pairs([(a, b)], 0.5),
             lambda: u.robust_translation(a, b, np.identity(3), 0.5), lambda: u.robust_translation_pairs([(a, b)], [np.identity(3)], 0.5),
             lambda: u.robust_fit_pairs([(a, b)], 0.5), lambda: u.solve_teaser_pairs([(a, b)], 0.5, 5), lambda: u.solve_teaser(a, b, 0.5, 5),
             lambda: u.compute_transform(a, b, 0.5, 5, coarse="teaser"), lambda: u.solve_icp(a, b, 0.5, 5, coarse="teaser"))
    for call in calls:
        with pytest.raises(_lib.CslamHipError):
            call()


def test_restatement_on_cases_worked_by_hand():
    # the lattice: odd matches agree exactly, (2, 3) is at the bound itself, (2, 1) beyond it
    ms, md = ref.lattice_case(8)
    adj = ref.consistency_graph(ms, md, 1.0)
    assert adj[1, 3] and adj[3, 5] and adj[2, 3] and adj[3, 2] and not adj[2, 1] and not adj[2, 4] and not adj.diagonal().any()
    assert adj[0].tolist() == [False, True, False, True, False, True, False, True]    # match 0 sits at both origins
    words = ref.to_words(adj)
    assert words.shape == (8, 1) and int(words[0, 0]) == 0b10101010 and np.array_equal(ref.from_words(words, 8), adj)
    # a triangle with a tail: clique {0, 1, 2}; core numbers 2, 2, 2, 1; the greedy clique is the triangle
    g = np.zeros((4, 4), dtype=bool)
    for i, j in ((0, 1), (0, 2), (1, 2), (2, 3)):
        g[i, j] = g[j, i] = True
    assert ref.max_clique(g) == ([0, 1, 2], True) and ref.core_numbers(g).tolist() == [2, 2, 2, 1] and ref.greedy_clique(g) == [0, 1, 2]
    assert ref.is_clique(g, [0, 1, 2]) and not ref.is_clique(g, [1, 2, 3])
    assert ref.max_cliques(np.zeros((3, 3), dtype=bool)) == (1, [[0], [1], [2]])
    # rotation by 90 degrees about z, exact: every residual is 0, mu < 0, the loop stops at once with unit weights
    ms = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 2, 0], [0.0, 2, 3]])
    Rz = np.array([[0.0, -1, 0], [1.0, 0, 0], [0.0, 0, 1]])
    md = ms @ Rz.T + np.array([5.0, -1.0, 2.0])
    R, w, it = ref.gnc_rotation(ms, md, [0, 1, 2, 3], 0.1)
    assert it == 0 and w.tolist() == [1.0, 1.0, 1.0] and np.abs(R - Rz).max() < 1e-15
    # scalars 0, 0.1, 0.2 and an outlier at 5 with c = 0.5: the three agree, the estimate is their mean
    est, inset = ref.scalar_tls(np.array([0.0, 5.0, 0.1, 0.2]), 0.5)
    assert inset.tolist() == [True, False, True, True] and abs(est - 0.1) < 1e-15
    t, sets = ref.tls_translation(ms, md, [0, 1, 2, 3], Rz, 0.1)
    assert np.abs(t - [5.0, -1.0, 2.0]).max() < 1e-14 and sets.all()
    fit = ref.robust_fit(ms, md, 0.1)
    assert fit.status == 0 and fit.clique == [0, 1, 2, 3] and np.abs(fit.transformation - iref.Rt2T(Rz, [5.0, -1.0, 2.0])).max() < 1e-14
    assert ref.robust_fit(ms[:2], md[:2], 0.1).status == 1


def test_clique_search_agrees_with_networkx():
    nx = pytest.importorskip("networkx")
    for n, n_in in CLIQUE_CASES:
        ms, md, _, _ = ref.planted(n, n, n_in)
        adj = ref.consistency_graph(ms, md, C_PLANTED)
        best = max(nx.find_cliques(nx.from_numpy_array(adj)), key=len)
        assert sorted(best) == ref.max_clique(adj)[0]
    rng = np.random.default_rng(1)
    adj = np.triu(rng.random((60, 60)) < 0.5, 1)
    adj = adj | adj.T
    sizes = [len(c) for c in nx.find_cliques(nx.from_numpy_array(adj))]
    size, cliques = ref.max_cliques(adj)
    assert size == max(sizes) and len(cliques) == sizes.count(size)


def lowest_position(case, clique):
    """The lowest position in the order of the search among the members of a clique: its root."""
    position = np.empty(len(case.adj), dtype=np.int64)
    position[ref.search_order(case.adj, case.core)] = np.arange(len(case.adj))
    return int(position[np.asarray(clique, dtype=np.int64)].min())


def check_winner(case, nx=None):
    """What the header's rule promises of `clique_search`: a maximum clique; the greedy one when that is one; otherwise one
    whose root no other maximum clique undercuts.  Returns (maximum size, number of maximum cliques)."""
    size, cliques = ref.max_cliques(case.adj)
    assert case.certified and case.clique in cliques
    if size == len(case.greedy):
        assert case.clique == case.greedy
    else:
        assert lowest_position(case, case.clique) == min(lowest_position(case, c) for c in cliques)
    if nx is not None and len(case.adj):
        assert size == nx.max_weight_clique(nx.from_numpy_array(case.adj), weight=None)[1]     # its own branch and bound
    return size, len(cliques)


def test_restated_search_on_cases_worked_by_hand():
    # two triangles {0, 1, 2} and {3, 4, 5} joined by the edge 2 - 3, and the pendant 6 on vertex 0: core numbers 2 but for
    # the pendant's 1; the greedy clique is the first triangle, nothing beats it, and every root is one node
    g = np.zeros((7, 7), dtype=bool)
    for i, j in ((0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3), (0, 6)):
        g[i, j] = g[j, i] = True
    assert ref.core_numbers(g).tolist() == [2, 2, 2, 2, 2, 2, 1] and ref.search_order(g).tolist() == [6, 0, 1, 2, 3, 4, 5]
    assert ref.clique_search(g) == ([0, 1, 2], True, 0)                # core + 1 = 3 <= g = 3: no root is searched
    # the 5-cycle 0-1-2-3-4 with the chords 1 - 3 and 2 - 4: core numbers 2, the order is the indices, the greedy clique
    # {0, 1} starts at the lowest index and misses both triangles.  Roots 4, 3 and 0 are one node each; root 2 meets
    # {2, 4, 3} and root 1 meets {1, 3, 2} in three nodes each: equal sizes, the lower root wins
    g = np.zeros((5, 5), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (1, 3), (2, 4)):
        g[i, j] = g[j, i] = True
    assert ref.core_numbers(g).tolist() == [2] * 5 and ref.greedy_clique(g) == [0, 1]
    assert ref.max_cliques(g) == (3, [[1, 2, 3], [2, 3, 4]]) and ref.clique_search(g) == ([1, 2, 3], True, 9)
    # the colouring: a path 0 - 1 - 2 has the classes {0, 2} and {1}; only vertex 1 has a colour above 1
    nb = ref._rows_as_ints(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=bool))
    assert ref._colour(nb, 0b111, 1) == 0b010 and ref._colour(nb, 0b111, 0) == 0b111 and ref._colour(nb, 0b111, 2) == 0
    assert ref._colour(nb, 0b101, 1) == 0 and ref._colour(nb, 0b011, 1) == 0b010
    # the depth: a clique of 5 beside three decoy pairs, in which the greedy clique starts, needs 4 levels below its root
    adj, planted = ref.decoy_case(3, 5)
    assert len(ref.greedy_clique(adj)) == 3 and planted.tolist() == [6, 7, 8, 9, 10]
    assert ref.clique_search(adj, stack_depth=5)[:2] == ([6, 7, 8, 9, 10], True)
    assert ref.clique_search(adj, stack_depth=4)[:2] == ([7, 8, 9, 10], False)       # root 7 found its 4 before root 6 gave up
    adj2, planted2 = ref.decoy_case(3, 5, seed=1)
    assert not np.array_equal(adj, adj2) and ref.clique_search(adj2)[0] == planted2.tolist() and ref.is_clique(adj2, planted2)
    assert ref.gnp_case(3, 50, .5).diagonal().sum() == 0 and np.array_equal(ref.gnp_case(3, 50, .5), ref.gnp_case(3, 50, .5).T)
    assert ref.clique_search(np.zeros((0, 0), dtype=bool)) == ([], True, 0)


def test_restated_search_on_the_random_family():
    """On every graph of the family the restated search returns the maximum clique that the header's rule names, and the
    family is one on which that rule decides something: the greedy clique is too small on two thirds of the graphs, more
    than one maximum clique exists on half, and no search comes near the node budget."""
    try:
        import networkx as nx
    except ImportError:
        nx = None
    from cslam_amd.lidar_pr import icp_utils as u
    cases = ref.family()
    assert len(cases) == 26
    smaller = several = 0
    for case in cases:
        size, count = check_winner(case, nx)
        smaller += len(case.greedy) < size
        several += count > 1
    nodes = max(case.nodes for case in cases)
    print("family: greedy smaller on %d of %d, several maximum cliques on %d, at most %d nodes, largest clique %d"
          % (smaller, len(cases), several, nodes, max(len(case.clique) for case in cases)))
    assert 3 * smaller >= 2 * len(cases) and 2 * several >= len(cases)
    assert nodes < u.ROBUST_DEFAULT_NODE_BUDGET // 16


def test_restated_search_at_the_depth_limit():
    """A clique of 512 beside 500 decoy pairs is found 511 levels below its root, which is as deep as a search may go; one
    of 513 would need another level: the search ends uncertified with what the roots above had recorded."""
    from cslam_amd.lidar_pr import icp_utils as u
    assert u.ROBUST_STACK_DEPTH == 512
    case = ref.decoy_search_case(512)
    print("decoy_case(500, 512): greedy %d, clique %d, %d nodes" % (len(case.greedy), len(case.clique), case.nodes))
    assert len(case.greedy) == 500 and case.certified and case.clique == case.planted.tolist() and case.nodes < 10 ** 5
    case = ref.decoy_search_case(513)
    assert len(case.greedy) == 500 and not case.certified and len(case.clique) >= 500 and ref.is_clique(case.adj, case.clique)
    assert case.clique == case.planted.tolist()[1:]                  # the root above the lowest one found its 512
    for seed, k in ((1, 512), (2, 513)):                             # relabelled, as the GPU tests run them
        adj, planted = ref.decoy_case(500, k, seed)
        assert len(ref.greedy_clique(adj)) == 500 and ref.is_clique(adj, planted) and len(planted) == k


@pytest.mark.parametrize("name", ref.WIDE_ALL)
def test_restated_search_on_the_wide_graphs(name):
    """More than 4096 vertices: a lane of the search holds two words of every set.  The winner is a maximum clique by the
    header's rule, every vertex is a root that is searched, and roots lie in both halves."""
    case = ref.wide_case(name)
    n = len(case.adj)
    if name == "K4097":                                              # listing its one clique would recurse 4097 deep
        assert case.clique == list(range(n)) and case.certified and case.nodes == 0 and case.greedy == case.clique
        return
    size, count = check_winner(case)
    print("%s: greedy %d, maximum %d (%d of them), %d nodes, core numbers %d .. %d" % (name, len(case.greedy), size, count, case.nodes,
                                                                                         case.core.min(), case.core.max()))
    assert n >= 4096 and (case.core + 1 > len(case.greedy)).all()    # every vertex is a root, in both halves of the order
    assert case.nodes >= n
    if case.planted is not None:
        assert count == 1 and case.clique == case.planted.tolist() and len(case.greedy) < size
        position = np.argsort(ref.search_order(case.adj, case.core))[case.planted]
        assert position.min() < 4096 <= position.max()               # the clique itself spans both halves
    else:
        assert len(case.greedy) < size and count > 1


def test_restated_search_comes_back_to_a_node_in_the_second_words():
    """`backtrack_case`: the winner is met after the root's first branch has ended elsewhere, so a search that loses the
    candidates of a node it comes back to, above position 4096, returns another clique."""
    case = ref.backtrack_search_case()
    adj, first, second = ref.backtrack_case()
    n, s = len(adj), len(adj) - 46
    assert s == 4096 and case.core[:s].max() == 0 and (case.core[s:] == 11).all()
    assert ref.search_order(adj, case.core).tolist() == list(range(n))              # positions are indices
    assert ref.max_cliques(adj[s:, s:]) == (12, sorted([[v - s for v in first], [v - s for v in second]]))
    assert len(case.greedy) == 2 and case.certified and case.clique == first and min(first) < min(second)
    nb = ref._rows_as_ints(adj)
    root = first[0]
    B = ref._colour(nb, (nb[root] >> (root + 1)) << (root + 1), len(case.greedy) - 1)
    assert (B & -B).bit_length() - 1 not in first                    # the first branch of the winning root leaves the winner


def test_input_conditions_of_the_wide_pair():
    ms, md, inliers, adj, margin = ref.wide_pair(C_PLANTED)
    clique, unique = ref.max_clique(adj)
    print("planted(5, 4200, 40): graph margin %.2e, mean degree %.1f, greedy %d" % (margin, adj.sum(axis=1).mean(), len(ref.greedy_clique(adj))))
    assert margin >= MARGIN and unique and clique == inliers.tolist() and len(ms) > 4096
    assert ref.clique_search(adj)[:2] == (clique, True)


def test_many_small_graphs_cover_every_size():
    cases = ref.many_cases()
    sizes = {len(case.adj) for case in cases}
    assert len(cases) == ref.MANY > 512 and sizes == set(range(41))
    assert all(case.certified and ref.is_clique(case.adj, case.clique) for case in cases)
    assert sum(len(case.greedy) < len(case.clique) for case in cases) >= 50


def test_input_conditions_of_the_graph_and_clique_comparisons():
    """Bit-level agreement of the graphs means something only where no |b - a| sits on the bound, and index-level agreement
    of the cliques only where the maximum clique is the only one."""
    worst = np.inf
    for n in GRAPH_SIZES:
        ms, md, _, _ = ref.planted(n, n, max(n // 3, 1))
        worst = min(worst, ref.consistency_graph(ms, md, C_PLANTED, return_margin=True)[1])
    for n, n_in in CLIQUE_CASES + ((1000, 100),):
        ms, md, _, inliers = ref.planted(n, n, n_in)
        adj, margin = ref.consistency_graph(ms, md, C_PLANTED, return_margin=True)
        worst = min(worst, margin)
        clique, unique = ref.max_clique(adj)
        assert unique, (n, n_in)
        if n <= 300:
            assert clique == inliers.tolist(), (n, n_in)
        else:                                                        # among 4950 inlier pairs one or two have more noise than 2 c
            assert set(clique) <= set(inliers.tolist()) and len(clique) >= n_in - 5
    ms, md, first, second = ref.two_planted(4, 200, 25)
    adj, margin = ref.consistency_graph(ms, md, C_PLANTED, return_margin=True)
    size, cliques = ref.max_cliques(adj)
    assert size == 25 and cliques == sorted([first.tolist(), second.tolist()])
    ms, md = ref.dense_case()
    adj, dense_margin = ref.consistency_graph(ms, md, DENSE_C, return_margin=True)
    print("graph margins: planted %.2e, two cliques %.2e, dense %.2e (edge share %.2f)" % (worst, margin, dense_margin, adj.mean()))
    assert min(worst, margin, dense_margin) >= MARGIN
    assert 0.3 < adj.mean() < 0.9 and len(ref.greedy_clique(adj)) >= 3


def test_input_conditions_of_the_rotation_comparisons():
    """Every r2 stays away from th1 and th2 in every iteration, every cost difference but the last is far from the
    threshold, and the last one is exactly 0: the iteration count and the weight sets do not hang on the last bits."""
    for m, share, seed in ref.ROTATION_CASES:
        ms, md, c = ref.rotation_case(m, share, seed)
        R, w, it, trace = ref.gnc_rotation(ms, md, np.arange(m + 1), c, return_trace=True)
        costs = trace["costs"]
        print("m = %d, outliers %.0f %%: %d iterations, band margin %.2e, smallest non-final cost difference %.2e, final %.1e"
              % (m, 100 * share, it, trace["band"], min(costs[:-1]) if len(costs) > 1 else np.inf, costs[-1] if costs else 0.0))
        if share == 0.0:
            assert it == 0 and np.array_equal(w, np.ones(m))
            continue
        assert 2 <= it < ref.GNC_MAX_ITER and trace["band"] >= MARGIN
        assert min(costs[:-1]) >= MARGIN and costs[-1] == 0.0
        assert (w == 0.0).sum() >= int(0.5 * share * m) and ((w == 0.0) | (w == 1.0)).all()


def test_input_conditions_of_the_sublist_and_small_pair_comparisons():
    """The GPU tests also compare, against the restatement, the rotation and the translation on the inlier list of
    planted(300, 300, 30), and the clique size of planted(5, 2, 2)."""
    ms, md, T, inliers = ref.planted(300, 300, 30)
    R, w, it, trace = ref.gnc_rotation(ms, md, inliers, C_PLANTED, return_trace=True)
    costs = trace["costs"]
    print("inlier list of planted(300, 300, 30): %d iterations, band margin %.2e, cost differences %s" % (it, trace["band"], costs))
    if it:
        assert trace["band"] >= MARGIN and all(d >= MARGIN for d in costs[:-1]) and (costs[-1] == 0.0 or it == ref.GNC_MAX_ITER)
    else:                                                            # stopped at mu <= 0: the largest r2 is well below nb2 / 2
        a, b = ref.chain(ms, md, inliers)
        r2 = ((b - a @ R.T) ** 2).sum(axis=1)
        assert abs(2.0 * r2.max() / (4.0 * C_PLANTED ** 2) - 1.0) >= 1e-3
    xs = ref.translation_scalars(ms, md, inliers, T[:3, :3])
    margins = [ref.scalar_tls(xs[a], C_PLANTED, return_margin=True)[2] for a in range(3)]
    print("translation on the same list under the true rotation: margins %s" % margins)
    assert min(margins) >= MARGIN
    ms, md, _, _ = ref.planted(5, 2, 2)
    adj, margin = ref.consistency_graph(ms, md, C_PLANTED, return_margin=True)
    assert margin >= MARGIN and ref.max_cliques(adj)[0] == 2
    ms, md, _, _ = ref.planted(65, 65, 7)
    assert ref.consistency_graph(ms, md, C_PLANTED, return_margin=True)[1] >= MARGIN


def test_translation_cases_have_outliers_and_duplicates():
    for K in ref.TRANSLATION_SIZES:
        ms, md, R, c = ref.translation_case(K, K)
        t, sets = ref.tls_translation(ms, md, np.arange(K), R, c)
        assert np.abs(t - [1.5, -2.25, 0.5]).max() < 0.03
        assert (np.abs(sets.sum(axis=1) - (K - K // 5)) <= 2).all()          # a duplicate may copy an outlier, or replace one
        if K >= 6:
            assert np.array_equal(md[K // 2], md[0]) and sets[:, K // 2].tolist() == sets[:, 0].tolist()


@pytest.fixture(scope="module")
def scene2():
    src, dst, T_true, _ = iref.street_scene(2)
    idx0, idx1 = fref.find_correspondences(fref.extract_fpfh(src, V), fref.extract_fpfh(dst, V))
    return src, dst, T_true, idx0, idx1


def test_end_to_end_restatement(scene2):
    """street_scene(2) through the restated chain: FPFH, mutual matches, the robust fit, one ICP stage."""
    src, dst, T_true, idx0, idx1 = scene2
    fit = ref.robust_fit(src[idx0], dst[idx1], V)
    deg, metres = ref.transform_error(fit.transformation, T_true)
    true = int((np.linalg.norm(iref.apply_T(T_true, src[idx0]) - dst[idx1], axis=1) < 0.5).sum())
    print("street_scene(2): %d / %d points, %d mutual matches, %d true, clique %d, coarse fit %.3f deg %.3f m"
          % (len(src), len(dst), len(idx0), true, fit.clique_size, deg, metres))
    assert fit.status == 0 and fit.clique_size > E2E_MIN_INLIERS
    assert deg <= E2E_COARSE_DEG and metres <= E2E_COARSE_M
    refined = iref.registration_icp(src, dst, V, fit.transformation, 100)
    rdeg, rmetres = ref.transform_error(refined.transformation, T_true)
    print("refined: %.4f deg %.4f m, fitness %.3f, %d iterations" % (rdeg, rmetres, refined.fitness, refined.iterations))
    assert rdeg <= E2E_REFINED_DEG and rmetres <= E2E_REFINED_M


def test_unrelated_scenes_have_no_large_clique():
    src = iref.street_scene(UNRELATED[0])[0]
    dst = iref.street_scene(UNRELATED[1])[1]
    idx0, idx1 = fref.find_correspondences(fref.extract_fpfh(src, V), fref.extract_fpfh(dst, V))
    fit = ref.robust_fit(src[idx0], dst[idx1], V)
    print("street_scene(%d) source, street_scene(%d) target: %d mutual matches, clique %d" % (*UNRELATED, len(idx0), fit.clique_size))
    assert fit.clique_size <= E2E_MIN_INLIERS
