"""GPU: the maximum-clique search of csrc/robust.hip (rb_prep_kernel, rb_permute_kernel, rb_search_kernel,
rb_clique_final_kernel) against `robust_reference.clique_search`, the rule of include/cslam_hip.h restated, index for index:
where the greedy clique is too small and several maximum cliques exist (which one wins), above 4096 vertices (the second
word of a lane's bitset), widths mixed in one call (the stride of the stacks), more pairs than waves (one wave per pair),
at the depth limit and at the node budget, and through the chained fit on a pair of 4200 matches.
tests/test_robust_cpu.py checks the restatement itself and that these graphs are ones on which the rule decides something.
Every comparison: the clique as a list, ascending, `certified`, and no more nodes than the restatement, which searches
every root that the library may skip."""
import time

import numpy as np
import pytest

import robust_reference as ref
from test_robust_cpu import C_PLANTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def u():
    from cslam_amd.lidar_pr import icp_utils
    return icp_utils


def check(got, case):
    clique, certified, nodes = got
    assert clique.tolist() == case.clique and certified == case.certified
    assert np.all(np.diff(clique) > 0) and ref.is_clique(case.adj, clique)
    assert nodes <= case.nodes


def same(a, b):
    """Two results of the library, bit for bit (the nodes may differ: a root that cannot win is skipped or not)."""
    return a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def timed(label, call):
    t0 = time.perf_counter()
    out = call()
    nodes = [r[2] for r in out]
    print("%s: %d graphs, %d nodes in all, %d at most, %.3f s" % (label, len(out), sum(nodes), max(nodes), time.perf_counter() - t0))
    return out


def test_family_in_one_call_and_alone(u):
    cases = ref.family()
    batch = timed("family in one call", lambda: u.max_clique_graphs([c.words for c in cases]))
    alone = timed("family one by one", lambda: [u.max_clique(c.words, return_info=True) for c in cases])
    for case, b, a in zip(cases, batch, alone):
        check(b, case)
        check(a, case)
        assert same(a, b)


@pytest.mark.parametrize("name", ref.WIDE_ALL)
def test_wide_sets(u, name):
    case = ref.wide_case(name)
    got = timed(name, lambda: u.max_clique_graphs([case.words]))[0]
    check(got, case)
    if name != "K4097":                                              # every vertex is a root that is searched: both halves
        assert (case.core + 1 > len(case.greedy)).all() and len(case.greedy) < len(case.clique)
    if case.planted is not None:
        assert got[0].tolist() == list(ref.WIDE_PLANTED)
    if name == "K4097":
        assert got[0].tolist() == list(range(4097)) and got[1]


def test_second_words_survive_a_backtrack(u):
    """The winning root comes back to its own node, whose candidates all lie above position 4096, before it meets the winner."""
    case = ref.backtrack_search_case()
    got = timed("backtrack_case", lambda: u.max_clique_graphs([case.words]))[0]
    check(got, case)
    assert got[0].tolist() == case.planted.tolist() and len(case.greedy) == 2
    behind = u.max_clique_graphs([ref.family_case(0, 65, .5).words, case.words])[1]
    check(behind, case)
    assert same(got, behind)


def test_mixed_widths_in_one_call(u):
    """The widest graph of a call sets the words per lane and the stride of every wave's stack; narrower graphs of the same
    call use them."""
    cases = [ref.wide_case("4160/40"), ref.family_case(0, 65, .5), ref.SearchCase(np.zeros((0, 0), dtype=bool)), ref.family_case(0, 1, .5),
             ref.family_case(0, 129, .5), ref.wide_case("4097/16")]
    assert [len(c.adj) for c in cases] == [4160, 65, 0, 1, 129, 4097]
    alone = [u.max_clique(c.words, return_info=True) for c in cases]
    forward = timed("mixed widths", lambda: u.max_clique_graphs([c.words for c in cases]))
    backward = timed("mixed widths, reversed", lambda: u.max_clique_graphs([c.words for c in cases[::-1]]))[::-1]
    for case, a, f, b in zip(cases, alone, forward, backward):
        check(a, case)
        check(f, case)
        check(b, case)
        assert same(a, f) and same(a, b)


def test_many_pairs_get_one_wave_each(u):
    cases = ref.many_cases()
    got = timed("many pairs", lambda: u.max_clique_graphs([c.words for c in cases]))
    for case, g in zip(cases, got):
        check(g, case)


def test_depth_limit_is_reached_and_not_passed(u):
    """A clique of ROBUST_STACK_DEPTH members found by the search, and one of a member more: the documented uncertified exit."""
    case = ref.decoy_search_case(512, 1)
    assert len(case.greedy) == 500 and case.certified and case.clique == case.planted.tolist()
    got = timed("decoy_case(500, 512)", lambda: u.max_clique_graphs([case.words]))[0]
    check(got, case)
    assert got[1] and got[0].tolist() == case.planted.tolist() and len(got[0]) == u.ROBUST_STACK_DEPTH
    case = ref.decoy_search_case(513, 2)
    assert not case.certified and case.clique == case.planted.tolist()[1:]
    got = timed("decoy_case(500, 513)", lambda: u.max_clique_graphs([case.words]))[0]
    check(got, case)
    assert not got[1] and len(got[0]) == 512


def test_budget_of_exactly_the_restated_count(u):
    case = ref.family_case(0, 129, .5)
    assert len(case.greedy) < len(case.clique) and case.nodes > 1000
    got = u.max_clique(case.words, node_budget=case.nodes, return_info=True)
    print("129 / .5 with a budget of %d nodes: %d used" % (case.nodes, got[2]))
    check(got, case)
    assert got[1]


def test_bits_on_the_diagonal_are_not_edges(u):
    """A vertex is never its own candidate.  With every diagonal bit set every degree and every core number grows by one:
    the order, the greedy clique and every root's search stay what they are (roots of core number + 1 == the greedy size are
    searched besides and cannot beat it), so the clique is that of the graph without loops."""
    for case in (ref.family_case(0, 129, .5), ref.family_case(1, 65, .5), ref.family_case(0, 63, .5)):
        n = len(case.adj)
        clique, certified, nodes = u.max_clique(ref.to_words(case.adj | np.eye(n, dtype=bool)), return_info=True)
        print("n = %d with loops: clique %d, %d nodes (%d without)" % (n, len(clique), nodes, case.nodes))
        assert clique.tolist() == case.clique and certified and len(case.greedy) < len(case.clique)


def test_chain_on_a_wide_pair(u):
    ms, md, inliers, adj, margin = ref.wide_pair(C_PLANTED)
    t0 = time.perf_counter()
    fit = u.robust_fit_pairs([(ms, md)], C_PLANTED)[0]
    print("planted(5, 4200, 40): clique %d, %d nodes, %.3f s" % (fit.clique_size, fit.nodes, time.perf_counter() - t0))
    words, deg = u.consistency_graph(ms, md, C_PLANTED)
    assert np.array_equal(words, ref.to_words(adj)) and np.array_equal(deg, adj.sum(axis=1))
    assert fit.status == 0 and fit.certified and fit.clique.tolist() == inliers.tolist() and fit.correspondences == 4200
    want = ref.robust_fit(ms, md, C_PLANTED, clique=inliers.tolist())
    assert fit.iterations == want.iterations and np.abs(fit.transformation - want.transformation).max() <= 1e-9
    behind = u.robust_fit_pairs([ref.planted(65, 65, 7)[:2], (ms, md)], C_PLANTED)[1]
    assert behind.transformation.tobytes() == fit.transformation.tobytes() and behind.clique.tobytes() == fit.clique.tobytes()
    assert (behind.status, behind.clique_size, behind.iterations, behind.certified) == (fit.status, fit.clique_size, fit.iterations,
                                                                                        fit.certified)
