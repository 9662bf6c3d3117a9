"""GPU: the pose-graph back end (csrc/pgo.hip) kernel by kernel and end to end against tests/pgo_reference.py.

Every bound is stated where it is used; the figures measured on one MI355X are recorded beside them and in DESIGN.md.
"""
import numpy as np
import pytest
from scipy.sparse.linalg import spsolve

import pgo_reference as ref
from cslam_amd import _lib
from cslam_amd.back_end import pose_graph as pg

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SEG_MAX = 64


def problem(n, ei, ej, meas, sig, prior, poses, known=None):
    values = {(0, v): poses[v] for v in range(n)}
    edges = [((0, int(i)), (0, int(j)), meas[k], sig[k]) for k, (i, j) in enumerate(zip(ei, ej))]
    return pg.Problem(values, edges, ((0, prior), meas[len(ei)], sig[len(ei)]), known)


def scene_problem(sc, known=True):
    gr = sc.graph
    return problem(gr.n, gr.ei, gr.ej, gr.meas, gr.sig, gr.prior, sc.init, sc.known if known else None)


def scene_args(sc, known=True):
    gr = sc.graph
    values = {(0, v): sc.init[v] for v in range(gr.n)}
    edges = [((0, int(gr.ei[k])), (0, int(gr.ej[k])), gr.meas[k], gr.sig[k]) for k in range(gr.nf)]
    return values, edges, ((0, gr.prior), gr.meas[gr.nf], gr.sig[gr.nf]), (sc.known if known else None)


# ---- linearise -------------------------------------------------------------------------------------------------------------------------
# |got - want| <= LIN_ULPS eps max|block| per block (E: per factor, against E itself).  Measured on an MI355X: 4.7 eps at the
# worst entry of these graphs; the bound is 64, about 14 x that figure.
LIN_ULPS = 64.0


def linearize_graph():
    """70 poses: pose 0 has 1 factor, pose 1 two; (2, 1) has i > j; (3, 4) is met by three parallel factors, one reversed;
    pose 5 carries 64 edges and the prior = 65 factors.  Factor 0 has residual angle exactly 0 (identity rotations, a
    translation residual), factor 1 residual angle pi - 1e-6."""
    rng = np.random.default_rng(21)
    n = 70
    poses = np.stack([ref.exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-5, 5, 3)])) for _ in range(n)])
    for v, t in ((0, [1.0, 2.0, -0.5]), (1, [2.5, 1.0, 0.25])):
        poses[v] = np.identity(4)
        poses[v][:3, 3] = t
    ed = [(0, 1), (2, 1), (3, 4), (4, 3), (3, 4)] + [(5, v) if v % 2 else (v, 5) for v in range(6, 70)]
    ei, ej = np.array([e[0] for e in ed], dtype=np.int32), np.array([e[1] for e in ed], dtype=np.int32)
    meas = [ref.inv(poses[i]) @ poses[j] @ ref.exp(rng.standard_normal(6) * 0.3) for i, j in ed]
    meas[0] = ref.inv(poses[0]) @ poses[1]
    meas[0][:3, 3] += [0.25, -0.125, 0.5]
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    meas[1] = ref.inv(poses[2]) @ poses[1] @ ref.inv(ref.exp(np.concatenate([(np.pi - 1e-6) * axis, [0.3, 0.2, -0.1]])))
    meas.append(poses[5] @ ref.exp(rng.standard_normal(6) * 0.1))
    sig = np.tile(ref.SIGMAS, (len(ed) + 1, 1)) * rng.uniform(0.5, 2.0, (len(ed) + 1, 6))
    return n, ei, ej, np.stack(meas), sig, 5, poses


def compare_system(st, gr, poses, w, figures):
    E = st.linearize(st.dev(poses), st.dev(w)).cpu().numpy().copy()
    Hd, g, Ho, pa, pb = st.system()
    rE, rHd, rg, rHo = ref.linearize(gr, poses, w)
    assert list(zip(pa.tolist(), pb.tolist())) == gr.pairs()
    worst = 0.0
    for k in range(gr.nf + 1):
        worst = max(worst, abs(E[k] - rE[k]) / (EPS * max(rE[k], np.finfo(np.float64).tiny)))
    for v in range(gr.n):
        scale = np.abs(rHd[v]).max()
        worst = max(worst, np.abs(Hd[v] - rHd[v]).max() / (EPS * scale))
        # the gradient A^T (e / sigma^2) of a pose inherits the rounding of its factors' residuals through the same A^T A / sigma^2
        # that makes the diagonal block: its error is scaled by the larger of the two
        worst = max(worst, np.abs(g[v] - rg[v]).max() / (EPS * max(np.abs(rg[v]).max(), scale)))
    for q, key in enumerate(gr.pairs()):
        worst = max(worst, np.abs(Ho[q] - rHo[key]).max() / (EPS * np.abs(rHo[key]).max()))
    figures.append(worst)
    return E, Hd, g, Ho


def test_linearize_matches_the_restatement_and_repeats_bit_for_bit():
    n, ei, ej, meas, sig, prior, poses = linearize_graph()
    gr = ref.Graph(n, ei, ej, meas, sig, prior)
    st = pg.Staged(problem(n, ei, ej, meas, sig, prior, poses))
    figures = []
    w = np.random.default_rng(3).uniform(0.0, 1.0, gr.nf + 1)
    w[:5] = 1.0
    first = compare_system(st, gr, poses, w, figures)
    again = compare_system(st, gr, poses, w, figures)
    for a, b in zip(first, again):
        assert np.array_equal(a, b), "two runs must agree bit for bit"
    e1 = ref.between(poses[2], poses[1], meas[1], jac=False)[0]
    assert abs(np.linalg.norm(e1[:3]) - (np.pi - 1e-6)) < 1e-9 and np.all(ref.between(poses[0], poses[1], meas[0], jac=False)[0][:3] == 0.0)
    # one edge, two poses
    st1 = pg.Staged(problem(2, ei[:1], ej[:1], meas[[0, -1]], sig[[0, -1]], 1, poses[:2]))
    compare_system(st1, ref.Graph(2, ei[:1], ej[:1], meas[[0, -1]], sig[[0, -1]], 1), poses[:2], np.ones(2), figures)
    print("linearise: worst error %.1f eps of the block's magnitude" % max(figures))
    assert max(figures) <= LIN_ULPS, figures


# ---- solve -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.plan_graphs(SEG_MAX)))
def test_solve_against_spsolve(name):
    """|| (H + lam I) d + g || / || g || <= 10 x the same figure of spsolve's solution of the same system (the system the GPU
    linearised, read back), and || d - d_spsolve || <= || A^-1 || (|| res || + || res_spsolve ||): the two solutions of A x = b
    differ by A^-1 applied to the difference of their residuals; || A^-1 ||_2 = 1 / lambda_min(A) from a dense eigh."""
    n, ei, ej, prior = ref.plan_graphs(SEG_MAX)[name]
    poses, meas, sig = ref.random_graph_values(n, ei, ej, 3)
    st = pg.Staged(problem(n, ei, ej, meas, sig, prior, poses))
    assert st.info["longest"] <= SEG_MAX and st.info["seg_max"] == SEG_MAX
    st.linearize(st.dev(poses), st.dev(np.ones(len(ei) + 1)))
    Hd, g, Ho, pa, pb = st.system()
    Hoff = {(int(a), int(b)): Ho[q] for q, (a, b) in enumerate(zip(pa, pb))}
    lams = [1e-5, 1e5] + ([] if name == "two-components" else [0.0])      # one component has no prior: singular at 0
    for lam in lams:
        A = ref.assemble(n, Hd, Hoff, lam)
        b = -g.ravel()
        want = spsolve(A, b)
        delta, status, predicted = st.solve(lam)
        got = delta.cpu().numpy().ravel().copy()
        assert status == 0
        res = lambda x: np.linalg.norm(A @ x - b)
        print("%s lam %g: residual %.3g (spsolve %.3g)" % (name, lam, res(got) / np.linalg.norm(b), res(want) / np.linalg.norm(b)))
        assert res(got) <= 10.0 * res(want), (name, lam, res(got), res(want))
        inv_norm = 1.0 / np.linalg.eigvalsh(A.toarray())[0]
        assert np.linalg.norm(got - want) <= inv_norm * (res(got) + res(want)), (name, lam)
        H = ref.assemble(n, Hd, Hoff, 0.0)
        model = -(float(g.ravel() @ got) + 0.5 * float(got @ (H @ got)))
        assert abs(predicted - model) <= 1e-12 * (abs(float(g.ravel() @ got)) + abs(float(got @ (H @ got))))
        delta2, _, predicted2 = st.solve(lam)
        assert np.array_equal(delta2.cpu().numpy().ravel(), got) and predicted2 == predicted, "two runs must agree bit for bit"


def test_non_positive_pivot_is_a_status():
    """Weights of zero on every factor: H = 0, and at lambda = 0 the first pivot is not positive.  Nothing aborts."""
    n, ei, ej, prior = ref.plan_graphs(SEG_MAX)["adjacent-junctions"]
    poses, meas, sig = ref.random_graph_values(n, ei, ej, 3)
    st = pg.Staged(problem(n, ei, ej, meas, sig, prior, poses))
    st.linearize(st.dev(poses), st.dev(np.zeros(len(ei) + 1)))
    assert st.solve(0.0)[1] == 1
    assert st.solve(1.0)[1] == 0


# ---- retract, cost, weights ------------------------------------------------------------------------------------------------------------
# of max(1, |t|): the product of two transforms, three terms per entry, and the rounding of sin / cos.  Measured 0.8 eps; 16 is 20 x.
RETRACT_ULPS = 16.0


def test_retract_matches_the_restatement():
    rng = np.random.default_rng(8)
    n = 300
    poses = np.stack([ref.exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-50, 50, 3)])) for _ in range(n)])
    delta = rng.standard_normal((n, 6)) * np.array([0.3, 0.3, 0.3, 2, 2, 2])
    delta[:5] *= 1e-4                                           # the series branch
    delta[5] = 0.0
    st = pg.Staged(problem(2, [0], [1], np.stack([np.identity(4)] * 2), np.tile(ref.SIGMAS, (2, 1)), 0, poses[:2]))
    out = st.retract(st.dev(poses), st.dev(delta)).cpu().numpy()
    want = ref.retract(poses, delta)
    assert np.array_equal(out[5], poses[5])
    worst = max(np.abs(out[v] - want[v]).max() / (EPS * max(1.0, np.abs(want[v][:3, 3]).max())) for v in range(n))
    print("retract: worst error %.1f eps" % worst)
    assert worst <= RETRACT_ULPS


def tree_sum(x):
    """pgo_cost_kernel: blocks of 256, halving tree inside a block, the block partials in block order."""
    total = 0.0
    for b in range(0, len(x), 256):
        sh = np.zeros(256)
        sh[:len(x[b:b + 256])] = x[b:b + 256]
        off = 128
        while off >= 1:
            sh[:off] = sh[:off] + sh[off:2 * off]
            off //= 2
        total = total + sh[0]
    return total


def test_cost_is_the_ordered_sum_of_the_weighted_errors():
    n, ei, ej, meas, sig, prior, poses = linearize_graph()
    gr = ref.Graph(n, ei, ej, meas, sig, prior)
    # 600 more factors: three blocks of partial sums
    rng = np.random.default_rng(2)
    extra = [(int(a), int(b)) for a, b in rng.integers(0, n, (700, 2)) if a != b][:600]
    ei2, ej2 = np.concatenate([ei, [e[0] for e in extra]]).astype(np.int32), np.concatenate([ej, [e[1] for e in extra]]).astype(np.int32)
    meas2 = np.concatenate([meas[:-1], np.stack([ref.inv(poses[a]) @ poses[b] @ ref.exp(rng.standard_normal(6) * 0.2) for a, b in extra]), meas[-1:]])
    sig2 = np.tile(ref.SIGMAS, (len(ei2) + 1, 1))
    gr = ref.Graph(n, ei2, ej2, meas2, sig2, prior)
    st = pg.Staged(problem(n, ei2, ej2, meas2, sig2, prior, poses))
    w = rng.uniform(0.0, 1.0, gr.nf + 1)
    cost = st.cost(st.dev(poses), st.dev(w))
    E = st.E.cpu().numpy()
    assert cost == tree_sum(w * E), "exact: the same products in the same order"
    rE = ref.errors(gr, poses)
    assert np.abs(E - rE).max() <= LIN_ULPS * EPS * rE.max()
    assert abs(cost - float(w @ rE)) <= LIN_ULPS * EPS * float(w @ rE)
    assert st.cost(st.dev(poses), st.dev(w)) == cost


def test_weights_are_exact():
    barc2 = ref.BARC2
    st = pg.Staged(problem(2, [0], [1], np.stack([np.identity(4)] * 2), np.tile(ref.SIGMAS, (2, 1)), 0, np.stack([np.identity(4)] * 2)))
    for mu in (1e-6, 0.013, 1.0, 37.5):
        up, lo = (mu + 1.0) / mu * barc2, mu / (mu + 1.0) * barc2
        E = np.array([0.0, lo, np.nextafter(lo, np.inf), np.nextafter(lo, 0.0), up, np.nextafter(up, 0.0), np.nextafter(up, np.inf),
                      0.5 * (lo + up), barc2, 1e300, lo, up])
        known = np.zeros(len(E), dtype=np.uint8)
        known[-2:] = 1
        w = st.weights(st.dev(E), mu, barc2, st.torch.from_numpy(known).cuda()).cpu().numpy()
        want = ref.tls_weights(E, mu, barc2, known)
        assert np.array_equal(w, want), (mu, w, want)
        assert w[0] == 1.0 and w[1] == 1.0 and w[4] == 0.0 and w[6] == 0.0 and w[9] == 0.0 and w[-1] == 1.0
        assert 0.0 <= w[5] < 1.0 and 0.0 < w[2] <= 1.0
        assert np.array_equal(st.weights(st.dev(E), mu, barc2, None).cpu().numpy(), ref.tls_weights(E, mu, barc2, None))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
# entries of the 4 x 4 results after the same 20 - 30 accepted steps: measured 3.6e-15 .. 1.1e-14 on the four scenes (DESIGN.md
# 3.9); the tolerance is 100 x the largest
POSE_TOL = 1e-12
SCENES = {"seed1": (1, {}, True), "seed2": (2, {}, True), "seed5": (5, dict(n_true=8, n_out=3), True), "seed1-no-mask": (1, {}, False)}


# seed1-no-mask: without known inliers the restatement ends with odometry edge 33 rejected and one outlier kept on this scene (seeds
# 4, 6, 9 and 10 lose odometry edges as well); the case asserts that the GPU takes the same decisions, not what the weights are
@pytest.fixture(scope="module")
def planted():
    out = {}
    for name, (seed, kw, known) in SCENES.items():
        sc = ref.planted_scene(seed, **kw)
        out[name] = (sc, ref.gnc(sc.graph, sc.init, known=sc.known if known else None))
    return out


def describe_first_difference(got_trace, want_trace, fidelity=1e-3):
    for k, ((ga, gr_), (wa, wr)) in enumerate(zip(got_trace, want_trace)):
        if ga != wa:
            return "trial step %d: GPU %s (ratio %r), restatement %s (ratio %r, %.3g from the threshold %g)" % (
                k, "accepts" if ga else "rejects", gr_, "accepts" if wa else "rejects", wr, abs(wr - fidelity), fidelity)
    return "the first %d decisions agree; lengths %d and %d" % (min(len(got_trace), len(want_trace)), len(got_trace), len(want_trace))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_end_to_end_takes_the_restatement_s_decisions(planted, name):
    sc, want = planted[name]
    values, edges, prior, known = scene_args(sc, SCENES[name][2])
    got, trace = pg.optimize_staged(values, edges, prior, known, return_trace=True)
    why = describe_first_difference(trace, want["trace"])
    assert [a for a, _ in trace] == [a for a, _ in want["trace"]], why
    assert (got.gnc_rounds, got.lm_iterations, got.solves) == (want["rounds"], want["lm_iterations"], want["solves"]), why
    w = np.concatenate([got.weights, [got.prior_weight]])
    if SCENES[name][2]:
        assert np.all(w[sc.outliers] == 0.0) and np.all(w[~sc.outliers] == 1.0)
    # the weights of the last round: equal where they are 0 or 1, close in between (the no-mask case only asserts agreement)
    assert np.array_equal(w == 0.0, want["weights"] == 0.0) and np.array_equal(w == 1.0, want["weights"] == 1.0)
    assert np.abs(w - want["weights"]).max() <= 1e-6
    diff = max(np.abs(got.poses[(0, v)] - want["poses"][v]).max() for v in range(sc.graph.n))
    print("%s: %d rounds, %d iterations, %d solves; poses differ by %.3g; cost %.12g vs %.12g"
          % (name, got.gnc_rounds, got.lm_iterations, got.solves, diff, got.cost, want["cost"]))
    assert diff <= POSE_TOL
    assert abs(got.cost - want["cost"]) <= 1e-9 * want["cost"]
    # the one-call form runs the same launches in the same order
    one = pg.optimize(values, edges, prior, known)
    assert (one.gnc_rounds, one.lm_iterations, one.solves, one.cost, one.lam, one.status) == \
           (got.gnc_rounds, got.lm_iterations, got.solves, got.cost, got.lam, got.status)
    assert np.array_equal(one.weights, got.weights) and one.prior_weight == got.prior_weight
    assert all(np.array_equal(one.poses[k], got.poses[k]) for k in got.poses), "cslam_pgo_optimize == the staged sequence, bit for bit"
    assert list(pg.last_trace()) == [int(a) for a, _ in trace]


# |g|_inf where LM stops without tolerances (lambda runs past its bound once no step lowers the cost any more).  One factor's
# gradient entries are about (1 / sigma) (|e| / sigma) (lever 30 m) = 3e3 here, so eps 3e3 = 7e-13 is the rounding floor of one
# factor; measured 2.5e-12 (GPU) and 6.1e-11 (restatement).  The bound is 1e-8, about 150 x the larger; the two stationary points
# then differ by H^-1 applied to gradients of that size: measured 3.2e-11, bound 1e-9 (30 x).
GRAD_BOUND = 1e-8
STATIONARY_POSE_TOL = 1e-9


def test_without_tolerances_both_reach_a_stationary_point():
    sc = ref.planted_scene(1, n_out=0)
    values, edges, prior, known = scene_args(sc)
    params = dict(rel_tol=0.0, abs_tol=0.0, max_iter=50, gnc_max_rounds=0)
    got = pg.optimize(values, edges, prior, known, **params)
    want = ref.gnc(sc.graph, sc.init, known=sc.known, **params)
    assert got.gnc_rounds == 0 and want["rounds"] == 0
    poses = np.stack([got.poses[(0, v)] for v in range(sc.graph.n)])
    st = pg.Staged(scene_problem(sc))
    st.linearize(st.dev(poses), st.dev(np.ones(sc.graph.nf + 1)))
    g_gpu = np.abs(st.system()[1]).max()
    g_ref = np.abs(ref.linearize(sc.graph, want["poses"], np.ones(sc.graph.nf + 1))[2]).max()
    diff = np.abs(poses - want["poses"]).max()
    print("no tolerances: |g|_inf %.3g (GPU) %.3g (restatement); poses differ by %.3g; iterations %d / %d"
          % (g_gpu, g_ref, diff, got.lm_iterations, want["lm_iterations"]))
    assert g_gpu <= GRAD_BOUND and g_ref <= GRAD_BOUND
    assert diff <= STATIONARY_POSE_TOL


MODERATE_OUTLIER_SCALE = 10.0


def test_moderate_size_rejects_the_outliers_and_cuts_long_segments():
    """8 robots x 2000 poses, 200 closures, 10 outliers.  The restatement needs minutes for this size, so the properties are
    asserted: every outlier ends with weight 0, the cost is not above the cost of the noise-free truth under the same
    weights, and the PGO_SEG_MAX cut was exercised.

    The size of an outlier at this scale: about 420 closure end points over 16 000 poses leave chains of 40 - 80 poses between
    them, which at the default sigmas drift by 0.1 sqrt(80) = 0.9 m and by 0.01 sqrt(80) = 0.09 rad over a lever of some 40 m,
    3.6 m.  The 3 - 4 m perturbations of the small scene are inside that slack and no estimator can tell them from noise (the
    restatement keeps two of four of them on a 4 x 250 scene); here their translations are taken 10 times as large, 30 - 40 m,
    beside the same 0.37 - 0.62 rad."""
    sc = ref.planted_scene(7, robots=8, length=2000, n_true=200, n_out=10, outlier_scale=MODERATE_OUTLIER_SCALE)
    values, edges, prior, known = scene_args(sc)
    got = pg.optimize(values, edges, prior, known)
    w = np.concatenate([got.weights, [got.prior_weight]])
    st = pg.Staged(scene_problem(sc))
    at_truth = st.cost(st.dev(sc.truth), st.dev(w))
    print("moderate: %d rounds, %d iterations, %d solves, cost %.6g (truth %.6g), %d junctions, %d segments, %d cuts; outlier weights %s"
          % (got.gnc_rounds, got.lm_iterations, got.solves, got.cost, at_truth, got.junctions, got.segments, st.info["cut"], w[sc.outliers]))
    assert np.all(w[sc.outliers] == 0.0), w[sc.outliers]
    assert st.info["cut"] > 0 and st.info["longest"] == SEG_MAX
    assert got.status == 0 and got.cost <= at_truth


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_more_junctions_than_the_cap_is_a_limit_error():
    cap = 4096
    n = cap + 1
    poses = np.stack([np.identity(4)] * n)
    ei, ej = np.zeros(cap, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    meas, sig = np.stack([np.identity(4)] * (cap + 1)), np.tile(ref.SIGMAS, (cap + 1, 1))
    pr = problem(n, ei, ej, meas, sig, 0, poses)
    with pytest.raises(_lib.CslamLimitError):
        pg.Staged(pr)
    with pytest.raises(_lib.CslamLimitError):
        pg.optimize(*scene_like(pr))


def scene_like(pr):
    values = {k: pr.poses[v] for v, k in enumerate(pr.keys)}
    edges = [(pr.keys[pr.ei[k]], pr.keys[pr.ej[k]], pr.meas[k], pr.sig[k]) for k in range(pr.nf)]
    return values, edges, (pr.keys[pr.prior], pr.meas[pr.nf], pr.sig[pr.nf])


def test_argument_errors_are_python_errors_before_any_launch():
    I = np.identity(4)
    values = {(0, 0): I, (0, 1): I}
    with pytest.raises(KeyError):
        pg.optimize(values, [((0, 0), (0, 7), I, ref.SIGMAS)])
    with pytest.raises(ValueError):
        pg.optimize(values, [((0, 0), (0, 0), I, ref.SIGMAS)])
    with pytest.raises(ValueError):
        pg.optimize(values, [((0, 0), (0, 1), I, np.array([0.01, 0.01, 0.0, 0.1, 0.1, 0.1]))])
