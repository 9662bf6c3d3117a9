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
def check_solve_against_spsolve(st, n, name, lams):
    """The two bounds of test_solve_against_spsolve on the system `st` has linearised, at every lambda of `lams`."""
    Hd, g, Ho, pa, pb = st.system()
    Hoff = {(int(a), int(b)): Ho[q] for q, (a, b) in enumerate(zip(pa, pb))}
    for lam in lams:
        A = ref.assemble(n, Hd, Hoff, lam)
        b = -g.ravel()
        want = spsolve(A, b)
        delta, status, predicted = st.solve(lam)
        got = delta.cpu().numpy().ravel().copy()
        assert status == 0
        res = lambda x: np.linalg.norm(A @ x - b)
        print("%s lam %g: residual %.3g (spsolve %.3g), %.2f x" % (name, lam, res(got) / np.linalg.norm(b), res(want) / np.linalg.norm(b),
                                                                  res(got) / res(want)))
        assert res(got) <= 10.0 * res(want), (name, lam, res(got), res(want))
        inv_norm = 1.0 / np.linalg.eigvalsh(A.toarray())[0]
        assert np.linalg.norm(got - want) <= inv_norm * (res(got) + res(want)), (name, lam)
        H = ref.assemble(n, Hd, Hoff, 0.0)
        model = -(float(g.ravel() @ got) + 0.5 * float(got @ (H @ got)))
        assert abs(predicted - model) <= 1e-12 * (abs(float(g.ravel() @ got)) + abs(float(got @ (H @ got))))
        delta2, _, predicted2 = st.solve(lam)
        assert np.array_equal(delta2.cpu().numpy().ravel(), got) and predicted2 == predicted, "two runs must agree bit for bit"


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
    check_solve_against_spsolve(st, n, name, [1e-5, 1e5] + ([] if name == "two-components" else [0.0]))   # no prior there: singular at 0


def test_solve_against_spsolve_at_mid_size():
    """4 robots x 120 poses and 40 closures: at least 87 junctions, so a dense system of 522 rows or more, 11 panels, three
    workgroups in the rows kernel and three strides in the triangular solve, with segments of every length between them."""
    sc = ref.planted_scene(3, robots=4, length=120, n_true=40, n_out=0)
    st = pg.Staged(scene_problem(sc))
    assert sc.graph.n == 480 and st.info["junctions"] >= 87 and st.info["segments"] > 0
    st.linearize(st.dev(sc.init), st.dev(np.ones(sc.graph.nf + 1)))
    check_solve_against_spsolve(st, sc.graph.n, "mid-size (%d junctions)" % st.info["junctions"], [1e-5, 1e5])


def test_non_positive_pivot_is_a_status():
    """Weights of zero on every factor: H = 0, and at lambda = 0 the first pivot is not positive.  Nothing aborts."""
    n, ei, ej, prior = ref.plan_graphs(SEG_MAX)["adjacent-junctions"]
    poses, meas, sig = ref.random_graph_values(n, ei, ej, 3)
    st = pg.Staged(problem(n, ei, ej, meas, sig, prior, poses))
    st.linearize(st.dev(poses), st.dev(np.zeros(len(ei) + 1)))
    assert st.solve(0.0)[1] == 1
    assert st.solve(1.0)[1] == 0


# ---- the dense factor on its own: cslam_pgo_dense_solve_dev, the launch sequence pgo_solve runs ------------------------------------------
NB = 48                                                      # PGO_CHOL_NB
# one short panel; exactly one; one row over; two exact panels; full panels and remainders of 1, 6 and 24; the last N with one
# workgroup in the rows kernel (256 rows below the first panel) and the first with two; a 7 x 7 tile grid whose last tile has one row
DENSE_SIZES = (1, 6, 47, 48, 49, 54, 96, 97, 102, 304, 305, 312, 337, 354)
DENSE_CASES = [(N, 1.0) for N in DENSE_SIZES] + [(102, 0.1), (354, 0.1)]       # 10 % fill: no neighbour hides a skipped tile


def dense_solve(A, b, upper=None):
    """Lower triangle of S and the solution after the call, the whole S, the status.  `upper` fills the strict upper triangle."""
    import torch
    S = np.array(A, dtype=np.float64)
    if upper is not None:
        S[np.triu_indices(len(S), 1)] = upper
    dS, drhs = torch.from_numpy(S).cuda(), torch.from_numpy(np.array(b, dtype=np.float64)).cuda()
    status = pg.dense_solve(dS, drhs)
    S = dS.cpu().numpy()
    return np.tril(S), drhs.cpu().numpy(), S, status


def first_difference(got, want, what, cols=None):
    """'' when the arrays agree; else where they first differ, in the terms of the kernels: panel = column block of 48, and
    the update tile (ti, tj) that entry has after panel k is (row block - k - 1, column block - k - 1)."""
    bad = got != want
    if cols is not None:
        bad[:, cols:] = False
    if not bad.any():
        return ""
    if got.ndim == 1:
        r = int(np.flatnonzero(bad)[0])
        return "%s: %d of %d entries differ, first at row %d (panel %d, row %d in it, stride %d of the triangular solve): got %r, want %r" % (
            what, bad.sum(), bad.size, r, r // NB, r % NB, r // 256, got[r], want[r])
    c = int(np.flatnonzero(bad.any(axis=0))[0])                 # columns are finished left to right
    r = int(np.flatnonzero(bad[:, c])[0])
    return ("%s: %d entries differ, the leftmost column's first at row %d, column %d: panel %d (column %d in it), row block %d (row %d in "
            "it; tile (%d, %d) of the update after panel 0; rows kernel workgroup %d); got %r, want %r"
            % (what, bad.sum(), r, c, c // NB, c % NB, r // NB, r % NB, r // NB - 1, c // NB - 1, max(r - (c // NB + 1) * NB, 0) // 256,
               got[r, c], want[r, c]))


@pytest.mark.parametrize("N,density", DENSE_CASES)
def test_dense_factor_and_solution_are_exact_on_integer_systems(N, density):
    """A = L L^T and b = A x in integers (ref.integer_system): every intermediate of the factor and of both solves is an
    integer below 2^53, so the factor is L and the solution x to the bit, whatever the order of the sums.  No tolerance."""
    L, A, x, b = ref.integer_system(N, 100 + N, density)
    F, sol, S, status = dense_solve(A, b)
    why = first_difference(F, L.astype(np.float64), "factor N = %d (status %d)" % (N, status))
    assert np.array_equal(F, L.astype(np.float64)), why
    assert status == 0
    assert np.array_equal(np.triu(S, 1), np.triu(A.astype(np.float64), 1)), "the strict upper triangle is not written"
    why = first_difference(sol, x.astype(np.float64), "solution N = %d" % N)
    assert np.array_equal(sol, x.astype(np.float64)), why
    F2, sol2, S2, status2 = dense_solve(A, b)
    assert status2 == 0 and np.array_equal(S2, S) and np.array_equal(sol2, sol), "two runs must agree bit for bit"


@pytest.mark.parametrize("N", (49, 354))
def test_dense_solve_never_touches_the_strict_upper_triangle(N):
    """NaN (with a payload) above the diagonal on entry: the same bits there on exit, none below it or in the solution."""
    L, A, x, b = ref.integer_system(N, 200 + N)
    nan = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]
    F, sol, S, status = dense_solve(A, b, upper=nan)
    iu = np.triu_indices(N, 1)
    assert status == 0 and np.all(S[iu].view(np.uint64) == np.uint64(0x7ff8dead0000beef))
    assert not np.isnan(F).any() and not np.isnan(sol).any()
    assert np.array_equal(F, L.astype(np.float64)), first_difference(F, L.astype(np.float64), "factor N = %d" % N)
    assert np.array_equal(sol, x.astype(np.float64)), first_difference(sol, x.astype(np.float64), "solution N = %d" % N)


@pytest.mark.parametrize("p", (0, 47, 48, 100, 101))
def test_dense_zero_pivot_is_a_status_and_leaves_the_columns_before_it(p):
    """A[p][p] lowered by L[p][p]^2 makes the pivot of column p exactly 0: first column, panel end, panel start, remainder
    panel, last column of N = 102.  The call returns, the status says so, and columns < p are still L's."""
    N = 102
    L, A, x, b = ref.integer_system(N, 300)
    assert dense_solve(A, b)[3] == 0
    A = A.copy()
    A[p, p] -= L[p, p] ** 2
    F, sol, S, status = dense_solve(A, b)
    assert status == 1
    why = first_difference(F, L.astype(np.float64), "columns before the pivot %d" % p, cols=p)
    assert np.array_equal(F[:, :p], L[:, :p].astype(np.float64)), why


def gamma(k):
    u = np.longdouble(2.0) ** -53
    return k * u / (1 - k * u)


def real_system(N, graded, seed):
    """A = G G^T / N + I (condition about 5), or D A D with D graded from 1 to 1e-4 (condition about 1e8); b = A x."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, N))
    A = G @ G.T / N + np.identity(N)
    A = 0.5 * (A + A.T)
    if graded:
        D = 10.0 ** (-4.0 * np.arange(N) / (N - 1))
        A = A * D[:, None] * D[None, :]
    return A, A @ rng.uniform(-1.0, 1.0, N)


@pytest.mark.parametrize("N,graded", [(102, False), (102, True), (354, False), (354, True)])
def test_dense_factor_and_solve_meet_the_backward_error_bounds(N, graded):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorems 10.3 and 10.4, component-wise, in np.longdouble on the
    factor L the GPU returned:  |A - L L^T| <= gamma_k |L| |L^T| with k = 2 (N + 1), and |b - A x| <= gamma_k |L| |L^T| |x| with
    k = 2 (3 N + 1); gamma_k = k u / (1 - k u), u = 2^-53.  They hold for any order of the sums and with fused multiply-adds;
    the 2 in k allows a square root and a division within one ulp that are not correctly rounded.  Nothing is measured.
    On one MI355X the worst entry is at 0.037 (factor) and 0.013 (solve) of its bound, both on the graded N = 102."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the bounds are evaluated in 80-bit arithmetic"
    A, b = real_system(N, graded, 400 + N)
    cond = np.linalg.cond(A)
    assert (cond < 10.0) if not graded else (1e7 < cond < 1e9), cond
    F, sol, S, status = dense_solve(A, b)
    assert status == 0
    Al, Fl, xl, bl = (np.asarray(v, dtype=np.longdouble) for v in (A, F, sol, b))
    env = np.abs(Fl) @ np.abs(Fl.T)
    fac = np.abs(Al - Fl @ Fl.T) / (gamma(2 * (N + 1)) * env)
    slv = np.abs(bl - Al @ xl) / (gamma(2 * (3 * N + 1)) * (env @ np.abs(xl)))
    print("dense N = %d cond %.3g: worst |A - L L^T| at %.4f of its bound, worst |b - A x| at %.4f of its bound"
          % (N, cond, float(fac.max()), float(slv.max())))
    r, c = np.unravel_index(int(np.argmax(fac)), fac.shape)
    assert fac.max() <= 1.0, "row %d, column %d (panel %d, row block %d): %r of the bound" % (r, c, c // NB, r // NB, float(fac.max()))
    assert slv.max() <= 1.0, "row %d: %r of the bound" % (int(np.argmax(slv)), float(slv.max()))


def test_dense_solve_argument_errors_come_before_any_launch():
    import ctypes as C
    import torch
    lib = _lib.load()
    S, rhs, status = torch.eye(6, dtype=torch.float64, device="cuda"), torch.ones(6, dtype=torch.float64, device="cuda"), C.c_int(7)
    cap = 6 * 4096
    for args in ((None, 6, rhs.data_ptr(), C.byref(status)), (S.data_ptr(), 6, None, C.byref(status)), (S.data_ptr(), 6, rhs.data_ptr(), None),
                 (S.data_ptr(), 0, rhs.data_ptr(), C.byref(status)), (S.data_ptr(), -6, rhs.data_ptr(), C.byref(status)),
                 (S.data_ptr(), cap + 1, rhs.data_ptr(), C.byref(status))):
        with pytest.raises(_lib.CslamHipError, match="cslam_pgo_dense_solve_dev"):
            _lib.check(lib.cslam_pgo_dense_solve_dev(*args, None))
    torch.cuda.synchronize()
    assert status.value == 7 and np.array_equal(S.cpu().numpy(), np.identity(6)) and np.array_equal(rhs.cpu().numpy(), np.ones(6))
    with pytest.raises(ValueError):
        pg.dense_solve(S, rhs[:5])
    with pytest.raises(ValueError):
        pg.dense_solve(S.float(), rhs)
    with pytest.raises(ValueError):
        pg.dense_solve(S.t()[:, :3], rhs)
    assert pg.dense_solve(S, rhs) == 0


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
