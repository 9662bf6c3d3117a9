"""Float64 restatement of the pose-graph back end (csrc/pose.h, csrc/pgo.hip): numpy plus scipy.sparse.linalg.spsolve.

This is the project's own statement of the algorithm the kernels are held to, not GTSAM: SE(3) with the tangent
[omega, v], between factors e = Log(Z^-1 Ti^-1 Tj) with Aj = Jr_inv(e), Ai = -Jr_inv(e) Ad(h^-1), one prior, diagonal
noise, Levenberg-Marquardt with lambda I damping and GNC-TLS around it, every constant as the issue of the back end
states them (the reference's LevenbergMarquardtParams / GncParams defaults).
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

SERIES_THETA = 1e-2
LOG_SMALL_SIN = 1e-10
BARC2 = 0.5 * 16.811893829770927          # 1/2 chi2inv(0.99, 6)
SIGMAS = np.array([0.01, 0.01, 0.01, 0.1, 0.1, 0.1])
PARAMS = dict(lambda0=1e-5, factor=10.0, lambda_max=1e5, max_iter=100, rel_tol=1e-5, abs_tol=1e-5, fidelity=1e-3,
              gnc_max_rounds=100, mu_step=1.4, gnc_cost_tol=1e-5, weights_tol=1e-4, barc2=BARC2, mu_floor=1e-6)
PARAM_ORDER = ("lambda0", "factor", "lambda_max", "max_iter", "rel_tol", "abs_tol", "fidelity", "gnc_max_rounds", "mu_step",
               "gnc_cost_tol", "weights_tol", "barc2")


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def coef(th2):
    """a, b, c, d, q2, q3 of csrc/pose.h."""
    if th2 < SERIES_THETA * SERIES_THETA:
        t4 = th2 * th2
        return (1.0 - th2 / 6.0 + t4 / 120.0, 0.5 - th2 / 24.0 + t4 / 720.0, 1.0 / 6.0 - th2 / 120.0 + t4 / 5040.0,
                1.0 / 12.0 + th2 / 720.0 + t4 / 30240.0, 1.0 / 24.0 - th2 / 720.0 + t4 / 40320.0,
                1.0 / 120.0 - th2 / 2520.0 + t4 / 120960.0)
    t = np.sqrt(th2)
    s, c, sh = np.sin(t), np.cos(t), np.sin(0.5 * t)
    omc = 2.0 * sh * sh
    return (s / t, omc / th2, (t - s) / (th2 * t), (1.0 - 0.5 * t * np.cos(0.5 * t) / sh) / th2,
            (0.5 * th2 - omc) / (th2 * th2), (2.0 * t + t * c - 3.0 * s) / (2.0 * th2 * th2 * t))


def exp(xi):
    xi = np.asarray(xi, dtype=np.float64)
    w, v = xi[:3], xi[3:]
    a, b, c, _, _, _ = coef(float(w @ w))
    W = skew(w)
    W2 = W @ W
    T = np.identity(4)
    T[:3, :3] = np.identity(3) + a * W + b * W2
    T[:3, 3] = (np.identity(3) + b * W + c * W2) @ v
    return T


def so3_log(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif R[1, 1] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    q = np.array(q)
    if q[0] < 0.0:
        q = -q
    n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    f = 2.0 / q[0] if n < LOG_SMALL_SIN else 2.0 * np.arctan2(n, q[0]) / n
    return f * q[1:]


def log(T):
    w = so3_log(T[:3, :3])
    d = coef(float(w @ w))[3]
    W = skew(w)
    return np.concatenate([w, (np.identity(3) - 0.5 * W + d * (W @ W)) @ T[:3, 3]])


def inv(T):
    out = np.identity(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, :3] = skew(t) @ R
    A[3:, 3:] = R
    return A


def jr_inv(xi):
    """Inverse right Jacobian of SE(3) = Jl_inv(-xi), Barfoot's Q matrix."""
    xi = np.asarray(xi, dtype=np.float64)
    w, v = -xi[:3], -xi[3:]
    _, _, c, d, q2, q3 = coef(float(w @ w))
    W, V = skew(w), skew(v)
    Ji = np.identity(3) - 0.5 * W + d * (W @ W)
    WVW = W @ V @ W
    Q = (0.5 * V + c * (W @ V + V @ W + WVW) + q2 * (W @ W @ V + V @ W @ W - 3.0 * WVW) + q3 * (WVW @ W + W @ WVW))
    J = np.zeros((6, 6))
    J[:3, :3] = Ji
    J[3:, 3:] = Ji
    J[3:, :3] = -Ji @ Q @ Ji
    return J


def between(Ti, Tj, Z, jac=True):
    """e, Ai, Aj of a between factor; Ti None = the prior (Ai None)."""
    h = Tj if Ti is None else inv(Ti) @ Tj
    e = log(inv(Z) @ h)
    if not jac:
        return e, None, None
    J = jr_inv(e)
    return e, (None if Ti is None else -J @ adjoint(inv(h))), J


class Graph:
    """n poses, between factors (ei, ej, meas, sig) and the prior as the last factor (index nf) on pose `prior`."""

    def __init__(self, n, ei, ej, meas, sig, prior=0):
        self.n, self.ei, self.ej, self.prior = int(n), np.asarray(ei, dtype=np.int32), np.asarray(ej, dtype=np.int32), int(prior)
        self.meas, self.sig = np.asarray(meas, dtype=np.float64).reshape(-1, 4, 4), np.asarray(sig, dtype=np.float64).reshape(-1, 6)
        self.nf = len(self.ei)
        assert len(self.meas) == self.nf + 1 and len(self.sig) == self.nf + 1

    def factor(self, k):
        return (None, self.prior) if k == self.nf else (int(self.ei[k]), int(self.ej[k]))

    def pairs(self):
        """Distinct pose pairs (a < b), sorted: the order of the kernels' off-diagonal blocks."""
        return sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in zip(self.ei, self.ej)})


def errors(gr, poses):
    E = np.zeros(gr.nf + 1)
    for k in range(gr.nf + 1):
        i, j = gr.factor(k)
        e, _, _ = between(None if i is None else poses[i], poses[j], gr.meas[k], jac=False)
        E[k] = 0.5 * float(np.sum((e / gr.sig[k]) ** 2))
    return E


def linearize(gr, poses, w):
    """E [nf + 1], Hdiag [n, 6, 6], g [n, 6], Hoff {(a, b): 6 x 6 block (row a, column b)}; sums in ascending factor index."""
    E = np.zeros(gr.nf + 1)
    Hd, g, Ho = np.zeros((gr.n, 6, 6)), np.zeros((gr.n, 6)), {}
    for k in range(gr.nf + 1):
        i, j = gr.factor(k)
        e, Ai, Aj = between(None if i is None else poses[i], poses[j], gr.meas[k])
        E[k] = 0.5 * float(np.sum((e / gr.sig[k]) ** 2))
        s = np.sqrt(w[k]) / gr.sig[k]
        e, Aj = s * e, s[:, None] * Aj
        Hd[j] += Aj.T @ Aj
        g[j] += Aj.T @ e
        if i is not None:
            Ai = s[:, None] * Ai
            Hd[i] += Ai.T @ Ai
            g[i] += Ai.T @ e
            blk = Ai.T @ Aj
            key, blk = ((i, j), blk) if i < j else ((j, i), blk.T)
            Ho[key] = Ho.get(key, np.zeros((6, 6))) + blk
    return E, Hd, g, Ho


def assemble(n, Hd, Ho, lam=0.0):
    """The sparse 6n x 6n matrix H + lam I."""
    rows, cols, vals = [], [], []
    r6, c6 = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")

    def put(a, b, blk):
        rows.append((6 * a + r6).ravel()); cols.append((6 * b + c6).ravel()); vals.append(np.asarray(blk).ravel())
    for v in range(n):
        put(v, v, Hd[v] + lam * np.identity(6))
    for (a, b), blk in Ho.items():
        put(a, b, blk)
        put(b, a, blk.T)
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))


def solve(n, Hd, g, Ho, lam):
    """delta [n, 6] of (H + lam I) delta = -g and the model's predicted decrease -(g . d + 1/2 d . H d)."""
    d = spsolve(assemble(n, Hd, Ho, lam), -g.ravel())
    H = assemble(n, Hd, Ho, 0.0)
    return d.reshape(n, 6), -(float(g.ravel() @ d) + 0.5 * float(d @ (H @ d)))


def retract(poses, delta):
    return np.stack([poses[v] @ exp(delta[v]) for v in range(len(poses))])


def tls_weights(E, mu, barc2=BARC2, known=None):
    up, lo = (mu + 1.0) / mu * barc2, mu / (mu + 1.0) * barc2
    w = np.empty_like(E)
    for k, e in enumerate(E):
        if known is not None and known[k]:
            w[k] = 1.0
        elif e >= up:
            w[k] = 0.0
        elif e <= lo:
            w[k] = 1.0
        else:
            w[k] = np.sqrt(barc2 * mu * (mu + 1.0) / e) - mu
    return w


def lm(gr, poses, w, P, log_=None):
    """Levenberg-Marquardt; returns poses, cost, iterations, solves, lambda.  log_ collects (accept, ratio) per trial step."""
    lam = P["lambda0"]
    c = float(w @ errors(gr, poses))
    its = solves = 0
    stop = False
    while its < P["max_iter"] and not stop:
        _, Hd, g, Ho = linearize(gr, poses, w)
        while True:
            delta, predicted = solve(gr.n, Hd, g, Ho, lam)
            solves += 1
            accept, ratio, c_new, trial = False, float("nan"), c, None
            if predicted > 0.0:
                trial = retract(poses, delta)
                c_new = float(w @ errors(gr, trial))
                ratio = (c - c_new) / predicted
                accept = ratio > P["fidelity"]
            if log_ is not None:
                log_.append((accept, ratio))
            if accept:
                poses = trial
                lam /= P["factor"]
                break
            lam *= P["factor"]
            if lam > P["lambda_max"]:
                stop = True
                break
        if stop:
            break
        its += 1
        decrease = c - c_new
        if decrease < P["abs_tol"] or decrease / c < P["rel_tol"]:
            stop = True
        c = c_new
    return poses, c, its, solves, lam


def gnc(gr, poses, known=None, **params):
    """GNC-TLS around lm().  Returns a dict: poses, weights, rounds, lm_iterations, solves, cost, lam, trace."""
    P = dict(PARAMS, **params)
    nfac = gr.nf + 1
    w = np.ones(nfac)
    trace = []
    poses, cost, its, solves, lam = lm(gr, np.asarray(poses, dtype=np.float64), w, P, trace)
    rounds = 0
    E = errors(gr, poses)
    free = np.ones(nfac, dtype=bool) if known is None else ~np.asarray(known, dtype=bool)
    r = float(np.max(E[free] / P["barc2"])) if free.any() else -1.0
    if r >= 0.0 and 2.0 * r - 1.0 > 0.0:
        mu, prev = max(1.0 / (2.0 * r - 1.0), P["mu_floor"]), cost
        for _ in range(P["gnc_max_rounds"]):
            w = tls_weights(errors(gr, poses), mu, P["barc2"], known)
            poses, cost, i2, s2, lam = lm(gr, poses, w, P, trace)
            its, solves, rounds = its + i2, solves + s2, rounds + 1
            if np.all((np.abs(w) <= P["weights_tol"]) | (np.abs(w - 1.0) <= P["weights_tol"])):
                break
            if abs(cost - prev) / max(prev, 1e-7) < P["gnc_cost_tol"]:
                break
            prev = cost
            mu *= P["mu_step"]
    return dict(poses=poses, weights=w, rounds=rounds, lm_iterations=its, solves=solves, cost=cost, lam=lam, trace=trace)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
STEP = np.array([0.02, -0.01, 0.15, 1.0, 0.05, 0.01])
OUTLIER_XI = (np.array([0.2, -0.1, 0.3, 3.0, -2.0, 0.5]), np.array([-0.3, 0.2, -0.5, -4.0, 1.0, 2.0]),
              np.array([0.25, 0.3, -0.2, 2.0, 3.0, -1.5]))


class Scene:
    pass


def planted_scene(seed, robots=2, length=30, n_true=6, n_out=2, intra=((0, 28), (4, 25)), outlier_scale=1.0):
    """R robots x `length` poses on the same step, robot r offset by a fixed transform.  Every measurement carries noise at
    the default sigmas; n_true random inter-robot closures (the first ones chain robot r to robot r - 1), the intra-robot
    closures of robot 0, n_out gross inter-robot outliers (OUTLIER_XI, its translation part times outlier_scale: a scaled rotation
    vector would wrap, 10 x (-0.3, 0.2, -0.5) is a turn of 2 pi - 0.12).  Robot 0 is initialised from its odometry, the others are anchored
    through their first closure.  Factor order: odometry, true closures, intra closures, outliers, then the prior (pose 0)."""
    rng = np.random.default_rng(seed)
    n = robots * length
    step = exp(STEP)
    truth = np.zeros((n, 4, 4))
    for r in range(robots):
        T = exp(np.array([0.0, 0.0, 0.3 * r, 2.0 * r, 5.0 * r, 0.0]))
        for k in range(length):
            truth[r * length + k] = T
            T = T @ step

    def noisy(i, j):
        return inv(truth[i]) @ truth[j] @ exp(rng.standard_normal(6) * SIGMAS)
    ei, ej, meas = [], [], []
    for r in range(robots):
        for k in range(length - 1):
            ei.append(r * length + k); ej.append(r * length + k + 1); meas.append(noisy(ei[-1], ej[-1]))
    n_odo = len(ei)
    true_pairs = []
    for r in range(1, robots):                                       # one closure that anchors robot r
        true_pairs.append(((r - 1) * length + int(rng.integers(length)), r * length + int(rng.integers(length))))
    while len(true_pairs) < n_true:
        ra, rb = sorted(rng.choice(robots, 2, replace=False))
        true_pairs.append((int(ra) * length + int(rng.integers(length)), int(rb) * length + int(rng.integers(length))))
    for i, j in true_pairs:
        ei.append(i); ej.append(j); meas.append(noisy(i, j))
    for i, j in intra:
        ei.append(i); ej.append(j); meas.append(noisy(i, j))
    out_at = len(ei)
    for o in range(n_out):
        ra, rb = sorted(rng.choice(robots, 2, replace=False))
        i, j = int(ra) * length + int(rng.integers(length)), int(rb) * length + int(rng.integers(length))
        ei.append(i); ej.append(j); meas.append(noisy(i, j) @ exp(OUTLIER_XI[o % len(OUTLIER_XI)] * np.array([1.0, 1.0, 1.0] + [outlier_scale] * 3)))
    nf = len(ei)
    meas.append(truth[0].copy())                                     # the prior's measurement
    sig = np.tile(SIGMAS, (nf + 1, 1))
    init = np.zeros((n, 4, 4))
    init[0] = truth[0]
    for k in range(length - 1):
        init[k + 1] = init[k] @ meas[k]
    for r in range(1, robots):
        i, j = true_pairs[r - 1]
        init[j] = init[i] @ meas[n_odo + r - 1]
        base = r * length
        for k in range(j - base, length - 1):
            init[base + k + 1] = init[base + k] @ meas[r * (length - 1) + k]
        for k in range(j - base, 0, -1):
            init[base + k - 1] = init[base + k] @ inv(meas[r * (length - 1) + k - 1])
    s = Scene()
    s.graph = Graph(n, ei, ej, np.stack(meas), sig, prior=0)
    s.init, s.truth, s.n_odo, s.out_at = init, truth, n_odo, out_at
    s.outliers = np.zeros(nf + 1, dtype=bool)
    s.outliers[out_at:nf] = True
    s.known = np.zeros(nf + 1, dtype=np.uint8)
    s.known[:n_odo] = 1
    s.known[nf] = 1
    return s


def path_edges(walk, reverse):
    """The edges of a walk; reversed: listed from its far end, every edge (v, u) for (u, v)."""
    ed = list(zip(walk[:-1], walk[1:]))
    return [(v, u) for u, v in ed[::-1]] if reverse else ed


def subdivided_complete(k):
    """K_k whose edge (a, b), a < b, carries (a + b) mod 3 interior poses (numbered from k on); where a + b is odd the path is
    listed from b to a.  For k = 9: 12 direct pairs, 24 segments, 45 poses."""
    ed, nxt = [], k
    for a in range(k):
        for b in range(a + 1, k):
            m = (a + b) % 3
            ed += path_edges([a] + list(range(nxt, nxt + m)) + [b], (a + b) % 2 == 1)
            nxt += m
    return ed


def integer_system(N, seed, density=1.0):
    """L, A = L L^T, x, b = A x, all int64.  L is lower triangular with off-diagonal entries from {-2 .. 2} (kept with
    probability `density`, zero otherwise) and a diagonal from {1, 2, 3, 4}; x is from {-3 .. 3}.  Every Schur complement
    A - L[:, :k] L[:, :k]^T = L[:, k:] L[:, k:]^T and every partial sum of it, in any order, is an integer below
    4 N max|L|^2 < 2^53; the pivots are perfect squares, the divisions leave integers: a float64 Cholesky factor and both
    triangular solves are exact whatever their summation order and whether or not products are fused."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.integers(-2, 3, (N, N)), -1)
    if density < 1.0:
        L *= rng.random((N, N)) < density
    L[np.arange(N), np.arange(N)] = rng.integers(1, 5, N)
    L = L.astype(np.int64)
    x = rng.integers(-3, 4, N).astype(np.int64)
    A = L @ L.T
    return L, A, x, A @ x


def plan_graphs(seg_max):
    """name -> (n, ei, ej, prior): the structures the plan and the solver are tested on."""
    def chain(a, b):
        return [(k, k + 1) for k in range(a, b)]
    out = {}
    out["chain2"] = (2, [(0, 1)], 0)
    out["ring"] = (7, chain(0, 6) + [(6, 0)], 3)
    out["ring-no-prior-junction"] = (12, chain(0, 4) + [(4, 0)] + chain(5, 11) + [(11, 5)] + [(0, 5)], 0)
    out["star"] = (9, [(0, k) for k in range(1, 9)], 0)
    out["complete8"] = (8, [(a, b) for a in range(8) for b in range(a + 1, 8)], 2)
    out["adjacent-junctions"] = (10, chain(0, 9) + [(3, 7), (4, 8), (5, 9)], 0)      # 3-4-5 adjacent, 5 and 7 one apart
    out["dangling"] = (8, chain(0, 5) + [(2, 6), (6, 7)], 0)
    out["parallel"] = (6, chain(0, 5) + [(2, 3), (3, 2), (0, 4), (4, 0)], 1)
    for m in (seg_max - 1, seg_max, seg_max + 1, 2 * seg_max + 2):
        out["segment-%d" % m] = (m + 2, chain(0, m + 1), 0)                          # m poses between two chain ends
    out["two-components"] = (11, chain(0, 4) + chain(5, 10) + [(5, 8)], 0)
    out["reversed"] = (6, [(k + 1, k) for k in range(5)] + [(5, 1)], 0)
    out["loop-at-junction"] = (6, [(0, 1), (1, 2), (2, 3), (3, 1), (1, 4), (4, 5)], 0)
    # the dense factor's panel edges (48 columns = 8 junctions a panel): two exact panels, and a 6-row remainder after them
    out["complete16"] = (16, [(a, b) for a in range(16) for b in range(a + 1, 16)], 2)
    out["complete17"] = (17, [(a, b) for a in range(17) for b in range(a + 1, 17)], 2)
    # 7 x 8 lattice: the four corners have two neighbours and become one-pose segments, 52 junctions, N = 312 > 256 + 48
    out["grid7x8"] = (56, [(8 * r + c, 8 * r + c + 1) for r in range(7) for c in range(7)]
                      + [(8 * r + c, 8 * r + c + 8) for r in range(6) for c in range(8)], 8 * 3 + 3)
    out["subdivided9"] = (45, subdivided_complete(9), 0)
    # junctions 0 and 1: a direct edge, its reversed duplicate, and paths of 1, 2, 3 and 5 interior poses; the second and the
    # fourth are listed from 1 to 0
    bundle, nxt = [(0, 1), (1, 0)], 2
    for k, m in enumerate((1, 2, 3, 5)):
        walk = [0] + list(range(nxt, nxt + m)) + [1]
        nxt += m
        bundle += path_edges(walk, k % 2 == 1)
    out["bundle"] = (nxt, bundle, 0)
    return {k: (n, np.array([e[0] for e in ed], dtype=np.int32), np.array([e[1] for e in ed], dtype=np.int32), p)
            for k, (n, ed, p) in out.items()}


def random_graph_values(n, ei, ej, seed, spread=0.3):
    """Poses, consistent-but-noisy measurements and sigmas for a structure: (poses [n,4,4], meas [nf+1,4,4], sig [nf+1,6])."""
    rng = np.random.default_rng(seed)
    poses = np.stack([exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-5, 5, 3)])) for _ in range(n)])
    meas = [inv(poses[i]) @ poses[j] @ exp(rng.standard_normal(6) * spread) for i, j in zip(ei, ej)]
    return poses, np.stack(meas + [np.identity(4)]), np.tile(SIGMAS, (len(ei) + 1, 1)) * rng.uniform(0.5, 2.0, (len(ei) + 1, 6))
