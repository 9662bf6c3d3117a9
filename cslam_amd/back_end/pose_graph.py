"""Pose-graph optimisation on the GPU: GNC-TLS around Levenberg-Marquardt on SE(3) (csrc/pgo.hip).

Replaces what the reference hands to GTSAM in src/back_end/decentralized_pgo.cpp:797-827 (`DecentralizedPGO::optimize`:
`GncOptimizer<GncParams<LevenbergMarquardtParams>>` over `BetweenFactor<Pose3>` with diagonal noise, default sigmas 0.01 rad
and 0.1 m, :64-70, and one prior on the first pose, :843-845).  Edges carry what `PoseGraphEdge` carries
(src/back_end/gtsam_utils.cpp:58-89): two keys (robot_id, keyframe_id), a measurement and noise_std[6], rotation first.

GTSAM is third party and was not available to compare against, so parity with GTSAM itself is unpinned: the algorithm is
the one csrc/pgo.hip states and tests/pgo_reference.py restates in float64.

`known_inliers` defaults to none, as in the reference.  Without it GNC rejects odometry edges on some graphs (the planted
scene of tests/test_pgo_gpu.py, seed 1, ends with one odometry edge rejected and one gross outlier kept; with the mask both
come out right); pass the odometry and the prior as known inliers to rule it out.

There is no CPU path: without the library or a GPU, optimize() raises CslamHipError.  read_g2o / write_g2o are host only.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib

DEFAULT_NOISE_STD = np.array([0.01, 0.01, 0.01, 0.1, 0.1, 0.1])
BARC2 = 0.5 * 16.811893829770927          # 1/2 chi2inv(0.99, 6): GncParams' default inlier threshold for 6 dof
PARAM_ORDER = ("lambda0", "factor", "lambda_max", "max_iter", "rel_tol", "abs_tol", "fidelity", "gnc_max_rounds", "mu_step",
               "gnc_cost_tol", "weights_tol", "barc2")
DEFAULT_PARAMS = dict(lambda0=1e-5, factor=10.0, lambda_max=1e5, max_iter=100, rel_tol=1e-5, abs_tol=1e-5, fidelity=1e-3,
                      gnc_max_rounds=100, mu_step=1.4, gnc_cost_tol=1e-5, weights_tol=1e-4, barc2=BARC2)
MU_FLOOR = 1e-6

PoseGraphEdge = namedtuple("PoseGraphEdge", "key_from key_to measurement noise_std")
PoseGraphResult = namedtuple("PoseGraphResult", "poses weights prior_weight inliers gnc_rounds lm_iterations solves cost lam status "
                                                "junctions segments")


def quat_to_rot(q):
    """(qx, qy, qz, qw) -> 3 x 3."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(R):
    """3 x 3 -> (qx, qy, qz, qw), qw >= 0 (Shepperd's branches)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = ((R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s)
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = (0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s)
    elif R[1, 1] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = ((R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s)
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = ((R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s)
    q = np.array(q)
    return -q if q[3] < 0.0 else q


def as_pose(p):
    """A 4 x 4 matrix, or 7 numbers: position then quaternion (x y z qx qy qz qw)."""
    p = np.asarray(p, dtype=np.float64)
    if p.shape == (4, 4):
        return p.copy()
    if p.shape == (7,):
        T = np.identity(4)
        T[:3, :3] = quat_to_rot(p[3:])
        T[:3, 3] = p[:3]
        return T
    raise ValueError("a pose is a 4 x 4 matrix or 7 numbers (x y z qx qy qz qw), not shape %s" % (p.shape,))


def _edge(e):
    if hasattr(e, "key_from"):
        kf, kt, meas, std = e.key_from, e.key_to, e.measurement, e.noise_std
        if hasattr(kf, "robot_id"):
            kf, kt = (kf.robot_id, kf.keyframe_id), (kt.robot_id, kt.keyframe_id)
        return tuple(kf), tuple(kt), meas, std
    kf, kt, meas, std = e
    return tuple(kf), tuple(kt), meas, std


class Problem:
    """The host arrays of one optimisation, checked: everything that can be wrong with the input raises here, before any launch."""

    def __init__(self, values, edges, prior=None, known_inliers=None):
        if not values:
            raise ValueError("no poses")
        self.keys = sorted(values)
        index = {k: v for v, k in enumerate(self.keys)}
        self.n, self.nf = len(self.keys), len(edges)
        self.poses = np.stack([as_pose(values[k]) for k in self.keys])
        self.ei, self.ej = np.zeros(self.nf, dtype=np.int32), np.zeros(self.nf, dtype=np.int32)
        self.meas, self.sig = np.zeros((self.nf + 1, 4, 4)), np.zeros((self.nf + 1, 6))
        for k, e in enumerate(edges):
            kf, kt, meas, std = _edge(e)
            if kf not in index or kt not in index:
                raise KeyError("edge %d names a pose that is not among the values: %s -> %s" % (k, kf, kt))
            if kf == kt:
                raise ValueError("edge %d joins pose %s to itself" % (k, kf))
            self.ei[k], self.ej[k], self.meas[k], self.sig[k] = index[kf], index[kt], as_pose(meas), np.asarray(std, dtype=np.float64)
        if prior is None:                                   # the reference: the first pose's current estimate, default noise
            prior = (self.keys[0], values[self.keys[0]], DEFAULT_NOISE_STD)
        pk, pz, ps = prior
        if tuple(pk) not in index:
            raise KeyError("the prior names a pose that is not among the values: %s" % (pk,))
        self.prior = index[tuple(pk)]
        self.meas[self.nf], self.sig[self.nf] = as_pose(pz), np.asarray(ps, dtype=np.float64)
        if not (np.all(np.isfinite(self.sig)) and np.all(self.sig > 0.0)):
            raise ValueError("noise_std must be positive and finite")
        if not (np.all(np.isfinite(self.poses)) and np.all(np.isfinite(self.meas))):
            raise ValueError("poses and measurements must be finite")
        self.known = None
        if known_inliers is not None:
            self.known = np.ascontiguousarray(known_inliers, dtype=np.uint8)
            if self.known.shape != (self.nf + 1,):
                raise ValueError("known_inliers has one entry per edge and one for the prior (the last): %d, not %s"
                                 % (self.nf + 1, self.known.shape))


def _params(params):
    unknown = set(params) - set(DEFAULT_PARAMS)
    if unknown:
        raise TypeError("unknown parameters: %s" % sorted(unknown))
    return dict(DEFAULT_PARAMS, **params)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _result(pr, poses, weights, info):
    w = np.asarray(weights)
    return PoseGraphResult(poses={k: poses[v].copy() for v, k in enumerate(pr.keys)}, weights=w[:pr.nf].copy(), prior_weight=float(w[pr.nf]),
                           inliers=w[:pr.nf] > 0.5, gnc_rounds=int(info[0]), lm_iterations=int(info[1]), solves=int(info[2]),
                           cost=float(info[3]), lam=float(info[4]), status=int(info[5]), junctions=int(info[6]), segments=int(info[7]))


def optimize(values, edges, prior=None, known_inliers=None, **params):
    """values {(robot_id, keyframe_id): pose}; edges: PoseGraphEdge-like objects or (key_from, key_to, measurement, noise_std)
    tuples; prior (key, pose, noise_std), default the first key at its value with the default sigmas; known_inliers: one flag
    per edge plus one for the prior.  Returns a PoseGraphResult: poses by key, per-edge GNC weights, the inlier mask and the
    info figures.  One call of cslam_pgo_optimize."""
    pr = Problem(values, edges, prior, known_inliers)
    P = _params(params)
    lib = _lib.load()
    _lib.require_gpu()
    poses = np.ascontiguousarray(pr.poses)
    weights, info = np.zeros(pr.nf + 1), np.zeros(8)
    pv = np.array([float(P[k]) for k in PARAM_ORDER])
    _lib.check(lib.cslam_pgo_optimize(pr.n, pr.nf, _ptr(pr.ei), _ptr(pr.ej), pr.prior, _ptr(poses), _ptr(pr.meas), _ptr(pr.sig),
                                      _ptr(pr.known) if pr.known is not None else None, _ptr(pv), _ptr(weights), _ptr(info)))
    return _result(pr, poses, weights, info)


def last_trace():
    """Accept (1) / reject (0) of every trial step of the last optimize() call."""
    lib = _lib.load()
    count = C.c_int64(0)
    _lib.check(lib.cslam_pgo_trace(None, 0, C.byref(count)))
    out = np.zeros(max(count.value, 1), dtype=np.int32)
    _lib.check(lib.cslam_pgo_trace(_ptr(out), count.value, C.byref(count)))
    return out[:count.value]


def dense_solve(S, rhs):
    """cslam_pgo_dense_solve_dev on float64 device tensors, in place: S [N, N] (its lower triangle becomes the factor) and
    rhs [N] (becomes the solution).  Returns the status, 1 on a non-positive pivot.  Needs no plan."""
    lib = _lib.load()
    _lib.require_gpu()
    if not (S.is_cuda and rhs.is_cuda and S.is_contiguous() and rhs.is_contiguous() and str(S.dtype) == str(rhs.dtype) == "torch.float64"):
        raise ValueError("S and rhs must be contiguous float64 device tensors")
    if S.dim() != 2 or S.shape[0] != S.shape[1] or tuple(rhs.shape) != (S.shape[0],):
        raise ValueError("S must be N x N and rhs N, not %s and %s" % (tuple(S.shape), tuple(rhs.shape)))
    status = C.c_int(0)
    _lib.check(lib.cslam_pgo_dense_solve_dev(S.data_ptr(), S.shape[0], rhs.data_ptr(), C.byref(status), None))
    return status.value


class Staged:
    """The staged entries (cslam_pgo_*_dev) on one graph, device arrays held as torch tensors: what the tests drive kernel
    by kernel, and optimize_staged() below the same loop as cslam_pgo_optimize written in Python."""

    def __init__(self, pr):
        import torch
        self.lib = _lib.load()
        _lib.require_gpu()
        self.pr, self.torch = pr, torch
        info = np.zeros(8, dtype=np.int64)
        _lib.check(self.lib.cslam_pgo_plan(pr.n, pr.nf, _ptr(pr.ei), _ptr(pr.ej), pr.prior, _ptr(info)))
        self.info = dict(zip(("junctions", "segments", "interior", "pairs", "cut", "longest", "seg_max", "max_junctions"), info.tolist()))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.meas, self.sig = dev(pr.meas), dev(pr.sig)
        self.known = dev(pr.known) if pr.known is not None else None
        self.E = torch.zeros(pr.nf + 1, dtype=torch.float64, device="cuda")
        self.delta = torch.zeros(pr.n, 6, dtype=torch.float64, device="cuda")

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    def linearize(self, poses, w):
        _lib.check(self.lib.cslam_pgo_linearize_dev(poses.data_ptr(), self.meas.data_ptr(), self.sig.data_ptr(), w.data_ptr(),
                                                    self.E.data_ptr(), None))
        return self.E

    def system(self):
        """E is what linearize returned; here Hdiag [n, 6, 6], g [n, 6], Hoff [pairs, 6, 6], pa, pb."""
        n, P = self.pr.n, self.info["pairs"]
        Hd, g, Ho = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros((max(P, 1), 6, 6))
        pa, pb = np.zeros(max(P, 1), dtype=np.int32), np.zeros(max(P, 1), dtype=np.int32)
        _lib.check(self.lib.cslam_pgo_system_host(_ptr(Hd), _ptr(g), _ptr(Ho), _ptr(pa), _ptr(pb), None))
        return Hd, g, Ho[:P], pa[:P], pb[:P]

    def solve(self, lam):
        status, predicted = C.c_int(0), C.c_double(0.0)
        _lib.check(self.lib.cslam_pgo_solve_dev(float(lam), self.delta.data_ptr(), C.byref(status), C.byref(predicted), None))
        return self.delta, status.value, predicted.value

    def retract(self, poses, delta):
        out = self.torch.empty_like(poses)
        _lib.check(self.lib.cslam_pgo_retract_dev(poses.data_ptr(), delta.data_ptr(), poses.shape[0], out.data_ptr(), None))
        return out

    def cost(self, poses, w):
        c = C.c_double(0.0)
        _lib.check(self.lib.cslam_pgo_cost_dev(poses.data_ptr(), self.meas.data_ptr(), self.sig.data_ptr(), w.data_ptr(), self.E.data_ptr(),
                                               C.byref(c), None))
        return c.value

    def weights(self, E, mu, barc2, known=None):
        w = self.torch.empty_like(E)
        _lib.check(self.lib.cslam_pgo_weights_dev(E.data_ptr(), E.shape[0], float(mu), float(barc2),
                                                  known.data_ptr() if known is not None else None, w.data_ptr(), None))
        return w

    def lm(self, x, w, P, trace, counters):
        lam = P["lambda0"]
        c = self.cost(x, w)
        it, stop = 0, False
        while it < P["max_iter"] and not stop:
            self.linearize(x, w)
            c_acc = c
            while True:
                delta, status, predicted = self.solve(lam)
                counters["solves"] += 1
                accept, ratio = False, float("nan")
                if status == 0 and predicted > 0.0:
                    trial = self.retract(x, delta)
                    c_new = self.cost(trial, w)
                    ratio = (c - c_new) / predicted
                    accept = ratio > P["fidelity"]
                elif status != 0:
                    counters["status"] = status
                trace.append((accept, ratio))
                if accept:
                    x, c_acc = trial, c_new
                    lam /= P["factor"]
                    break
                lam *= P["factor"]
                if lam > P["lambda_max"]:
                    stop = True
                    break
            if stop:
                break
            it += 1
            decrease = c - c_acc
            if decrease < P["abs_tol"] or decrease / c < P["rel_tol"]:
                stop = True
            c = c_acc
        counters["lm_iterations"] += it
        counters["lam"] = lam
        return x, c


def optimize_staged(values, edges, prior=None, known_inliers=None, return_trace=False, **params):
    """optimize() driven from Python through the staged entries: the same launches in the same order, so the same bits."""
    pr = Problem(values, edges, prior, known_inliers)
    P = _params(params)
    st = Staged(pr)
    torch = st.torch
    nfac = pr.nf + 1
    w = torch.ones(nfac, dtype=torch.float64, device="cuda")
    trace, cnt = [], dict(solves=0, lm_iterations=0, status=0, lam=0.0)
    x, cost = st.lm(st.dev(pr.poses), w, P, trace, cnt)
    rounds = 0
    st.cost(x, w)
    E = st.E.cpu().numpy()
    free = np.ones(nfac, dtype=bool) if pr.known is None else pr.known == 0
    r = float(np.max(E[free] / P["barc2"])) if free.any() else -1.0
    hw = np.ones(nfac)
    if r >= 0.0 and 2.0 * r - 1.0 > 0.0:
        mu, prev = max(1.0 / (2.0 * r - 1.0), MU_FLOOR), cost
        for _ in range(int(P["gnc_max_rounds"])):
            st.cost(x, w)
            w = st.weights(st.E, mu, P["barc2"], st.known)
            hw = w.cpu().numpy()
            x, cost = st.lm(x, w, P, trace, cnt)
            rounds += 1
            if np.all((np.abs(hw) <= P["weights_tol"]) | (np.abs(hw - 1.0) <= P["weights_tol"])):
                break
            if abs(cost - prev) / max(prev, 1e-7) < P["gnc_cost_tol"]:
                break
            prev = cost
            mu *= P["mu_step"]
    info = [rounds, cnt["lm_iterations"], cnt["solves"], cost, cnt["lam"], cnt["status"], st.info["junctions"], st.info["segments"]]
    res = _result(pr, x.cpu().numpy(), hw, info)
    return (res, trace) if return_trace else res


# ---- g2o (host only): the files the reference's logger writes (src/back_end/utils/logger.cpp:89,96, gtsam::writeG2o) ----------------
_INFO_DIAG = (0, 6, 11, 15, 18, 20)       # positions of the diagonal in the 21 upper-triangular entries
_GRAPH_CHAR, _ROBOT_BASE = ord("g"), ord("A")


def _key_to_id(key):
    """gtsam::LabeledSymbol('g', 'A' + robot_id, keyframe_id) as the reference builds it."""
    return (_GRAPH_CHAR << 56) | ((_ROBOT_BASE + int(key[0])) << 48) | int(key[1])


def _id_to_key(i):
    i = int(i)
    return (((i >> 48) & 0xFF) - _ROBOT_BASE, i & ((1 << 48) - 1)) if i >> 48 else (0, i)


def write_g2o(path, values, edges):
    """VERTEX_SE3:QUAT and EDGE_SE3:QUAT lines; the information matrix is diag(1 / noise_std^2) in g2o's order (translation
    first)."""
    with open(path, "w") as f:
        for key in sorted(values):
            T = as_pose(values[key])
            f.write("VERTEX_SE3:QUAT %d %s\n" % (_key_to_id(key), " ".join(repr(float(x)) for x in list(T[:3, 3]) + list(rot_to_quat(T[:3, :3])))))
        for e in edges:
            kf, kt, meas, std = _edge(e)
            T = as_pose(meas)
            std = np.asarray(std, dtype=np.float64)
            diag = 1.0 / np.concatenate([std[3:], std[:3]]) ** 2
            info = np.zeros(21)
            info[list(_INFO_DIAG)] = diag
            f.write("EDGE_SE3:QUAT %d %d %s %s\n" % (_key_to_id(kf), _key_to_id(kt),
                                                     " ".join(repr(float(x)) for x in list(T[:3, 3]) + list(rot_to_quat(T[:3, :3]))),
                                                     " ".join(repr(float(x)) for x in info)))


def read_g2o(path):
    """-> (values {key: 4 x 4}, [PoseGraphEdge]).  Where an edge's information matrix is not diagonal, ONLY ITS DIAGONAL IS
    TAKEN (noise_std = 1 / sqrt(diagonal), reordered to rotation first): the back end's noise model is diagonal."""
    values, edges = {}, []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "VERTEX_SE3:QUAT":
                values[_id_to_key(tok[1])] = as_pose([float(x) for x in tok[2:9]])
            elif tok[0] == "EDGE_SE3:QUAT":
                info = np.array([float(x) for x in tok[10:31]])
                diag = info[list(_INFO_DIAG)]
                std = 1.0 / np.sqrt(np.concatenate([diag[3:], diag[:3]]))
                edges.append(PoseGraphEdge(_id_to_key(tok[1]), _id_to_key(tok[2]), as_pose([float(x) for x in tok[3:10]]), std))
    return values, edges
