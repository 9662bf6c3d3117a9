"""Float64 restatement of the rules of csrc/robust.hip (a helper for the robust-fit tests, not a test): the consistency
graph, the maximum clique, GNC-TLS on the chain, per-axis TLS and the chained fit, as include/cslam_hip.h states them.

Neither TEASER++ nor its source is available where these tests run, so parity with TEASER++ itself is not pinned; this
file follows the algorithm that the reference's `get_teaser_solver` parameters select (cslam/lidar_pr/icp_utils.py:68-83).
Two clique searches: `max_cliques`, a small exact one of its own (Bron-Kerbosch with a pivot on Python ints used as
bitsets) that lists every maximum clique, and `clique_search`, the header's branch and bound restated rule by rule, which
says WHICH of them the library returns, index for index.
Also here: the generators of the tests and the measures of how close an input comes to a decision that rounding could turn.
"""
import functools

import numpy as np

import fpfh_reference as fref
import icp_reference as iref

MAX_N = 8192
GNC_FACTOR = 1.4
GNC_MAX_ITER = 10000
GNC_COST_TOL = 1e-16


# ---- (a) the consistency graph ----------------------------------------------------------------------------------------
def pair_lengths(pts):
    """[N, N] distances sqrt(dz dz + (dy dy + dx dx)), the order of the kernels' fma chain."""
    d = pts[None, :, :] - pts[:, None, :]
    return np.sqrt(d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0]))


def consistency_graph(ms, md, c, return_margin=False):
    """[N, N] bool: an edge iff | |md_j - md_i| - |ms_j - ms_i| | <= 2 c, no loops.  With `return_margin` also the
    smallest | |b - a| - 2 c | / (2 c) over the pairs i < j (inf for N < 2)."""
    ms, md = np.asarray(ms, dtype=np.float64).reshape(-1, 3), np.asarray(md, dtype=np.float64).reshape(-1, 3)
    diff = np.abs(pair_lengths(md) - pair_lengths(ms))
    adj = diff <= 2.0 * c
    np.fill_diagonal(adj, False)
    if not return_margin:
        return adj
    iu = np.triu_indices(len(ms), 1)
    return adj, (float(np.abs(diff[iu] - 2.0 * c).min() / (2.0 * c)) if len(iu[0]) else np.inf)


def to_words(adj):
    """The bit matrix of the library: [N, ceil(N / 64)] uint64, bit j of row i = bit j % 64 of word j // 64."""
    n = len(adj)
    w = (n + 63) // 64
    if n == 0:
        return np.zeros((0, 0), dtype=np.uint64)
    padded = np.zeros((n, 64 * w), dtype=bool)
    padded[:, :n] = adj
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(n, w)


def from_words(words, n):
    return np.array([[(int(words[i, j // 64]) >> (j % 64)) & 1 for j in range(n)] for i in range(n)], dtype=bool).reshape(n, n)


# ---- (b) the maximum clique -------------------------------------------------------------------------------------------
def _rows_as_ints(adj):
    """Row i as an int whose bit j is adj[i, j]."""
    packed = np.packbits(np.asarray(adj, dtype=bool), axis=1, bitorder="little")
    return [int.from_bytes(row.tobytes(), "little") for row in packed]


def _bits(x):
    while x:
        low = x & -x
        yield low.bit_length() - 1
        x ^= low


def max_cliques(adj):
    """(size, list of ALL maximum cliques as ascending lists): Bron-Kerbosch with a pivot, a branch cut when it cannot
    reach the best size so far."""
    nb = _rows_as_ints(adj)
    n = len(nb)
    best = [0, []]

    def expand(R, P, X):
        if not P and not X:
            if len(R) > best[0]:
                best[0], best[1] = len(R), [sorted(R)]
            elif len(R) == best[0]:
                best[1].append(sorted(R))
            return
        if len(R) + bin(P).count("1") < best[0]:
            return
        pivot = max(_bits(P | X), key=lambda u: bin(P & nb[u]).count("1"))
        for v in _bits(P & ~nb[pivot]):
            expand(R + [v], P & nb[v], X & nb[v])
            P &= ~(1 << v)
            X |= 1 << v

    if n:
        expand([], (1 << n) - 1, 0)
    return best[0], best[1]


def max_clique(adj):
    """One maximum clique (ascending indices) and whether it is the only one."""
    size, cliques = max_cliques(adj)
    return (cliques[0] if cliques else []), len(cliques) == 1


def is_clique(adj, members):
    m = np.asarray(members, dtype=np.int64)
    sub = np.asarray(adj, dtype=bool)[np.ix_(m, m)]
    return len(set(m.tolist())) == len(m) and bool((sub | np.eye(len(m), dtype=bool)).all())


def core_numbers(adj):
    """Core number of every vertex: peel the vertex of smallest remaining degree again and again; the core number is the
    largest degree seen at a removal so far."""
    adj = np.asarray(adj, dtype=bool)
    deg = adj.sum(axis=1).astype(np.int64)
    alive = np.ones(len(adj), dtype=bool)
    core = np.zeros(len(adj), dtype=np.int64)
    k = 0
    for _ in range(len(adj)):
        v = int(np.where(alive, deg, np.iinfo(np.int64).max).argmin())
        k = max(k, int(deg[v]))
        core[v] = k
        alive[v] = False
        deg[adj[v] & alive] -= 1
    return core


def greedy_clique(adj, core=None):
    """The lower bound of the search: the vertex of largest core number (the lowest index of equals), then again and
    again the same choice among the common neighbours of those taken.  `core`: the core numbers, where they are at hand."""
    adj = np.asarray(adj, dtype=bool)
    core = core_numbers(adj) if core is None else core
    cand = np.ones(len(adj), dtype=bool)
    out = []
    while cand.any():
        v = int(np.where(cand, core, -1).argmax())                   # argmax takes the first of equals
        out.append(v)
        cand &= adj[v]
    return sorted(out)


def search_order(adj, core=None):
    """The order of the search: the original indices in ascending (core number, index)."""
    core = core_numbers(adj) if core is None else core
    return np.lexsort((np.arange(len(core)), core))


def _colour(nb, P, kmin):
    """The members of P (a bitset of order positions) whose greedy colour exceeds kmin.  The colouring takes P in ascending
    position, class by class: a class is the lowest member left and, again and again, the lowest one left that is adjacent
    to none of the class so far.  Once kmin classes are full every member still left has a colour above kmin."""
    if kmin <= 0:
        return P
    q, k = P, 0
    while q:
        k += 1
        if k > kmin:
            return q
        c = q
        while c:
            low = c & -c
            c &= ~(nb[low.bit_length() - 1] | low)
            q ^= low
    return 0


def clique_search(adj, stack_depth=512, core=None):
    """The clique that `cslam_robust_clique_dev` returns, by the rules of include/cslam_hip.h alone:
    (clique as ascending original indices, certified, nodes).

    Vertices are relabelled by `search_order`; g = the size of `greedy_clique`.  Roots go from the top of the order down
    to the first whose core number + 1 is no more than g.  A root starts at own = g with R = [root] and P = its neighbours
    later in the order.  At a node: an empty P records R when |R| > own (strictly: the first clique of a size stays) and
    own becomes |R|; otherwise B = the members of P whose colour exceeds own - |R| (`_colour`; all of P when that is not
    positive), fixed when the node is entered, and the members of B are branched on in ascending position, each leaving P
    before its branch.  The winner is the largest clique recorded, of equal ones that of the lowest root, and the greedy
    clique when no root beat g.  A push that would bring the depth below the root to `stack_depth` ends the whole search
    uncertified: the answer is then the best clique recorded until there.
    `nodes` counts every node entered with every such root searched.  The library also skips a root whose core number + 1
    is below a size that another root has found already, so it reports this count or fewer.  `core`: the core numbers,
    where they are at hand."""
    adj = np.asarray(adj, dtype=bool)
    n = len(adj)
    if n == 0:
        return [], True, 0
    core = core_numbers(adj) if core is None else core
    order = search_order(adj, core)
    greedy = greedy_clique(adj, core)
    g = len(greedy)
    nb = _rows_as_ints(adj[np.ix_(order, order)])
    top = core[order]
    best_size, best, nodes, certified = g, None, 0, True
    for root in range(n - 1, -1, -1):
        if top[root] + 1 <= g or not certified:
            break
        own, found = g, None
        R, saved = [root], []                                        # saved[d] = (P, B) of the node at depth d
        P, B, enter = (nb[root] >> (root + 1)) << (root + 1), 0, True
        while True:
            if enter:
                nodes += 1
                enter = False
                if not P:
                    B = 0
                    if len(R) > own:
                        own, found = len(R), list(R)
                else:
                    B = _colour(nb, P, own - len(R))
            if not B:
                if not saved:
                    break
                P, B = saved.pop()
                R.pop()
                continue
            low = B & -B
            P ^= low
            B ^= low
            if len(R) >= stack_depth:                                # R holds the root and (depth below it) members
                certified = False
                break
            saved.append((P, B))
            P &= nb[low.bit_length() - 1]
            R.append(low.bit_length() - 1)
            enter = True
        if own >= best_size and found is not None:                   # a lower root wins among equal sizes
            best_size, best = own, found
    return (greedy if best is None else sorted(int(order[v]) for v in best)), certified, nodes


# ---- (c) rotation: GNC-TLS on the chain -------------------------------------------------------------------------------
def horn_rotation(a, b, w):
    """argmax over proper rotations of sum w_k b_k . (R a_k): the eigenvector of the largest eigenvalue of Horn's 4 x 4."""
    M = (a * w[:, None]).T @ b                                       # M[x][y] = sum w a_x b_y
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]])
    _, vec = np.linalg.eigh(N)
    qw, x, y, z = vec[:, -1] / np.linalg.norm(vec[:, -1])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - qw * z), 2 * (x * z + qw * y)],
                     [2 * (x * y + qw * z), 1 - 2 * (x * x + z * z), 2 * (y * z - qw * x)],
                     [2 * (x * z - qw * y), 2 * (y * z + qw * x), 1 - 2 * (x * x + y * y)]])


def chain(ms, md, q):
    q = np.asarray(q, dtype=np.int64)
    return ms[q[1:]] - ms[q[:-1]], md[q[1:]] - md[q[:-1]]


def gnc_rotation(ms, md, q, c, return_trace=False):
    """(R, weights, iterations): `iterations` = the weight updates made (0 when the loop stops at mu <= 0).  With
    `return_trace` also a dict of margins: `band` = the smallest relative distance of an r2 from th1 or th2 over all
    iterations, `costs` = the |cost - prev| of every iteration that reached the test."""
    ms, md = np.asarray(ms, dtype=np.float64), np.asarray(md, dtype=np.float64)
    if len(q) < 2:
        out = (np.identity(3), np.zeros(0), 0)
        return out + ({"band": np.inf, "costs": []},) if return_trace else out
    a, b = chain(ms, md, q)
    nb2 = 4.0 * c * c
    if nb2 < 1e-16:
        nb2 = 1e-2
    w = np.ones(len(a))
    mu, prev, iterations = 1.0, np.inf, 0
    trace = {"band": np.inf, "costs": []}
    R = np.identity(3)
    for it in range(GNC_MAX_ITER):
        R = horn_rotation(a, b, w)
        r = b - a @ R.T
        r2 = (r * r).sum(axis=1)
        if it == 0:
            with np.errstate(divide="ignore"):
                mu = 1.0 / (2.0 * r2.max() / nb2 - 1.0)
            if mu <= 0:
                break
        th1, th2 = (mu + 1.0) / mu * nb2, mu / (mu + 1.0) * nb2
        cost = float((w * r2).sum())
        trace["band"] = min(trace["band"], float(np.abs(r2 - th1).min() / th1), float(np.abs(r2 - th2).min() / th2))
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(nb2 * mu * (mu + 1.0) / r2) - mu
        w = np.where(r2 >= th1, 0.0, np.where(r2 <= th2, 1.0, mid))
        iterations = it + 1
        d = abs(cost - prev)
        trace["costs"].append(d)
        mu *= GNC_FACTOR
        prev = cost
        if d < GNC_COST_TOL:
            break
    return (R, w, iterations, trace) if return_trace else (R, w, iterations)


# ---- (d) translation: per-axis TLS ------------------------------------------------------------------------------------
def scalar_tls(x, c, return_margin=False):
    """(estimate, consensus set [K] bool) of the scalars x with the range c for every one of them.  With `return_margin`
    also how far the result is from a decision that rounding could turn: the smaller of (the distance of an x_k from the
    edge of the winning interval) / c and (the cost of the best centre with ANOTHER consensus set - the winning cost) / c."""
    x = np.asarray(x, dtype=np.float64)
    K = len(x)
    ends = np.sort(np.stack([x - c, x + c], axis=1).reshape(-1))       # equal values are interchangeable
    best, out, centres = np.inf, (0.0, np.zeros(K, dtype=bool)), []
    for m in range(2 * K - 1):
        centre = (ends[m] + ends[m + 1]) * 0.5
        dist = np.abs(x - centre)
        inset = dist <= c
        if not inset.any():
            continue
        total = 0.0
        for v in x[inset]:                                           # in index order
            total += v
        est = total / int(inset.sum())
        res = 0.0
        for v in x[inset]:
            res += (v - est) * (v - est)
        cost = res + c * (K - int(inset.sum()))
        centres.append((cost, inset, float(np.abs(dist - c).min())))
        if cost < best:
            best, out, edge = cost, (est, inset), float(np.abs(dist - c).min())
    if not return_margin:
        return out
    others = [cost for cost, inset, _ in centres if not np.array_equal(inset, out[1])]
    return out + (min(edge / c, (min(others) - best) / c if others else np.inf),)


def translation_scalars(ms, md, q, R):
    q = np.asarray(q, dtype=np.int64)
    s, d = np.asarray(ms, dtype=np.float64)[q], np.asarray(md, dtype=np.float64)[q]
    return np.stack([d[:, a] - ((R[a, 0] * s[:, 0] + R[a, 1] * s[:, 1]) + R[a, 2] * s[:, 2]) for a in range(3)])


def tls_translation(ms, md, q, R, c):
    """(t [3], sets [3, K] bool)."""
    xs = translation_scalars(ms, md, q, R)
    res = [scalar_tls(xs[a], c) for a in range(3)]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- (e) the chained fit ----------------------------------------------------------------------------------------------
class Fit:
    def __init__(self, T, status, clique, iterations, unique):
        self.transformation = T
        self.status = status
        self.clique = clique
        self.clique_size = len(clique)
        self.iterations = iterations
        self.unique = unique


def robust_fit(ms, md, c, clique=None):
    ms, md = np.asarray(ms, dtype=np.float64).reshape(-1, 3), np.asarray(md, dtype=np.float64).reshape(-1, 3)
    if len(ms) > MAX_N:
        return Fit(np.identity(4), 2, [], 0, True)
    unique = True
    if clique is None:
        clique, unique = max_clique(consistency_graph(ms, md, c))
    if len(clique) < 3:
        return Fit(np.identity(4), 1, clique, 0, unique)
    R, _, iterations = gnc_rotation(ms, md, clique, c)
    t, _ = tls_translation(ms, md, clique, R, c)
    return Fit(iref.Rt2T(R, t), 0, clique, iterations, unique)


def transform_error(T, T_true):
    """(rotation error in degrees, translation error in metres)."""
    return iref.rotation_error_deg(T[:3, :3], T_true[:3, :3]), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


# ---- generators ---------------------------------------------------------------------------------------------------------
def planted(seed, n, n_in, noise=0.02):
    """(ms, md, T, inliers): n matched points, the source uniform in +-20 m, the target moved by `fpfh_reference.moved_copy`'s
    transform of this seed with `noise` of Gaussian noise; all but the n_in inliers (ascending indices) then get a random
    target point."""
    rng = np.random.default_rng(7000 + seed)
    ms = rng.uniform(-20.0, 20.0, (n, 3))
    _, T, _ = fref.moved_copy(ms[:1], seed)
    md = ms @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((n, 3))
    inliers = np.sort(rng.permutation(n)[:n_in])
    out = np.setdiff1d(np.arange(n), inliers)
    md[out] = rng.uniform(-20.0, 20.0, (len(out), 3))
    return ms, md, T, inliers


def two_planted(seed, n, n_in):
    """Two disjoint inlier sets of n_in under two different transforms: two maximum cliques of equal size."""
    ms, md, T, first = planted(seed, n, n_in)
    rng = np.random.default_rng(7500 + seed)
    rest = np.setdiff1d(np.arange(n), first)
    second = np.sort(rng.permutation(rest)[:n_in])
    _, T2, _ = fref.moved_copy(ms[:1], seed + 50)
    md[second] = ms[second] @ T2[:3, :3].T + T2[:3, 3] + 0.02 * rng.standard_normal((n_in, 3))
    return ms, md, first, second


def dense_case(seed=3, n=128, noise=0.5):
    """n matches, all under one transform, with `noise` of target noise: at c = noise about half the pairs are consistent."""
    rng = np.random.default_rng(7900 + seed)
    ms = rng.uniform(-20.0, 20.0, (n, 3))
    _, T, _ = fref.moved_copy(ms[:1], seed)
    return ms, ms @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((n, 3))


def gnp_case(seed, n, p):
    """[n, n] bool: every pair an edge with probability p; symmetric, zero diagonal."""
    rng = np.random.default_rng(11000 + seed)
    adj = np.triu(rng.random((n, n), dtype=np.float32) < p, 1)
    return adj | adj.T


def decoy_case(parts, k, seed=None):
    """(adj, planted): a cocktail-party graph on 2 * parts vertices (complete but for the perfect matching (2 i, 2 i + 1);
    its maximum cliques have `parts` members and its core numbers are 2 * parts - 2) beside a disjoint clique of k (core
    numbers k - 1): for parts < k <= 2 * parts - 2 (and one more without a seed: equal core numbers, the decoys have the lower
    indices) the greedy clique sits among the decoys and the planted clique has to be found by the search, k - 1 levels
    below its lowest root.  With a seed the vertices are relabelled by a permutation;
    `planted` = the ascending indices of the clique of k."""
    m = 2 * parts
    adj = np.zeros((m + k, m + k), dtype=bool)
    adj[:m, :m] = True
    i = np.arange(parts)
    adj[2 * i, 2 * i + 1] = adj[2 * i + 1, 2 * i] = False
    adj[m:, m:] = True
    np.fill_diagonal(adj, False)
    at = np.arange(m + k) if seed is None else np.random.default_rng(12000 + seed).permutation(m + k)
    out = np.zeros_like(adj)
    out[np.ix_(at, at)] = adj
    return out, np.sort(at[m:])


def planted_gnp_case(seed, n, p, members):
    """`gnp_case` with a clique planted on the original indices `members`."""
    adj = gnp_case(seed, n, p)
    m = np.asarray(members, dtype=np.int64)
    adj[np.ix_(m, m)] = True
    adj[m, m] = False
    return adj


def backtrack_case(fill=4096):
    """(adj, A, second clique): a graph whose winner is met only after its root has come back from another branch, with
    every set of that search in the second word of a lane (positions from `fill` on; the `fill` vertices below are isolated).
    On the last 46 indices, all of core number 11 and so in index order: a complete bipartite graph on 11 + 11 vertices
    (the greedy clique starts there and ends with 2), then r, d1 .. d10, x1, x2, a1 .. a11, where {r, d1 .. d10} is a
    clique of 11, {d1 .. d10, x1, x2} one of 12 and A = {r, a1 .. a11} one of 12.  Root d1 meets its 12 first; the lower
    root r first goes down d2, d1, ... to the 11, comes back to its own node, and only then goes down a2 to A, which wins
    as the equal clique of the lower root."""
    n = fill + 46
    adj = np.zeros((n, n), dtype=bool)
    idx = lambda a, k: list(range(fill + a, fill + a + k))
    left, right, r, d, x, a = idx(0, 11), idx(11, 11), idx(22, 1), idx(23, 10), idx(33, 2), idx(35, 11)
    adj[np.ix_(left, right)] = True
    adj[np.ix_(right, left)] = True
    for members in (r + d, d + x, r + a):
        adj[np.ix_(members, members)] = True
    np.fill_diagonal(adj, False)
    return adj, r + a, d + x


# The graphs on which the library's clique is compared with `clique_search` index for index.  The CPU tests assert what
# makes them worth it (the greedy clique is too small, several maximum cliques exist, roots lie in both halves of a lane's
# bitset); the GPU tests run the library on them.
FAMILY_SEEDS = (0, 1)
FAMILY = ((1, .5), (2, .5), (3, .5), (63, .5), (64, .5), (65, .5), (129, .3), (129, .5), (100, .7), (70, .9), (200, .2), (257, .1),
          (192, .4))                                                 # (n, p): around one and two words, sparse to dense
WIDE_PLANTED = (0, 63, 64, 4095, 4096, 4097, 4159, 4160, 8127, 8128, 8190, 8191)
WIDE = {"4096/16": (4096, 16), "4097/16": (4097, 16), "8191/16": (8191, 16), "4160/40": (4160, 40), "8192/30": (8192, 30)}     # (n, mean degree)
WIDE_ALL = tuple(WIDE) + ("8192/30+12", "K4097")
MANY = 600


class SearchCase:
    """A graph and what the restatement makes of it: `adj`, `words` (the library's bit matrix), `core`, `greedy`, and
    `clique`, `certified`, `nodes` = clique_search(adj)."""

    def __init__(self, adj, planted=None):
        self.adj, self.planted = adj, planted
        self.words = to_words(adj)
        self.core = core_numbers(adj)
        self.greedy = greedy_clique(adj, self.core)
        self.clique, self.certified, self.nodes = clique_search(adj, core=self.core)

    @property
    def want(self):
        return self.clique, self.certified


@functools.lru_cache(maxsize=None)
def family_case(s, n, p):
    return SearchCase(gnp_case(1000 * s + n, n, p))


def family():
    return [family_case(s, n, p) for s in FAMILY_SEEDS for n, p in FAMILY]


@functools.lru_cache(maxsize=None)
def wide_case(name):
    if name == "K4097":
        return SearchCase(~np.eye(4097, dtype=bool))
    if name == "8192/30+12":
        return SearchCase(planted_gnp_case(1, 8192, 30 / 8192, WIDE_PLANTED), np.array(WIDE_PLANTED))
    n, degree = WIDE[name]
    return SearchCase(gnp_case(n, n, degree / n))


@functools.lru_cache(maxsize=None)
def backtrack_search_case():
    adj, first, second = backtrack_case()
    return SearchCase(adj, np.array(first))


@functools.lru_cache(maxsize=None)
def decoy_search_case(k, seed=None):
    return SearchCase(*decoy_case(500, k, seed))


@functools.lru_cache(maxsize=None)
def wide_pair(c):
    """planted(5, 4200, 40), a pair whose bitsets need both words of a lane: (ms, md, inliers, graph, margin of the graph).
    The point-based graph allocates [N, N, 3] float64 arrays: this is as large as a point case should get."""
    ms, md, _, inliers = planted(5, 4200, 40)
    adj, margin = consistency_graph(ms, md, c, return_margin=True)
    return ms, md, inliers, adj, margin


@functools.lru_cache(maxsize=None)
def many_cases():
    """MANY small graphs: n from 0 .. 40, p from .2, .5 and .8."""
    rng = np.random.default_rng(13000)
    return [SearchCase(gnp_case(20000 + i, int(rng.integers(0, 41)), float(rng.choice([.2, .5, .8])))) for i in range(MANY)]


def lattice_case(n):
    """n matches on a line with exact integer distances, for c = 1: sources at x = 3 k, targets at x = 5 k for even k and
    3 k for odd k.  Two odd matches agree exactly; matches 2 and 3 have a = 3 and b = 1: |b - a| == 2 c, which is an edge;
    matches 2 and 1 have |b - a| = 4: no edge."""
    k = np.arange(n, dtype=np.float64)
    zero = np.zeros(n)
    return np.stack([3.0 * k, zero, zero], axis=1), np.stack([np.where(k % 2 == 0, 5.0 * k, 3.0 * k), zero, zero], axis=1)


ROTATION_CASES = ((2, 0.0, 11), (63, 0.2, 12), (64, 0.4, 13), (65, 0.6, 14), (257, 0.3, 15), (1030, 0.5, 16))


def rotation_case(m, outlier_share, seed, c=0.05):
    """m + 1 matched points whose chain has m measurements: inliers with 1 cm noise, the share of outliers with a random
    target point.  Returns (ms, md, c)."""
    rng = np.random.default_rng(8000 + seed)
    ms = rng.uniform(-20.0, 20.0, (m + 1, 3))
    _, T, _ = fref.moved_copy(ms[:1], seed)
    md = ms @ T[:3, :3].T + T[:3, 3] + 0.01 * rng.standard_normal((m + 1, 3))
    bad = rng.permutation(m + 1)[:int(round(outlier_share * (m + 1)))]
    md[bad] = rng.uniform(-20.0, 20.0, (len(bad), 3))
    return ms, md, c


TRANSLATION_SIZES = (3, 63, 64, 65, 500)


def translation_case(K, seed):
    """(ms, md, R, c): scalars per axis around a true shift with noise well inside c, a fifth of them planted outliers, and
    exact duplicates of some values.  The source is the origin and R the identity, so that x_k = md[k] exactly."""
    rng = np.random.default_rng(9000 + seed)
    c = 0.1
    md = np.array([1.5, -2.25, 0.5]) + 0.03 * rng.uniform(-1.0, 1.0, (K, 3))
    bad = rng.permutation(K)[:K // 5]
    md[bad] += rng.uniform(0.5, 3.0, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))
    if K >= 6:
        md[K // 2] = md[0]                                           # duplicates: equal endpoints
        md[K // 3] = md[1]
    return np.zeros((K, 3)), md, np.identity(3), c


def golden(name):
    """A recorded array of tests/golden, or None where the file is missing."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
    return np.load(path) if os.path.exists(path) else None
