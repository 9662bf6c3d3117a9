"""The robust coarse fit of matched lidar points (csrc/robust.hip): TEASER++'s algorithm at the reference's parameters
(icp_utils.py:68-83,116-121) -- the consistency graph of the matches, its exact maximum clique, GNC-TLS for the rotation
and per-axis TLS for the translation -- as one batched call (`robust_fit_pairs`) and stage by stage."""
import numpy as np

from .. import _lib
from ._batch import gpu, host, offsets, rows, stream, to_dev, upload

ROBUST_MAX_N = 8192            # most correspondences of a pair the robust fit attempts (csrc/robust.hip); above it: status 2
ROBUST_GRAPH_BLOCK = 64        # rows of the consistency graph per workgroup
ROBUST_GRAPH_CHUNK = 256       # matched points per LDS chunk of the graph kernel; the tests size around it
ROBUST_STACK_DEPTH = 512       # deepest branch of the clique search below a root; deeper ends the search uncertified
ROBUST_DEFAULT_NODE_BUDGET = 2097152     # nodes of one pair's clique search (CSLAM_ROBUST_DEFAULT_NODE_BUDGET)


def matched_points(pairs):
    """Matched points of a list of pairs: (ms [total, 3], md [total, 3], offsets).  A pair is (src_points, dst_points)
    with row k of one matched to row k of the other."""
    ms, md = [], []
    for a, b in pairs:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, 3))
        if a.shape != b.shape:
            raise ValueError("matched points come in pairs: %s source rows, %s target rows" % (a.shape, b.shape))
        ms.append(a)
        md.append(b)
    cat = lambda xs: np.concatenate(xs, axis=0) if xs else np.zeros((0, 3))
    return cat(ms), cat(md), offsets([len(a) for a in ms])


def noise(noise_bound):
    c = float(noise_bound)
    if not (np.isfinite(c) and c > 0):
        raise _lib.CslamHipError("invalid argument: noise_bound must be positive and finite")
    return c


def budget_of(node_budget):
    b = int(node_budget)
    if b < 1:
        raise _lib.CslamHipError("invalid argument: node_budget must be at least 1")
    return b


def used(off):
    """The correspondences the stages use per pair (0 above the cap) and the word offsets of the bit matrices."""
    n = np.diff(off)
    n = np.where(n > ROBUST_MAX_N, 0, n)
    return n, offsets(n * ((n + 63) // 64))


def consistency_graph_pairs(pairs, noise_bound, device=0):
    """The consistency graphs of a list of (matched source points, matched target points) in ONE call
    (`cslam_robust_graph_dev`): per pair (adj [N, ceil(N / 64)] uint64, deg [N] int32).  Matches i and j are joined iff
    the distance between the two source points and that between the two target points differ by 2 noise_bound at most.
    Bit j of row i is bit j % 64 of word j // 64.  A pair of more than ROBUST_MAX_N rows gets an empty result."""
    c = noise(noise_bound)
    ms, md, off = matched_points(pairs)
    with gpu(device) as (lib, dev):
        import torch
        n, words = used(off)
        if len(pairs) == 0:
            return []
        t_ms, t_md, t_off = to_dev(ms, dev), to_dev(md, dev), to_dev(off, dev)
        t_adj = torch.zeros(max(int(words[-1]), 1), dtype=torch.int64, device=dev)
        t_adj_off = torch.zeros(len(off), dtype=torch.int64, device=dev)
        t_deg = torch.zeros(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_graph_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), None, len(pairs), c, t_adj.data_ptr(),
                                              t_adj_off.data_ptr(), t_deg.data_ptr(), host(off), None, stream()))
        adj, deg, adj_off = t_adj.cpu().numpy().view(np.uint64), t_deg.cpu().numpy(), t_adj_off.cpu().numpy()
    assert np.array_equal(adj_off, words)
    return [(adj[words[p]:words[p + 1]].reshape(int(n[p]), -1).copy() if n[p] else np.zeros((0, 0), np.uint64),
             deg[off[p]:off[p] + n[p]].copy()) for p in range(len(pairs))]


def consistency_graph(src_points, dst_points, noise_bound, device=0):
    return consistency_graph_pairs([(src_points, dst_points)], noise_bound, device)[0]


def max_clique_graphs(graphs, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """The maximum cliques of a list of bit matrices (as `consistency_graph` returns them) in ONE call
    (`cslam_robust_clique_dev`): per graph (clique: ascending int64 indices, certified, nodes).  The search is exact;
    `certified` is False when `node_budget` nodes did not finish it (or a branch went deeper than ROBUST_STACK_DEPTH below
    its root): the clique is then the best found, never smaller than the greedy one.  Of equal cliques the greedy one wins,
    then the first that the search of the lowest root in the (core number, index) order meets."""
    budget = budget_of(node_budget)
    graphs = [np.ascontiguousarray(g, dtype=np.uint64) for g in graphs]
    for g in graphs:
        if g.ndim != 2 or g.shape[1] != (g.shape[0] + 63) // 64 or g.shape[0] > ROBUST_MAX_N:
            raise ValueError("a graph is an [N <= %d, ceil(N / 64)] uint64 bit matrix, got shape %s" % (ROBUST_MAX_N, g.shape))
    with gpu(device) as (lib, dev):
        import torch
        if not graphs:
            return []
        npairs = len(graphs)
        off = offsets([len(g) for g in graphs])
        n, words = used(off)
        adj = np.concatenate([g.reshape(-1) for g in graphs]) if words[-1] else np.zeros(1, np.uint64)
        deg = np.concatenate([np.unpackbits(g.view(np.uint8).reshape(len(g), 8 * g.shape[1]), axis=1).sum(axis=1, dtype=np.int32) for g in graphs])
        t_adj, t_words, t_deg, t_off = to_dev(adj.view(np.int64), dev), to_dev(words, dev), to_dev(deg.astype(np.int32), dev), to_dev(off, dev)
        t_clique = torch.zeros(max(int(off[-1]), 1), dtype=torch.int32, device=dev)
        t_small = torch.zeros((2, npairs), dtype=torch.int32, device=dev)
        t_nodes = torch.zeros(npairs, dtype=torch.int64, device=dev)
        _lib.check(lib.cslam_robust_clique_dev(t_adj.data_ptr(), t_words.data_ptr(), t_deg.data_ptr(), t_off.data_ptr(), None, npairs, budget,
                                               t_clique.data_ptr(), t_small[0].data_ptr(), t_small[1].data_ptr(), t_nodes.data_ptr(),
                                               host(off), None, stream()))
        clique, small, nodes = t_clique.cpu().numpy(), t_small.cpu().numpy(), t_nodes.cpu().numpy()
    return [(clique[off[p]:off[p] + small[0, p]].astype(np.int64), bool(small[1, p]), int(nodes[p])) for p in range(npairs)]


def max_clique(graph, node_budget=ROBUST_DEFAULT_NODE_BUDGET, return_info=False, device=0):
    """The maximum clique of one bit matrix: ascending indices; with `return_info` (clique, certified, nodes)."""
    out = max_clique_graphs([graph], node_budget, device)[0]
    return out if return_info else out[0]


def _index_lists(cliques, off):
    """Per-pair index lists in the capacity layout (None = all rows in order): (int32 [total], sizes int32 [n])."""
    total = int(off[-1])
    flat = np.zeros(max(total, 1), dtype=np.int32)
    sizes = np.zeros(len(off) - 1, dtype=np.int32)
    for p in range(len(off) - 1):
        cap = int(off[p + 1] - off[p])
        q = np.arange(cap) if cliques is None or cliques[p] is None else np.asarray(cliques[p], dtype=np.int64).reshape(-1)
        if len(q) > cap or (len(q) and (q.min() < 0 or q.max() >= cap)):
            raise ValueError("an index list addresses rows outside its pair")
        flat[off[p]:off[p] + len(q)] = q
        sizes[p] = len(q)
    return flat, sizes


def robust_rotation_pairs(pairs, noise_bound, cliques=None, device=0):
    """GNC-TLS rotations of a list of (matched source points, matched target points) in ONE call
    (`cslam_robust_rotation_dev`), each on the chain of its index list (`cliques[p]`, None = every row in order): per pair
    (R [3, 3], weights [K - 1], iterations)."""
    c = noise(noise_bound)
    ms, md, off = matched_points(pairs)
    flat, sizes = _index_lists(cliques, off)
    with gpu(device) as (lib, dev):
        import torch
        if not pairs:
            return []
        npairs = len(pairs)
        t_ms, t_md, t_off, t_q, t_k = to_dev(ms, dev), to_dev(md, dev), to_dev(off, dev), to_dev(flat, dev), to_dev(sizes, dev)
        t_R = torch.zeros((npairs, 9), dtype=torch.float64, device=dev)
        t_w = torch.zeros(len(flat), dtype=torch.float64, device=dev)
        t_it = torch.zeros(npairs, dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_rotation_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), t_q.data_ptr(), t_k.data_ptr(), npairs,
                                                 c, t_R.data_ptr(), t_w.data_ptr(), t_it.data_ptr(), host(off), stream()))
        R, w, it = t_R.cpu().numpy(), t_w.cpu().numpy(), t_it.cpu().numpy()
    return [(R[p].reshape(3, 3).copy(), w[off[p]:off[p] + max(int(sizes[p]) - 1, 0)].copy(), int(it[p])) for p in range(npairs)]


def robust_rotation(src_points, dst_points, noise_bound, clique=None, device=0):
    return robust_rotation_pairs([(src_points, dst_points)], noise_bound, [clique], device)[0]


def robust_translation_pairs(pairs, rotations, noise_bound, cliques=None, device=0):
    """Per-axis TLS translations of a list of (matched source points, matched target points) under the given rotations in
    ONE call (`cslam_robust_translation_dev`): per pair (t [3], sets [3, K] bool: the consensus set of each axis)."""
    c = noise(noise_bound)
    ms, md, off = matched_points(pairs)
    flat, sizes = _index_lists(cliques, off)
    if len(rotations) != len(pairs):
        raise ValueError("%d rotations for %d pairs" % (len(rotations), len(pairs)))
    R = np.stack([np.asarray(r, dtype=np.float64).reshape(9) for r in rotations]) if pairs else np.zeros((0, 9))
    with gpu(device) as (lib, dev):
        import torch
        if not pairs:
            return []
        npairs, total = len(pairs), max(int(off[-1]), 1)
        t_ms, t_md, t_off, t_q, t_k, t_R = (to_dev(x, dev) for x in (ms, md, off, flat, sizes, R))
        t_t = torch.zeros((npairs, 3), dtype=torch.float64, device=dev)
        t_set = torch.zeros((3, total), dtype=torch.int32, device=dev)
        _lib.check(lib.cslam_robust_translation_dev(t_ms.data_ptr(), t_md.data_ptr(), t_off.data_ptr(), t_q.data_ptr(), t_k.data_ptr(),
                                                    t_R.data_ptr(), npairs, c, t_t.data_ptr(), t_set.data_ptr() if off[-1] else None,
                                                    host(off), stream()))
        t, sets = t_t.cpu().numpy(), t_set.cpu().numpy()
    return [(t[p].copy(), sets[:, off[p]:off[p] + sizes[p]].astype(bool)) for p in range(npairs)]


def robust_translation(src_points, dst_points, rotation, noise_bound, clique=None, device=0):
    return robust_translation_pairs([(src_points, dst_points)], [rotation], noise_bound, [clique], device)[0]


class RobustFit:
    """The robust fit of one pair: `transformation` (4 x 4, source -> target), `status` (0 solved; 1 fewer than 3 clique
    members: the identity, never a fit; 2 more than ROBUST_MAX_N correspondences: not attempted), `clique` (ascending
    correspondence indices), `clique_size`, `iterations` of the rotation, `certified`, `nodes` of the clique search and
    `correspondences` given."""

    def __init__(self, transformation, status, clique, clique_size, iterations, certified, nodes, correspondences):
        self.transformation = transformation
        self.status = status
        self.clique = clique
        self.clique_size = clique_size
        self.iterations = iterations
        self.certified = certified
        self.nodes = nodes
        self.correspondences = correspondences

    def __repr__(self):
        return "RobustFit(status=%d, clique_size=%d of %d, iterations=%d, certified=%s, nodes=%d)" % (
            self.status, self.clique_size, self.correspondences, self.iterations, self.certified, self.nodes)


def fit_enqueue(lib, a, b, p_rows, p_row_off, p_count, c, budget, row_off, h_count):
    """`cslam_robust_fit_dev` on uploaded sources `a` and targets `b` and device pointers to the correspondence rows, their
    offsets and their counts (`row_off`, `h_count`: the same on the host, None = not known there): device (T [n, 16],
    info [n, 6], clique [total rows])."""
    import torch
    n, dev = len(a.off) - 1, a.buf.device
    t_T = torch.zeros((n, 16), dtype=torch.float64, device=dev)
    t_info = torch.zeros((n, 6), dtype=torch.int64, device=dev)
    t_clique = torch.zeros(max(int(row_off[-1]), 1), dtype=torch.int32, device=dev)
    _lib.check(lib.cslam_robust_fit_dev(a.rows, a.d_off, b.rows, b.d_off, p_rows, p_row_off, p_count, n, c, budget, t_T.data_ptr(),
                                        t_info.data_ptr(), t_clique.data_ptr(), host(row_off),
                                        host(h_count) if h_count is not None else None, stream()))
    return t_T, t_info, t_clique


def fits(T, info, clique, row_off):
    """`RobustFit`s of the downloaded results of `fit_enqueue`."""
    return [RobustFit(T[p].reshape(4, 4).copy(), int(info[p, 0]), clique[row_off[p]:row_off[p] + info[p, 1]].astype(np.int64),
                      int(info[p, 1]), int(info[p, 2]), bool(info[p, 3]), int(info[p, 4]), int(info[p, 5])) for p in range(len(T))]


def robust_fit_pairs(pairs, noise_bound, node_budget=ROBUST_DEFAULT_NODE_BUDGET, device=0):
    """The robust fit (consistency graph, maximum clique, GNC-TLS rotation, per-axis TLS translation: TEASER++ with the
    reference's parameters, icp_utils.py:68-83,116-121) for a list of pairs in ONE batched call (`cslam_robust_fit_dev`).
    A pair is (matched source points, matched target points), or (source cloud, target cloud, rows) with rows [N, 2] =
    (source row, target row) as `find_correspondences` gives them.  Returns one `RobustFit` per pair."""
    c, budget = noise(noise_bound), budget_of(node_budget)
    srcs, dsts, corr = [], [], []
    for pr in pairs:
        a, b = rows(pr[0]), rows(pr[1])
        if len(pr) == 2:
            if a.shape != b.shape:
                raise ValueError("matched points come in pairs: %s source rows, %s target rows" % (a.shape, b.shape))
            r = np.repeat(np.arange(len(a), dtype=np.int32)[:, None], 2, axis=1)
        else:
            r = np.asarray(pr[2])
            r = (np.stack(r, axis=1) if isinstance(pr[2], tuple) else r).astype(np.int32).reshape(-1, 2)
        srcs.append(a)
        dsts.append(b)
        corr.append(r)
    with gpu(device) as (lib, dev):
        if not srcs:
            return []
        r_off = offsets([len(r) for r in corr])
        count = np.diff(r_off).astype(np.int32)
        _, a, b = upload(srcs + dsts, dev, pairs=True)
        t_rows, t_ro, t_cnt = to_dev(np.concatenate(corr), dev), to_dev(r_off, dev), to_dev(count, dev)
        t_T, t_info, t_clique = fit_enqueue(lib, a, b, t_rows.data_ptr(), t_ro.data_ptr(), t_cnt.data_ptr(), c, budget, r_off, count)
        T, info, clique = t_T.cpu().numpy(), t_info.cpu().numpy(), t_clique.cpu().numpy()
    return fits(T, info, clique, r_off)
