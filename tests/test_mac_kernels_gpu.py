"""Per-kernel tests of the sparsifier's float64 device code (-m gpu): the segmented scans and the chain reduction /
back-substitution, L X, the 4-column block products (csrc/mac_kernels.hip), and both builders of the chain / junction
structure (chain_solver.py and cslam_fiedler in csrc/fiedler.hip).

Three kinds of check:
  1. EXACT: integer-valued inputs in [-8, 8] and chain conductances in {1/4, 1/2, 1, 2} make every partial sum of every
     summation tree exactly representable, so the kernels must return the int64 reference bit for bit.  The builders
     assert the bound that makes this true (sum of |terms| < 2^51 in the finest unit, 1/4).
  2. REAL: standard_normal inputs against the same operation in np.longdouble, within a derived bound: a sum of l terms in
     any order errs by at most l 2^-53 sum|terms|.  A dropped or misplaced element moves a result by about
     sum|terms| / l, orders of magnitude above that.
  3. WHOLE SOLVES on topologies the pose-graph family of test_mac_gpu.py never produces (path, ring, every node a
     junction, no chain edge at all, missing chain edges, stored zeros, duplicate entries), against an `splu` solve
     refined with longdouble residuals, and through `cslam_fiedler` against the sparse-LU TraceMIN oracle.
Junction layouts are written out; no case relies on where a seed happens to put a junction."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNK = 2048                     # SCAN_CHUNK of mac_kernels.hip
LD = np.longdouble


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


# ------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------
def chain_laplacian(n, c, loops, canonical=True):
    """Laplacian (CSR float64) of the chain i -- i+1 with conductances c[i] (0: the edge is absent and not stored) plus the
    loop edges (i, j, w).  canonical=False keeps the entries as given (duplicates, explicit zeros) and sorts nothing."""
    import scipy.sparse as sp
    c = np.asarray(c, dtype=np.float64)
    k = np.flatnonzero(c != 0)
    li = np.array([e[0] for e in loops], dtype=np.int64)
    lj = np.array([e[1] for e in loops], dtype=np.int64)
    lw = np.array([e[2] for e in loops], dtype=np.float64)
    ii = np.concatenate([k, li]); jj = np.concatenate([k + 1, lj]); ww = np.concatenate([c[k], lw])
    rows = np.concatenate([ii, jj, ii, jj]); cols = np.concatenate([ii, jj, jj, ii])
    data = np.concatenate([ww, ww, -ww, -ww])
    if canonical:
        return sp.csr_matrix(sp.coo_matrix((data, (rows, cols)), shape=(n, n)))
    # raw CSR: the diagonal is summed (one entry per row), every off-diagonal entry stays as given
    diag = np.bincount(np.concatenate([ii, jj]), weights=np.concatenate([ww, ww]), minlength=n)
    rows = np.concatenate([np.arange(n), ii, jj]); cols = np.concatenate([np.arange(n), jj, ii])
    data = np.concatenate([diag, -ww, -ww])
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return sp.csr_matrix((data[order], cols[order], indptr), shape=(n, n))


def junction_graph(n, junctions, ground, c, seed=0):
    """Chain of n nodes whose junction set is EXACTLY `junctions` (0 and n-1 belong to it): every junction gets one loop
    edge to `ground` (to node 0 or n-1 when it is the ground's neighbour), which also gives the ground the largest row
    of the Laplacian -- the rule by which both solvers choose the grounded node."""
    J = sorted(set(int(j) for j in junctions) | {0, n - 1, int(ground)})
    rng = np.random.default_rng(seed)
    loops = []
    for j in J:
        if j == ground:
            continue
        far = ground if abs(j - ground) >= 2 else (0 if j >= 2 else n - 1)
        if abs(j - far) >= 2:
            loops.append((min(j, far), max(j, far), float(rng.uniform(0.1, 1.0))))
    L = chain_laplacian(n, c, loops)
    deg = np.diff(L.indptr)
    assert int(deg.argmax()) == ground and (deg == deg.max()).sum() == 1, "the ground is not pinned"
    return L, np.array(J, dtype=np.int64)


def pow2_conductances(n, seed):
    return np.random.default_rng(seed).choice(np.array([0.25, 0.5, 1.0, 2.0]), size=n - 1)


def segment_starts(n, is_j):
    """per node: the junction at or before it"""
    return np.maximum.accumulate(np.where(is_j, np.arange(n), -1))


def int_scan_reference(b, is_j, r4):
    """The two segmented scans of cslam_chain_forward_dev in int64: B (running injection since the last junction, 0 on
    junctions) and Q in units of 1/4 (running sum of r[k-1] B[k-1]); r4 = 4 r.  Asserts that sum|terms| stays under 2^51
    in units of 1/4, which makes every partial sum of any summation order exact in float64."""
    n = b.shape[0]
    start = segment_starts(n, is_j)
    bz = np.where(is_j[:, None], 0, b).astype(np.int64)
    cs = np.cumsum(bz, axis=0)
    B = cs - cs[start]
    t = np.zeros_like(B)
    t[1:] = r4[:, None] * B[:-1]
    t[is_j] = 0
    cq = np.cumsum(t, axis=0)
    Q4 = cq - cq[start]
    ab = np.cumsum(np.abs(bz), axis=0); ab -= ab[start]
    at = np.zeros_like(ab); at[1:] = r4[:, None] * ab[:-1]; at[is_j] = 0
    aq = np.cumsum(at, axis=0); aq -= aq[start]
    assert 4 * int(ab.max()) < 2 ** 51 and int(aq.max()) < 2 ** 51, "inputs no longer exact: shrink the ranges"
    return B, Q4


def int_block(rng, n, cols=4):
    a = rng.integers(-8, 9, size=(n, cols))
    assert n * 4 * 64 * 9 < 2 ** 51                    # sum|terms| of every product below
    return a


# ------------------------------------------------------------------------------------------------
# 1. exact: segmented scans and the reduced right-hand side
# ------------------------------------------------------------------------------------------------
def _aligned_layout():
    """Segments of length 2047, 2048, 2049, 4096 and 4097, each once from a chunk boundary and once from 77 past one."""
    J, want, cur = [], [], 1
    for off in (0, 77):
        for ln in (2047, 2048, 2049, 4096, 4097):
            s = -(-cur // CHUNK) * CHUNK + off
            J += [s, s + ln]; want.append((s, s + ln)); cur = s + ln + 1
    return cur + 10, J, J[3], want


def _big_layout(n):
    """About 50 junctions over n > 2^21 nodes: one segment straddles node 1024 * 2048 (where the carry pass starts its
    second tile of 1024 chunks; at n = 1024 * 2048 + 1 that node is the last one and ends the segment), one is longer
    than three chunks, the rest are spread evenly."""
    last = min(2099000, n - 1)
    J = [100000, 110000, 2090000, last] + [200000 + 39997 * i for i in range(46)]
    assert all(not (2090000 < j < last) and not (100000 < j < 110000) for j in J) and max(J) < n
    return J, 200000 + 39997 * 20, [(100000, 110000), (2090000, last)]


def _scan_layouts():
    n3 = 3 * CHUNK + 5
    na, Ja, ga, wa = _aligned_layout()
    nb1, nb2 = 1024 * CHUNK + 1, 2100000
    Jb1, gb1, wb1 = _big_layout(nb1)
    Jb2, gb2, wb2 = _big_layout(nb2)
    return {
        "n2049_ends_only": (2049, [], 1000, [(0, 1000), (1000, 2048)]),
        "middle_chunk_without_junction": (n3, [2040, 4100], 2040, [(2040, 4100)]),
        "junctions_on_chunk_edges": (n3, [2047, 2048, 4095], 4095, [(2047, 2048), (2048, 4095)]),
        "adjacent_junctions": (n3, [100, 101, 3000, 3001, 3002], 3001, [(100, 101), (3000, 3001), (3001, 3002)]),
        "aligned_lengths": (na, Ja, ga, wa),
        "carry_tile_edge_n2097153": (nb1, Jb1, gb1, wb1),
        "carry_tile_edge_n2100000": (nb2, Jb2, gb2, wb2),
    }


_SCAN_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_cases():
    yield
    _SCAN_CACHE.clear(); _B4_CACHE.clear(); _TOPO.clear()


def _exact_scan_case(name):
    """(solver, inputs, int64 reference) of one layout, after one .solve(): built once per layout and shared."""
    import torch
    from cslam_amd.mac.chain_solver_gpu import ChainReducedSolverGPU
    if name in _SCAN_CACHE:
        return _SCAN_CACHE[name]
    _SCAN_CACHE.clear()                                       # one layout resident at a time (the big ones hold 0.5 GB)
    n, junctions, ground, want = _scan_layouts()[name]
    c = pow2_conductances(n, seed=n)
    L, J = junction_graph(n, junctions, ground, c)
    is_j = np.zeros(n, dtype=bool); is_j[J] = True
    b = int_block(np.random.default_rng(n + 1), n)
    r4 = np.rint(4.0 / c).astype(np.int64)
    B, Q4 = int_scan_reference(b, is_j, r4)
    solver = ChainReducedSolverGPU(L, ground)
    x = solver.solve(_dev(b, np.float64))
    torch.cuda.synchronize()
    case = dict(n=n, J=J, ground=ground, want=want, c=c, r4=r4, b=b, is_j=is_j, B=B, Q4=Q4, solver=solver, x=x, L=L)
    _SCAN_CACHE[name] = case
    return case


@pytest.mark.parametrize("name", list(_scan_layouts()))
def test_segmented_scans_are_exact_on_integer_inputs(name):
    """Bn and Qn of cslam_chain_forward_dev == the int64 segmented cumulative sums, bit for bit; bt within one division
    and three additions of b + Ql/Rl + Bl - Ql/Rl evaluated in longdouble; the host structure is the layout asked for."""
    k = _exact_scan_case(name)
    s, n, J = k["solver"], k["n"], k["J"]
    h = s.host
    assert np.array_equal(h.is_j, k["is_j"]) and np.array_equal(h.J, J) and h.ground == k["ground"]
    segs = set(zip(h.sa.tolist(), h.sb.tolist()))
    assert all(w in segs for w in k["want"]), "a listed segment is cut by a junction"
    assert len(h.sa) == len(J) - 1                           # no chain edge is missing: consecutive junctions are joined
    # the structure's resistances are exact too (multiples of 1/4 well under 2^53)
    rc4 = np.concatenate([[0], np.cumsum(k["r4"])])
    start = segment_starts(n, k["is_j"])
    assert np.array_equal(s.r.cpu().numpy() * 4, k["r4"])
    assert np.array_equal(s.Rn.cpu().numpy() * 4, rc4[np.arange(n)] - rc4[start])
    assert np.array_equal(s.Rl.cpu().numpy() * 4, rc4[h.sb] - rc4[h.sa])
    Bn, Qn = s.Bn.cpu().numpy(), s.Qn.cpu().numpy()
    bad = np.argwhere(Bn != k["B"])
    assert bad.size == 0, f"Bn differs first at node {bad[0]}: {Bn[tuple(bad[0])]} != {k['B'][tuple(bad[0])]}"
    bad = np.argwhere(Qn * 4 != k["Q4"])
    assert bad.size == 0, f"Qn differs first at node {bad[0]}: {Qn[tuple(bad[0])] * 4} != {k['Q4'][tuple(bad[0])]} (x 1/4)"
    assert np.array_equal(Bn, k["B"]) and np.array_equal(Qn * 4, k["Q4"])
    # reduced right-hand side
    e = h.sb - 1
    Ql = (k["Q4"][e] + k["r4"][e][:, None] * k["B"][e]).astype(LD) / 4
    Bl = k["B"][e].astype(LD)
    corr = Ql / (rc4[h.sb] - rc4[h.sa]).astype(LD)[:, None] * 4
    bt = k["b"][J].astype(LD)
    mag = np.abs(bt)
    ja, jb = h.jid[h.sa], h.jid[h.sb]                     # every junction starts / ends at most one segment
    bt[ja] += corr; mag[ja] += np.abs(corr)
    bt[jb] += Bl - corr; mag[jb] += np.abs(Bl) + np.abs(corr)
    err = np.abs(s.bt.cpu().numpy().astype(LD) - bt)
    bound = 4 * U * mag
    print(f"\n[scan {name}] n={n} nJ={len(J)} max|B|={np.abs(k['B']).max()} max|Q|={np.abs(k['Q4']).max() / 4:.3g} "
          f"bt err/bound max={float((err / np.maximum(bound, LD(1e-300))).max()):.3f}")
    assert np.all(err <= bound)


def _back_substitute(s, xJ, out):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    _lib.check(lib.cslam_chain_backward_dev(_vp(xJ), _vp(s.Bn), _vp(s.Qn), _vp(s.r), _vp(s.Rn), _vp(s.jid), _vp(s.seg_of),
                                            _vp(s.sa), _vp(s.sb), _vp(s.Rl), s.n, _vp(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _back_subst_reference(h, r, Rl, Rn, Bn, Qn, xJ):
    """x_k = x_a - f1 R_k - Q_k, f1 = (x_a - x_b - Ql) / Rl in longdouble from the kernel's own inputs; (x, magnitude)."""
    n = h.n
    sidx = h.seg_of_start[h.start]
    k = np.flatnonzero(~h.is_j)
    sg = sidx[k]
    assert np.all(sg >= 0)
    e = h.sb - 1
    Ql = Qn[e].astype(LD) + r[e].astype(LD)[:, None] * Bn[e].astype(LD)
    xa, xb = xJ[h.jid[h.sa[sg]]].astype(LD), xJ[h.jid[h.sb[sg]]].astype(LD)
    f1 = (xa - xb - Ql[sg]) / Rl[sg].astype(LD)[:, None]
    fr = f1 * Rn[k].astype(LD)[:, None]
    x = np.zeros((n, 4), dtype=LD); mag = np.zeros((n, 4), dtype=LD)
    x[k] = xa - fr - Qn[k].astype(LD)
    mag[k] = np.abs(xa) + np.abs(fr) + np.abs(Qn[k].astype(LD))
    x[h.J] = xJ
    return x, mag


def _chosen_xJ(nJ, seed):
    """Junction potentials with 1 <= |x| <= 2 and random signs.  The kernel rounds x_a - x_b, the numerator, the
    quotient, f1 R_k and two subtractions: to first order 2^-53 (3|x_a| + |x_b| R_k/Rl + 5|f1 R_k| + |Q_k|), and with
    |x_b| <= 2|x_a| that is below the 8 2^-53 (|x_a| + |f1 R_k| + |Q_k|) the test allows."""
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, size=(nJ, 4)) * rng.choice([-1.0, 1.0], size=(nJ, 4))


@pytest.mark.parametrize("name", ["junctions_on_chunk_edges", "adjacent_junctions", "aligned_lengths", "carry_tile_edge_n2100000"])
def test_back_substitution_against_longdouble(name):
    import torch
    k = _exact_scan_case(name)
    s, h = k["solver"], k["solver"].host
    xJ = _chosen_xJ(s.nJ, 5)
    out = torch.full((s.n, 4), float("nan"), dtype=torch.float64, device="cuda")
    x = _back_substitute(s, _dev(xJ), out)
    assert np.array_equal(x[h.J], xJ)                       # junction rows are copies
    ref, mag = _back_subst_reference(h, h.r, h.Rl, h.R, k["B"].astype(np.float64), k["Q4"] / 4.0, xJ)
    err = np.abs(x.astype(LD) - ref)
    bound = 8 * U * mag
    inner = ~h.is_j
    print(f"\n[back-subst {name}] max err/bound = {float((err[inner] / bound[inner]).max()):.3f}")
    assert np.all(err[inner] <= bound[inner])


# ------------------------------------------------------------------------------------------------
# 1. exact: block products and L X
# ------------------------------------------------------------------------------------------------
B4_SIZES = [1, 63, 64, 255, 256, 257, 65537, 262144, 262145, 524588]
_B4_CACHE = {}


def _b4_inputs(n):
    if n not in _B4_CACHE:
        _B4_CACHE.clear()
        rng = np.random.default_rng(n)
        A, Bm = int_block(rng, n), int_block(rng, n)
        _B4_CACHE[n] = (A, Bm, _dev(A, np.float64), _dev(Bm, np.float64))
    return _B4_CACHE[n]


def _b4_scratch():
    import torch
    return (torch.full((20 * 1024,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((20,), float("nan"), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("n", B4_SIZES)
def test_block4_gram_is_exact(n):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    A, Bm, dA, dB = _b4_inputs(n)
    ref = np.concatenate([(A.T @ Bm).ravel(), Bm.sum(axis=0)])
    partial, out20 = _b4_scratch()
    _lib.check(lib.cslam_block4_gram_dev(_vp(dA), _vp(dB), n, _vp(partial), _vp(out20), None))
    torch.cuda.synchronize()
    got_dev = out20.cpu().numpy()
    partial, out20 = _b4_scratch()
    h20 = np.full(20, np.nan)
    _lib.check(lib.cslam_block4_gram_sync(_vp(dA), _vp(dB), n, _vp(partial), _vp(out20), _hp(h20), None))
    assert np.array_equal(got_dev, ref), (got_dev - ref)
    assert np.array_equal(h20, ref) and np.array_equal(out20.cpu().numpy(), ref)


@pytest.mark.parametrize("n", B4_SIZES)
def test_block4_residual_is_exact(n):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    W, X, dW, dX = _b4_inputs(n)
    y = np.array([3.0, -7.0, 0.0, 5.0]); sigma = -6.0
    ref = int(np.abs(W @ y.astype(np.int64) - int(sigma) * X[:, 0]).sum())
    partial, out1 = _b4_scratch()
    dy = _dev(y)
    _lib.check(lib.cslam_block4_residual_dev(_vp(dW), _vp(dX), n, _vp(dy), sigma, _vp(partial), _vp(out1), None))
    torch.cuda.synchronize()
    assert float(out1[0]) == ref
    partial, out1 = _b4_scratch()
    h1 = np.full(1, np.nan)
    _lib.check(lib.cslam_block4_residual_sync(_vp(dW), _vp(dX), n, _hp(y), sigma, _vp(partial), _vp(out1), _hp(h1), None))
    assert h1[0] == ref and float(out1[0]) == ref


@pytest.mark.parametrize("n", B4_SIZES)
def test_block4_affine_is_exact(n):
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    A, _, dA, _ = _b4_inputs(n)
    rng = np.random.default_rng(7)
    M, shift = rng.integers(-8, 9, size=(4, 4)), rng.integers(-8, 9, size=4)
    Mf, sf = M.astype(np.float64), shift.astype(np.float64)
    dM, ds = _dev(Mf), _dev(sf)
    for with_shift in (True, False):
        ref = A @ M - (shift if with_shift else 0)
        out = torch.full((n + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.cslam_block4_affine_dev(_vp(dA), n, _vp(dM), _vp(ds) if with_shift else None, _vp(out), None))
        torch.cuda.synchronize()
        assert np.array_equal(out[:n].cpu().numpy(), ref) and bool(out[n].isnan().all())
        out = torch.full((n + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.cslam_block4_affine_host(_vp(dA), n, _hp(Mf), _hp(sf) if with_shift else None, _vp(out), None))
        torch.cuda.synchronize()
        assert np.array_equal(out[:n].cpu().numpy(), ref) and bool(out[n].isnan().all())


def awkward_csr(n, rng, integer):
    """CSR (indptr int64, indices int32, data) with empty rows in the middle and at the end, one hub row holding every
    other column, and column indices in random order within every row (never sorted)."""
    hub = n // 3
    empty = {n // 2, n // 2 + 1, n - 1} - {hub} if n >= 4 else set()
    indptr, indices = [0], []
    for r in range(n):
        if r in empty:
            cols = np.zeros(0, dtype=np.int64)
        elif r == hub and n > 1:
            cols = rng.permutation(np.delete(np.arange(n), r))
        else:
            cols = rng.choice(n, size=min(n, int(rng.integers(1, 7))), replace=False)
        indices.append(cols); indptr.append(indptr[-1] + len(cols))
    indices = np.concatenate(indices).astype(np.int32)
    data = rng.integers(-8, 9, size=len(indices)) if integer else rng.standard_normal(len(indices))
    return np.array(indptr, dtype=np.int64), indices, data


def _spmm_both(indptr, indices, data, X):
    """(cslam_csr_spmm4_dev result [n,4] or None, {nvec: cslam_csr_spmm_dev result [n, nvec]})"""
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    n = len(indptr) - 1
    dp, di, dd, dx = _dev(indptr), _dev(indices), _dev(data, np.float64), _dev(X, np.float64)
    y4 = torch.full((n + 1, 4), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.cslam_csr_spmm4_dev(_vp(dp), _vp(di), _vp(dd), n, _vp(dx), _vp(y4), None))
    torch.cuda.synchronize()
    assert bool(y4[n].isnan().all())
    got = {}
    for nvec in (1, 3, 4):
        xt = _dev(X[:, :nvec].T, np.float64)                 # [nvec][n]
        yt = torch.full((nvec + 1, n), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.cslam_csr_spmm_dev(_vp(dp), _vp(di), _vp(dd), n, _vp(xt), nvec, _vp(yt), None))
        torch.cuda.synchronize()
        assert bool(yt[nvec].isnan().all())
        got[nvec] = yt[:nvec].cpu().numpy().T
    return y4[:n].cpu().numpy(), got


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_csr_products_are_exact(n):
    import scipy.sparse as sp
    rng = np.random.default_rng(n)
    indptr, indices, data = awkward_csr(n, rng, integer=True)
    if n >= 4:
        deg = np.diff(indptr)
        assert deg[n - 1] == 0 and deg[n // 2] == 0 and deg.max() == n - 1
        assert any(np.any(np.diff(indices[indptr[r]:indptr[r + 1]]) < 0) for r in range(n))
    X = int_block(rng, n)
    ref = sp.csr_matrix((data.astype(np.int64), indices, indptr), shape=(n, n)) @ X.astype(np.int64)
    y4, got = _spmm_both(indptr, indices, data, X)
    assert np.array_equal(y4, ref)
    for nvec in (1, 3, 4):
        assert np.array_equal(got[nvec], ref[:, :nvec])


# ------------------------------------------------------------------------------------------------
# 2. real-valued inputs against longdouble, derived bounds
# ------------------------------------------------------------------------------------------------
def _loguniform(rng, size, lo=0.1, hi=10.0):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))


def test_chain_kernels_on_real_inputs_against_longdouble():
    """cslam_chain_forward_dev and cslam_chain_backward_dev with standard_normal right-hand sides and conductances
    log-uniform in [0.1, 10], each stage against longdouble on that stage's OWN inputs (r, Rl, Rn as the solver holds
    them; Q from the device's t = r B): scans within l 2^-53 sum|terms| (l = segment length), t within one rounding, bt
    and the back-substitution within the bounds of the exact tests."""
    import torch
    from cslam_amd.mac.chain_solver_gpu import ChainReducedSolverGPU
    n = 3 * CHUNK + 5
    rng = np.random.default_rng(42)
    c = _loguniform(rng, n - 1)
    L, J = junction_graph(n, [2047, 2048, 2500, 2501, 4095, 4300], 2500, c)
    s = ChainReducedSolverGPU(L, 2500)
    h = s.host
    b = rng.standard_normal((n, 4))
    s.solve(_dev(b))
    torch.cuda.synchronize()
    Bn, Qn, t = s.Bn.cpu().numpy(), s.Qn.cpu().numpy(), s.tmp.cpu().numpy()
    is_j, start = h.is_j, h.start
    nxt = np.minimum.accumulate(np.where(is_j, np.arange(n), n)[::-1])[::-1]
    seglen = (np.where(is_j, 1, nxt - start))[:, None].astype(LD)

    def seg_cumsum(v):                                        # segment by segment: a global cumsum would cancel
        out = np.zeros(v.shape, dtype=LD)
        for a, e in zip(J[:-1], J[1:]):
            out[a + 1:e] = np.cumsum(v[a + 1:e], axis=0)
        return out
    refB, absB = seg_cumsum(b.astype(LD)), seg_cumsum(np.abs(b).astype(LD))
    eB = np.abs(Bn.astype(LD) - refB)
    assert np.all(eB <= seglen * U * absB) and np.all(Bn[is_j] == 0)
    t_ref = np.zeros((n, 4), dtype=LD)
    t_ref[1:] = h.r.astype(LD)[:, None] * Bn[:-1].astype(LD)
    assert np.all(np.abs(t.astype(LD) - t_ref) <= U * np.abs(t_ref))
    refQ, absQ = seg_cumsum(t.astype(LD)), seg_cumsum(np.abs(t).astype(LD))
    eQ = np.abs(Qn.astype(LD) - refQ)
    assert np.all(eQ <= seglen * U * absQ) and np.all(Qn[is_j] == 0)
    # reduced right-hand side from the device's own Bn, Qn
    e = h.sb - 1
    Ql = np.where((e > h.sa)[:, None], Qn[e], 0.0).astype(LD) + h.r[e].astype(LD)[:, None] * Bn[e].astype(LD)
    corr = Ql / h.Rl.astype(LD)[:, None]
    bt = b[J].astype(LD); mag = np.abs(bt)
    ja, jb = h.jid[h.sa], h.jid[h.sb]
    bt[ja] += corr; mag[ja] += np.abs(corr)
    bt[jb] += Bn[e].astype(LD) - corr; mag[jb] += np.abs(Bn[e]).astype(LD) + np.abs(corr)
    ebt = np.abs(s.bt.cpu().numpy().astype(LD) - bt)
    # Ql itself is a rounded product and sum here (not exact integers): two more roundings on |Ql| / Rl
    assert np.all(ebt <= 6 * U * mag)
    xJ = _chosen_xJ(s.nJ, 9)
    out = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    x = _back_substitute(s, _dev(xJ), out)
    ref, xmag = _back_subst_reference(h, h.r, h.Rl, h.R, Bn, Qn, xJ)
    inner = ~is_j
    ex = np.abs(x.astype(LD) - ref)
    # as in the exact test, plus the two roundings of Ql = Qn[e] + r[e] Bl, which reach x_k scaled by R_k / Rl <= 1
    e_k = h.sb[h.seg_of_start[start]] - 1
    Qlmag = (np.abs(Qn[e_k]) + np.abs(h.r[np.minimum(e_k, n - 2)][:, None] * Bn[e_k])).astype(LD)
    bound = 8 * U * xmag + 2 * U * Qlmag
    assert np.array_equal(x[J], xJ) and np.all(ex[inner] <= bound[inner])
    print(f"\n[real chain] err/bound max: Bn {float((eB[inner] / (seglen * U * absB)[inner]).max()):.3f} "
          f"Qn {float(np.nanmax(eQ[inner] / np.maximum((seglen * U * absQ)[inner], LD(1e-300)))):.3f} "
          f"bt {float((ebt / (6 * U * mag)).max()):.3f} x {float((ex[inner] / bound[inner]).max()):.3f}")


@pytest.mark.parametrize("n", [257, 262145])
def test_block_products_on_real_inputs_against_longdouble(n):
    """gram within n 2^-53 sum|a_i b_j|; residual within (n + 5) 2^-53 sum(|W_k| |y| + |sigma X_k0|) (each term is a 4-term
    dot and a difference: 5 roundings, then a sum of n terms); affine within 5 2^-53 (|a| |M| + |shift|)."""
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(n)
    A, Bm = rng.standard_normal((n, 4)), rng.standard_normal((n, 4))
    dA, dB = _dev(A), _dev(Bm)
    Al, Bl = A.astype(LD), Bm.astype(LD)
    partial, out20 = _b4_scratch()
    h20 = np.full(20, np.nan)
    _lib.check(lib.cslam_block4_gram_sync(_vp(dA), _vp(dB), n, _vp(partial), _vp(out20), _hp(h20), None))
    ref = np.concatenate([(Al.T @ Bl).ravel(), Bl.sum(axis=0)])
    mag = np.concatenate([(np.abs(Al).T @ np.abs(Bl)).ravel(), np.abs(Bl).sum(axis=0)])
    eg = np.abs(h20.astype(LD) - ref)
    gram_ratio = float((eg / (n * U * mag)).max())
    assert np.all(eg <= n * U * mag)
    partial2, out20b = _b4_scratch()
    _lib.check(lib.cslam_block4_gram_dev(_vp(dA), _vp(dB), n, _vp(partial2), _vp(out20b), None))
    torch.cuda.synchronize()
    assert np.array_equal(out20b.cpu().numpy(), h20)        # the two forms run the same kernels
    y = rng.standard_normal(4); sigma = 0.37
    ref = np.abs(Al @ y.astype(LD) - LD(sigma) * Bl[:, 0]).sum()
    mag = (np.abs(Al) @ np.abs(y).astype(LD) + abs(sigma) * np.abs(Bl[:, 0])).sum()
    h1 = np.full(1, np.nan)
    dy = _dev(y)
    _lib.check(lib.cslam_block4_residual_sync(_vp(dA), _vp(dB), n, _hp(y), sigma, _vp(partial), _vp(out20), _hp(h1), None))
    _lib.check(lib.cslam_block4_residual_dev(_vp(dA), _vp(dB), n, _vp(dy), sigma, _vp(partial), _vp(out20), None))
    torch.cuda.synchronize()
    er = [abs(LD(h1[0]) - ref), abs(LD(float(out20[0])) - ref)]
    assert max(er) <= (n + 5) * U * mag
    M, shift = rng.standard_normal((4, 4)), rng.standard_normal(4)
    ref = Al @ M.astype(LD) - shift.astype(LD)
    mag = np.abs(Al) @ np.abs(M).astype(LD) + np.abs(shift).astype(LD)
    ea = []
    dM, ds = _dev(M), _dev(shift)
    for host in (False, True):
        out = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
        if host:
            _lib.check(lib.cslam_block4_affine_host(_vp(dA), n, _hp(M), _hp(shift), _vp(out), None))
        else:
            _lib.check(lib.cslam_block4_affine_dev(_vp(dA), n, _vp(dM), _vp(ds), _vp(out), None))
        torch.cuda.synchronize()
        ea.append(np.abs(out.cpu().numpy().astype(LD) - ref))
        assert np.all(ea[-1] <= 5 * U * mag)
    print(f"\n[real block4 n={n}] err/bound max: gram {gram_ratio:.2e} affine {float(max((e / (5 * U * mag)).max() for e in ea)):.3f}")


def test_csr_products_on_real_inputs_against_longdouble():
    """Row r within l_r 2^-53 sum|a| |x| (l_r stored entries: l_r products and l_r - 1 additions, each rounded once)."""
    n = 5000
    rng = np.random.default_rng(3)
    indptr, indices, data = awkward_csr(n, rng, integer=False)
    X = rng.standard_normal((n, 4))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    ref = np.zeros((n, 4), dtype=LD); mag = np.zeros((n, 4), dtype=LD)
    prod = data.astype(LD)[:, None] * X[indices].astype(LD)
    np.add.at(ref, rows, prod); np.add.at(mag, rows, np.abs(prod))
    bound = np.diff(indptr)[:, None].astype(LD) * U * mag
    y4, got = _spmm_both(indptr, indices, data, X)
    assert np.all(np.abs(y4.astype(LD) - ref) <= bound)
    for nvec in (1, 3, 4):
        assert np.all(np.abs(got[nvec].astype(LD) - ref[:, :nvec]) <= bound[:, :nvec])


# ------------------------------------------------------------------------------------------------
# 3. whole solves and Fiedler pairs on the topologies the pose-graph family leaves out
# ------------------------------------------------------------------------------------------------
def _topologies():
    """name -> (Laplacian handed to the solvers, canonical Laplacian for the references, expectations)"""
    out = {}
    rng = np.random.default_rng(2024)

    def add(name, n, c, loops, raw=False, **expect):
        Lc = chain_laplacian(n, c, loops)
        out[name] = (chain_laplacian(n, c, loops, canonical=False) if raw else Lc, Lc, expect)
    n = 513
    add("path", n, _loguniform(rng, n - 1), [], nseg=2)
    # a ring of near-uniform conductances has lambda_2 ~ lambda_3: one weak stretch separates them
    n = 700
    c = _loguniform(rng, n - 1, 0.5, 2.0); c[300:340] *= 0.2
    add("ring", n, c, [(0, n - 1, 1.7)])
    n = 257
    add("every_node_a_junction", n, _loguniform(rng, n - 1),
        [(i, i + 2, float(w)) for i, w in zip(range(n - 2), _loguniform(rng, n - 2))], nJ=n, nseg=n - 1)
    n = 301
    add("no_chain_edge_at_all", n, np.zeros(n - 1),
        [(i, i + 2, float(w)) for i, w in zip(range(n - 2), _loguniform(rng, n - 2))] +
        [(i, i + 3, float(w)) for i, w in zip(range(0, n - 3, 5), _loguniform(rng, n))], nJ=n, nseg=0)
    P = 1100
    c = _loguniform(rng, 2 * P - 1); c[P - 1] = 0.0
    add("two_robots_no_chain_edge_between", 2 * P, c, [(40, P + 700, 0.8), (900, P + 3, 1.3), (P - 1, 2 * P - 1, 0.4)])
    n = 3000
    c = _loguniform(rng, n - 1); c[1499] = 0.0
    add("chain_edge_missing_inside_a_robot", n, c, [(100, 2900, 0.6), (1400, 1600, 2.5), (700, 2200, 0.3)])
    n = 2500
    add("stored_zero_loop_entry", n, _loguniform(rng, n - 1), [(10, 2000, 0.7), (500, 1500, 0.0), (1000, 2400, 1.9)],
        raw=True, nJ=6)
    n = CHUNK + 3
    add("duplicate_entries", n, _loguniform(rng, n - 1), [(5, 1500, 0.25), (5, 1500, 0.5), (300, 2047, 1.1), (300, 2047, 1.1)],
        raw=True, nJ=6)
    n = 3 * CHUNK + 5
    add("loguniform_chain_6149", n, _loguniform(rng, n - 1),
        [(0, 3000, 2.3), (n - 1, 1000, 0.6), (2047, 4096, 0.9), (2048, 5000, 3.1), (700, 4095, 0.2), (1999, 6000, 5.0)])
    return out


_TOPO = {}


def _topology(name):
    if not _TOPO:
        _TOPO.update(_topologies())
    return _TOPO[name]


_TOPO_NAMES = ["path", "ring", "every_node_a_junction", "no_chain_edge_at_all", "two_robots_no_chain_edge_between",
               "chain_edge_missing_inside_a_robot", "stored_zero_loop_entry", "duplicate_entries", "loguniform_chain_6149"]


def ld_matvec(L, x):
    """L @ x in longdouble (L canonical CSR float64, x [n, q] longdouble)"""
    rows = np.repeat(np.arange(L.shape[0]), np.diff(L.indptr))
    y = np.zeros(x.shape, dtype=LD)
    np.add.at(y, rows, L.data.astype(LD)[:, None] * x[L.indices])
    return y


def refined_grounded_solve(L, g, B):
    """(refined x, plain float64 splu x): the grounded Laplacian through SuperLU, then three steps of iterative refinement
    with the residual in longdouble.  Knows nothing of chains or junctions."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    n = L.shape[0]
    keep = np.delete(np.arange(n), g)
    A = sp.csc_matrix(L[keep][:, keep])
    lu = spla.splu(A)
    Ac = sp.csr_matrix(A); Ac.sum_duplicates()
    x0 = lu.solve(np.ascontiguousarray(B[keep]))
    x = x0.astype(LD)
    for _ in range(3):
        res = B[keep].astype(LD) - ld_matvec(Ac, x)
        x = x + lu.solve(np.ascontiguousarray(res.astype(np.float64))).astype(LD)
    res = B[keep].astype(LD) - ld_matvec(Ac, x)
    full = np.zeros((n, B.shape[1]), dtype=LD); full[keep] = x
    plain = np.zeros((n, B.shape[1])); plain[keep] = x0
    return full, plain, float(np.abs(res).max())


@pytest.mark.parametrize("name", _TOPO_NAMES)
def test_whole_solve_on_unusual_topologies(name):
    """ChainReducedSolverGPU.solve within 8 x the larger forward error of the two float64 CPU solvers (plain splu, the host
    chain solver) against the refined reference, floor 1e-9 max|x| (the bound of test_chain_solver_gpu_matches_host): the
    GPU runs the host chain solver's algorithm with other summation orders and a dense junction factor."""
    import torch
    from cslam_amd.mac.chain_solver import ChainReducedSolver
    from cslam_amd.mac.chain_solver_gpu import ChainReducedSolverGPU
    L, Lc, expect = _topology(name)
    n = L.shape[0]
    g = int(np.diff(Lc.indptr).argmax())
    B = np.random.default_rng(1).standard_normal((n, 4))
    ref, x_lu, refined_res = refined_grounded_solve(Lc, g, B)
    host = ChainReducedSolver(L.copy(), g)
    x_host = host.solve(B)
    s = ChainReducedSolverGPU(L.copy(), g)
    if "nJ" in expect:
        assert s.nJ == expect["nJ"]
    if "nseg" in expect:
        assert len(s.host.sa) == expect["nseg"]
    x_gpu = s.solve(torch.from_numpy(B).cuda()).cpu().numpy()
    scale = float(np.abs(ref).max())
    e_lu, e_host, e_gpu = (float(np.abs(v.astype(LD) - ref).max()) for v in (x_lu, x_host, x_gpu))
    tol = max(8 * max(e_lu, e_host), 1e-9 * scale)
    print(f"\n[solve {name}] n={n} nJ={s.nJ} nseg={len(s.host.sa)} refined residual {refined_res:.1e} | forward error / max|x|: "
          f"splu {e_lu / scale:.2e}  host chain {e_host / scale:.2e}  GPU {e_gpu / scale:.2e}  (allowed {tol / scale:.2e})")
    assert refined_res < 1e-11 * max(1.0, float(np.abs(B).max()))
    assert np.all(x_gpu[g] == 0) and e_gpu <= tol


@pytest.mark.parametrize("name", _TOPO_NAMES)
def test_one_call_fiedler_on_unusual_topologies(name):
    """cslam_fiedler builds the chain / junction structure a second time, in C++: same graphs, against the sparse-LU
    TraceMIN oracle with the numbers of test_one_call_c_abi_fiedler_matches_reference_algorithm."""
    from cslam_amd.mac.chain_solver_gpu import fiedler_tracemin_hip
    from oracle.fiedler_oracle import fiedler_tracemin_lu
    L, Lc, _ = _topology(name)
    l1, v1 = fiedler_tracemin_lu(Lc)
    l2, v2 = fiedler_tracemin_hip(L.copy())
    res = np.linalg.norm(Lc @ v2 - l2 * v2, 1) / abs(Lc).sum(axis=1).max()
    dv = min(np.max(np.abs(v1 - v2)), np.max(np.abs(v1 + v2)))
    print(f"\n[fiedler {name}] lambda2 {l2:.12e} (oracle {l1:.12e})  |dv| {dv:.2e}  residual {res:.2e}")
    assert abs(l1 - l2) < 1e-9 * abs(l1) + 1e-13
    assert res < 1e-8
    assert abs(np.linalg.norm(v2) - 1.0) < 1e-12 and abs(v2.sum()) < 1e-9
    assert dv < 1e-6


def test_one_call_fiedler_reports_disconnected_variants():
    from cslam_amd._lib import CslamGraphError
    from cslam_amd.mac.chain_solver_gpu import fiedler_tracemin_hip
    rng = np.random.default_rng(8)
    n = 513
    c = _loguniform(rng, n - 1); c[200] = 0.0                          # the path with one chain edge removed
    with pytest.raises(CslamGraphError, match="not connected"):
        fiedler_tracemin_hip(chain_laplacian(n, c, []))
    c = _loguniform(rng, n - 1); c[100] = 0.0; c[400] = 0.0             # the ring cut twice
    with pytest.raises(CslamGraphError, match="not connected"):
        fiedler_tracemin_hip(chain_laplacian(n, c, [(0, n - 1, 1.0)]))
    c[400] = 1.0                                                        # cut once it is a path again
    lam, v = fiedler_tracemin_hip(chain_laplacian(n, c, [(0, n - 1, 1.0)]))
    assert lam > 0 and abs(np.linalg.norm(v) - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------
# 5. argument checks: refused (or accepted as empty) without a launch
# ------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    import torch
    from cslam_amd import _lib
    lib = _lib.load()
    n = 300
    S = 77.0
    f = lambda *shape: torch.full(shape, S, dtype=torch.float64, device="cuda")
    A, Bm, out, partial, out20 = f(n, 4), f(n, 4), f(n, 4), f(20 * 1024), f(20)
    M, sh, y = f(16), f(4), f(4)
    hM, hs, hy, h20, h1 = np.full(16, S), np.full(4, S), np.full(4, S), np.full(20, S), np.full(1, S)
    p = _vp
    E = -1
    # n = 0
    assert lib.cslam_block4_gram_dev(p(A), p(Bm), 0, p(partial), p(out20), None) == E
    assert lib.cslam_block4_gram_sync(p(A), p(Bm), 0, p(partial), p(out20), _hp(h20), None) == E
    assert lib.cslam_block4_affine_dev(p(A), 0, p(M), p(sh), p(out), None) == E
    assert lib.cslam_block4_affine_host(p(A), 0, _hp(hM), _hp(hs), p(out), None) == E
    assert lib.cslam_block4_residual_dev(p(A), p(Bm), 0, p(y), 1.0, p(partial), p(out20), None) == E
    assert lib.cslam_block4_residual_sync(p(A), p(Bm), 0, _hp(hy), 1.0, p(partial), p(out20), _hp(h1), None) == E
    assert b"invalid argument" in lib.cslam_last_error()
    # NULL pointers, one at a time
    for i in range(5):
        a = [p(A), p(Bm), n, p(partial), p(out20)]
        if i != 2:
            a[i] = None
            assert lib.cslam_block4_gram_dev(*a, None) == E
            assert lib.cslam_block4_gram_sync(*a, _hp(h20), None) == E
    assert lib.cslam_block4_gram_sync(p(A), p(Bm), n, p(partial), p(out20), None, None) == E
    for a in ([None, n, p(M), p(sh), p(out)], [p(A), n, None, p(sh), p(out)], [p(A), n, p(M), p(sh), None]):
        assert lib.cslam_block4_affine_dev(*a, None) == E
    for a in ([None, n, _hp(hM), _hp(hs), p(out)], [p(A), n, None, _hp(hs), p(out)], [p(A), n, _hp(hM), _hp(hs), None]):
        assert lib.cslam_block4_affine_host(*a, None) == E
    for i in (0, 1, 3, 5, 6):
        a = [p(A), p(Bm), n, p(y), 1.0, p(partial), p(out20)]
        a[i] = None
        assert lib.cslam_block4_residual_dev(*a, None) == E
        a[3] = _hp(hy) if i != 3 else None
        assert lib.cslam_block4_residual_sync(*a, _hp(h1), None) == E
    assert lib.cslam_block4_residual_sync(p(A), p(Bm), n, _hp(hy), 1.0, p(partial), p(out20), None, None) == E
    # chain forward: n < 2, nJ < 1
    isj = torch.ones(n, dtype=torch.uint8, device="cuda")
    i64 = torch.zeros(n, dtype=torch.int64, device="cuda")
    i32 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    Bn, Qn, tmp, scratch, bt = f(n, 4), f(n, 4), f(n, 4), f(128), f(n, 4)
    fw = lambda nn, nJ: lib.cslam_chain_forward_dev(p(A), p(isj), p(sh), nn, p(i64), nJ, p(i32), p(i32), p(i64), p(i64), p(sh),
                                                    p(Bn), p(Qn), p(tmp), p(scratch), p(bt), None)
    assert fw(1, 1) == E and fw(0, 1) == E and fw(n, 0) == E and fw(n, -1) == E
    # empty sizes are accepted and launch nothing
    g = f(n)
    ip = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ix = torch.zeros(n, dtype=torch.int32, device="cuda")
    assert lib.cslam_csr_spmm4_dev(p(ip), p(ix), p(sh), 0, p(A), p(out), None) == 0
    assert lib.cslam_mac_grad_dev(p(sh), p(ix), p(ix), p(sh), 0, p(g), None) == 0
    assert lib.cslam_csr_spmm4_dev(p(ip), p(ix), p(sh), -1, p(A), p(out), None) == E
    assert lib.cslam_mac_grad_dev(p(sh), p(ix), p(ix), p(sh), -1, p(g), None) == E
    torch.cuda.synchronize()
    for t in (out, partial, out20, Bn, Qn, tmp, scratch, bt, g):
        assert int((t != S).sum()) == 0                          # nothing was launched
    assert np.all(h20 == S) and np.all(h1 == S)
    # and the same buffers do work with valid arguments
    assert lib.cslam_block4_gram_sync(p(A), p(Bm), n, p(partial), p(out20), _hp(h20), None) == 0
    assert np.array_equal(h20, np.concatenate([np.full(16, n * S * S), np.full(4, n * S)]))
