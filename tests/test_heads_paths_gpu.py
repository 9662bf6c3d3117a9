"""GPU tests (-m gpu) of every kernel path of the descriptor heads against float64, at derived tolerances (tests/heads_reference.py;
the conditions on the cases are proved without a device in tests/test_heads_reference_cpu.py).

VLAD (heads.hip, cslam_vlad_aggregate_dev / _nhwc_dev / _nhwc_pairs_dev): the five paths `generic`, `split`, `fast`, `fast_nhwc`,
`matrix` at their tile edges, on gaussian and on trunk-like maps; err(got, vlad_f64) <= tol = 4 err(vlad_seq32, vlad_f64), the
float32 layer with the longest chains as the yardstick.  Every case prints err(got), the yardstick and their ratio.
Float32 projection (gemm_nt.hip, cslam_pca_project_dev): integer operands on which every partial sum is exact, so only the epilogue
rounds: |out - ref| <= (Dout / 2 + 4) u |ref|.  Row normalisation (cslam_l2_normalize_dev): ((ceil(d / 256) + 10) / 2 + 4) u |ref|.

Largest err(got) / err(vlad_seq32) per path, measured on an MI355X (gaussian kind | trunk kind; the margin is 4):
    generic    0.49 | 1.62   at (2, 31, 300)
    split      0.40 | 1.62   at (3, 33, 17) | (8, 500, 255)
    fast       0.32 | 0.84   at (9, 33, 17)
    fast_nhwc  0.32 | 0.84   at (9, 33, 17)
    matrix     0.20 | 0.54   at (9, 128, 32); with the pair store 0.41 | 0.55 at (1, 128, 33)
The kernels sum in shorter chains than the yardstick and stay below it, but for the steep softmax in the two paths whose logits are
one chain over all channels.  At C = 1 the float32 layer is exact (yardstick 0) and the kernels, which multiply by a rounded
reciprocal where the layer divides, are off by 2^-24 on the gaussian kind: there the yardstick is the restatement with their
normalisations (heads_reference.vlad_case), which gives the same 2^-24.
Measured on the CPU: the yardstick is 4.2e-7 .. 4.1e-6 on the gaussian kind and 6.8e-7 .. 7.2e-5 on the trunk kind over the cases of
the table (C > 1); the smallest planted defect is 43 tolerances (the assignment sum missing one of 255 pixels at C = 500).
"""
import ctypes as C

import numpy as np
import pytest

import heads_reference as hr

pytestmark = pytest.mark.gpu

K = hr.K
SENTINEL = 0x7FC0DEAD                 # a NaN bit pattern no kernel computes
CASES = hr.all_vlad_cases()
CASE_IDS = ["%s-%dx%dx%d" % ((p,) + c) for p, c in CASES]


@pytest.fixture(scope="module")
def T():
    import torch
    from cslam_amd import _lib
    from cslam_amd.vpr import heads
    return torch, heads, _lib.load()


def dev(T, a):
    return T[0].from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached cases are read-only


def stream(T):
    return C.c_void_p(T[0].cuda.current_stream().cuda_stream)


def sentinel_rows(T, n, pitch):
    torch = T[0]
    return torch.full((n, pitch), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def keeps_sentinel(T, t):
    return bool((t.contiguous().view(T[0].int32) == SENTINEL).all())


def same_bytes(T, a, b):
    return a.shape == b.shape and T[0].equal(a.contiguous().view(T[0].int32), b.contiguous().view(T[0].int32))


def run_vlad(T, x, w, b, cent, channels_last, pad=0):
    """x [B,C,P] numpy -> [B, 64 C] device rows through the C entry point of the layout (the map as [B,P,C] when channels_last);
    pad > 0: the rows are a view of a [B, 64 C + pad] buffer of sentinels, returned as well."""
    torch, _, lib = T
    B, Cc, P = x.shape
    feat = dev(T, x.transpose(0, 2, 1) if channels_last else x)
    buf = sentinel_rows(T, B, K * Cc + pad)
    dw, db, dc = dev(T, w), (dev(T, b) if b is not None else None), dev(T, cent)
    fn = lib.cslam_vlad_aggregate_nhwc_dev if channels_last else lib.cslam_vlad_aggregate_dev
    rc = fn(feat.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None, dc.data_ptr(), B, Cc, P, K,
            buf.data_ptr(), buf.stride(0), stream(T))
    assert rc == 0, lib.cslam_last_error()
    torch.cuda.synchronize()
    out = buf[:, :K * Cc]
    return (out, buf) if pad else out


def check_rows(got, d, rows=None):
    """-> (err, message or None): finite, within the case's tolerance of float64, unit rows"""
    ref = d["ref"] if rows is None else d["ref"][rows]
    g = got.cpu().numpy().astype(np.float64)
    if not np.all(np.isfinite(g)):
        return float("inf"), "not finite"
    e = hr.err(g, ref)
    if not e <= d["tol"]:
        return e, "err %.3g > tol %.3g" % (e, d["tol"])
    nrm = np.abs(np.linalg.norm(g, axis=1) - 1.0).max()
    if not nrm <= d["tol"] * np.sqrt(g.shape[1]):
        return e, "row norm off by %.3g > %.3g" % (nrm, d["tol"] * np.sqrt(g.shape[1]))
    return e, None


# --------------------------------------------------------------------------------------------------------------------- VLAD ----
@pytest.mark.parametrize("path,case", CASES, ids=CASE_IDS)
def test_vlad_paths_against_float64(T, path, case):
    """Every case of the table, both kinds, NCHW and (B > 8, P <= 256) channels-last."""
    B, Cc, P = case
    bad = []
    for kind in hr.KINDS:
        d = hr.vlad_case(B, Cc, P, kind)
        for cl, runs in hr.vlad_layouts(path, case):
            got = run_vlad(T, d["x"], d["w"], d["b"], d["cent"], cl)
            e, msg = check_rows(got, d)
            print("vlad %-9s %-5s %-4s B=%d C=%d P=%d: err %.3g yardstick %.3g ratio %.2f" % (
                runs, kind, "nhwc" if cl else "nchw", B, Cc, P, e, d["yard"], e / d["yard"] if d["yard"] else float("inf")))
            if msg:
                bad.append("%s %s %s: %s" % (runs, kind, "nhwc" if cl else "nchw", msg))
    assert not bad, bad


@pytest.mark.parametrize("case,hw", [((1, 128, 33), (3, 11)), ((3, 384, 200), (10, 20))])
def test_vlad_pair_store(T, case, hw):
    """cslam_vlad_aggregate_nhwc_pairs_dev with 1, 8 and 64 splits: the float32 rows within the tolerance, the pair rows byte-equal
    to pca_pairs_rows_kernel's arithmetic (test_head_floor_gpu.pair_rows) on those rows, with and without the float32 rows."""
    import test_head_floor_gpu as hf
    torch, heads, _ = T
    B, Cc, P = case
    bad = []
    for kind in hr.KINDS:
        d = hr.vlad_case(B, Cc, P, kind)
        xl = dev(T, d["x"].reshape(B, Cc, *hw)).contiguous(memory_format=torch.channels_last)
        args = (dev(T, d["w"]), dev(T, d["b"]) if d["b"] is not None else None, dev(T, d["cent"]))
        for S in (1, 8, 64):
            a2, v = heads.vlad_aggregate_pairs(xl, *args, splits=S, keep_v=True)
            e, msg = check_rows(v, d)
            print("vlad pairs     %-5s S=%-2d B=%d C=%d P=%d: err %.3g yardstick %.3g ratio %.2f" % (kind, S, B, Cc, P, e, d["yard"], e / d["yard"]))
            if msg:
                bad.append("%s S=%d: %s" % (kind, S, msg))
            want = hf.pair_rows(torch, v.contiguous(), heads.VLAD_BOUND, S)
            assert a2.shape == want.shape and torch.equal(a2.view(torch.int16), want.view(torch.int16)), (kind, S)
            a2_only, none = heads.vlad_aggregate_pairs(xl, *args, splits=S)
            assert none is None and torch.equal(a2_only.view(torch.int16), a2.view(torch.int16)), (kind, S)
    assert not bad, bad


def test_vlad_eight_images_against_nine(T):
    """Images 0..7 of a nine-image batch given alone run the split path, the nine the batch kernel: both within the tolerance
    (not bit-equal: other partial sums)."""
    bad = []
    for kind in hr.KINDS:
        d = hr.vlad_case(9, 500, 255, kind)
        for n in (9, 8):
            assert hr.vlad_path(n, 500, 255, False) == ("fast" if n == 9 else "split")
            got = run_vlad(T, d["x"][:n], d["w"], d["b"], d["cent"], False)
            e, msg = check_rows(got[:8], d, slice(0, 8))
            print("vlad %d images %-5s: err %.3g yardstick %.3g" % (n, kind, e, d["yard"]))
            if msg:
                bad.append("%s B=%d: %s" % (kind, n, msg))
    assert not bad, bad


def test_vlad_wrapper_converts_a_small_channels_last_batch(T):
    """heads.vlad_aggregate: a channels-last map of eight images is no input of the batch kernels; the wrapper converts it, and
    the rows are those of the NCHW call byte for byte."""
    torch, heads, _ = T
    d = hr.vlad_case(8, 500, 255, "gauss")
    x4 = dev(T, d["x"].reshape(8, 500, 15, 17))
    xl = x4.contiguous(memory_format=torch.channels_last)
    assert not xl.is_contiguous() and hr.vlad_path(8, 500, 255, True) == "split"
    args = (dev(T, d["w"]), dev(T, d["b"]), dev(T, d["cent"]))
    a, b = heads.vlad_aggregate(xl, *args), heads.vlad_aggregate(x4, *args)
    assert same_bytes(T, a, b)
    assert check_rows(a, d)[1] is None


@pytest.mark.parametrize("path,case,cl", [("fast", (9, 33, 17), False), ("fast_nhwc", (9, 33, 17), True),
                                          ("matrix", (9, 256, 33), True), ("generic", (9, 33, 384), False)])
def test_vlad_row_does_not_depend_on_its_place_in_the_batch(T, path, case, cl):
    """One image as frame 0 and as frame 8 of two batches of nine: the same bytes."""
    B, Cc, P = case
    assert hr.vlad_path(B, Cc, P, cl) == path
    d = hr.vlad_case(B, Cc, P, "trunk")
    first, last = d["x"].copy(), d["x"].copy()
    first[0] = d["x"][3]
    last[8] = d["x"][3]
    r0 = run_vlad(T, first, d["w"], d["b"], d["cent"], cl)
    r8 = run_vlad(T, last, d["w"], d["b"], d["cent"], cl)
    assert same_bytes(T, r0[0], r8[8])
    assert same_bytes(T, r0[1:8], r8[1:8])


@pytest.mark.parametrize("path,case,cl", [("generic", (2, 31, 300), False), ("split", (3, 33, 17), False), ("fast", (9, 33, 17), False),
                                          ("fast_nhwc", (9, 33, 17), True), ("matrix", (9, 256, 33), True)])
def test_vlad_output_pitch(T, path, case, cl):
    """`out` a view of a [B, 64 C + 40] buffer of sentinels: the 40 padding columns keep them, the rows are those of a tight call."""
    B, Cc, P = case
    assert hr.vlad_path(B, Cc, P, cl) == path
    d = hr.vlad_case(B, Cc, P, "gauss")
    tight = run_vlad(T, d["x"], d["w"], d["b"], d["cent"], cl)
    rows, buf = run_vlad(T, d["x"], d["w"], d["b"], d["cent"], cl, pad=40)
    assert keeps_sentinel(T, buf[:, K * Cc:])
    assert same_bytes(T, rows, tight)
    assert check_rows(tight, d)[1] is None


def test_vlad_refusals_launch_nothing(T):
    """K = 32, C = 513, a pitch below 64 C, and the channels-last entry with eight images: an argument error, the output untouched
    (the buffers are large enough for the shape asked for), and a good call on the same stream right after still works."""
    torch, _, lib = T
    B, Cc, P = 9, 33, 17
    d = hr.vlad_case(B, Cc, P, "gauss")
    big = 513
    feat = torch.zeros((B, big, P), device="cuda")
    feat[:, :Cc] = dev(T, d["x"])
    dw, db, dc = torch.zeros((K, big), device="cuda"), dev(T, d["b"]), torch.zeros((K, big), device="cuda")
    good = run_vlad(T, d["x"], d["w"], d["b"], d["cent"], False)

    def call(fn, B_, C_, K_, ldo):
        out = sentinel_rows(T, B, K * big)
        rc = fn(feat.data_ptr(), dw.data_ptr(), db.data_ptr(), dc.data_ptr(), B_, C_, P, K_, out.data_ptr(), ldo, stream(T))
        torch.cuda.synchronize()
        return rc, lib.cslam_last_error(), out

    for what, fn, B_, C_, K_, ldo in [("K = 32", lib.cslam_vlad_aggregate_dev, B, Cc, 32, K * big),
                                      ("C = 513", lib.cslam_vlad_aggregate_dev, B, big, K, K * big),
                                      ("pitch", lib.cslam_vlad_aggregate_dev, B, Cc, K, K * Cc - 1),
                                      ("nhwc B = 8", lib.cslam_vlad_aggregate_nhwc_dev, 8, Cc, K, K * big)]:
        rc, msg, out = call(fn, B_, C_, K_, ldo)
        assert rc == -1 and b"invalid argument" in msg, (what, rc, msg)
        assert keeps_sentinel(T, out), what
        again = run_vlad(T, d["x"], d["w"], d["b"], d["cent"], False)
        assert same_bytes(T, again, good), what
    assert check_rows(good, d)[1] is None


# --------------------------------------------------------------------------------------------------------------- projection ----
def run_pca(T, xb, cb, B, din, dout, mean, scale, ops):
    """cslam_pca_project_dev on the leading [B, din] of the pitched x buffer and the leading [dout, din] of the components'"""
    torch, _, lib = T
    _, _, mp, inv = ops
    out = torch.empty((B, dout), device="cuda")
    rc = lib.cslam_pca_project_dev(xb.data_ptr(), xb.stride(0), cb.data_ptr(), cb.stride(0), mp.data_ptr() if mean else None,
                                   inv.data_ptr() if scale else None, B, din, dout, out.data_ptr(), stream(T))
    assert rc == 0, lib.cslam_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def pitched(T, a, din, extra):
    """the leading `din` columns of `a` in a buffer of pitch din + extra whose padding is NaN"""
    buf = np.full((a.shape[0], din + extra), np.nan, np.float32)
    buf[:, :din] = a[:, :din]
    return dev(T, buf)


def check_pca(got, B, din, dout, mean, scale):
    ref, raw = hr.pca_ref(B, din, dout, mean, scale)
    assert np.all(np.isfinite(got)), "a NaN of the padding reached the output: B=%d Din=%d Dout=%d" % (B, din, dout)
    over = np.abs(got.astype(np.float64) - ref) - hr.pca_bound(dout, ref)
    assert over.max() <= 0, "B=%d Din=%d Dout=%d mean=%s scale=%s: %.3g over the bound at %s" % (
        B, din, dout, mean, scale, over.max(), np.unravel_index(over.argmax(), over.shape))
    if not mean and B > hr.PCA_ZERO_ROW:
        assert np.all(got[hr.PCA_ZERO_ROW] == 0)


@pytest.fixture(scope="module")
def pca_ops(T):
    x, comp, mp, inv = hr.pca_operands()
    return x, comp, dev(T, mp), dev(T, inv)


@pytest.mark.parametrize("table,din", [("gemv", k) for k in hr.PCA_GEMV["Din"]] + [("tile", k) for k in hr.PCA_TILE["Din"]])
def test_pca_project_on_exact_integers(T, pca_ops, table, din):
    """Every (B, Dout) of the table at this Din, the four epilogues in turn, x and the components as views of wider buffers whose
    padding holds NaN: within (Dout / 2 + 4) u |ref| of float64, the zero row exactly zero where no mean term is given."""
    t = hr.PCA_GEMV if table == "gemv" else hr.PCA_TILE
    xb, cb = pitched(T, pca_ops[0], din, 8), pitched(T, pca_ops[1], din, 12)
    i = t["Din"].index(din)
    seen = set()
    for B in t["B"]:
        for dout in t["Dout"]:
            mean, scale = hr.pca_epilogues(i)
            i += 1
            seen.add((mean, scale))
            check_pca(run_pca(T, xb, cb, B, din, dout, mean, scale, pca_ops), B, din, dout, mean, scale)
    assert len(seen) == 4


@pytest.mark.parametrize("din", [2016, 4128])
def test_pca_project_four_rows_against_five(T, pca_ops, din):
    """Rows 0..3 through the matrix-vector kernel (B = 4) and through the tile kernel (B = 5): both within the bound."""
    xb, cb = pitched(T, pca_ops[0], din, 8), pitched(T, pca_ops[1], din, 12)
    for i in range(4):
        mean, scale = hr.pca_epilogues(i)
        for B in (4, 5):
            check_pca(run_pca(T, xb, cb, B, din, 129, mean, scale, pca_ops), B, din, 129, mean, scale)


# ------------------------------------------------------------------------------------------------------------ normalisation ----
def run_l2(T, x, ld, eps, zero_one):
    torch, _, lib = T
    n, d = x.shape
    buf = sentinel_rows(T, n, ld)
    buf[:, :d] = dev(T, x)
    rc = lib.cslam_l2_normalize_dev(buf.data_ptr(), n, d, ld, eps, int(zero_one), stream(T))
    assert rc == 0, lib.cslam_last_error()
    torch.cuda.synchronize()
    assert keeps_sentinel(T, buf[:, d:]) or ld == d, "padding overwritten"
    return buf[:, :d].cpu().numpy()


@pytest.mark.parametrize("d", hr.L2_D)
def test_l2_normalize(T, d):
    """One and 37 rows, tight and pitched (ld = d + 5, sentinels in the padding): every output within
    ((ceil(d / 256) + 10) / 2 + 4) u |ref| of float64 (256 threads: ceil(d / 256) squares per thread, six shuffle steps, four wave
    partials; half of that for the norm, one ulp for the square root, one for the quotient); integer rows with an exact
    perfect-square sum byte-equal to float32(x / norm); a zero row stays zero under both rules; a norm below eps is divided by eps;
    eps = 10 above every norm."""
    x37, sp = hr.l2_rows(37, d, d)
    sets = [x37, x37[:1], x37[sp["square"]:sp["square"] + 1]]
    for x in sets:
        for ld in (d, d + 5):
            for eps, zero_one, scale in ((1e-12, False, 1.0), (1e-12, True, 1.0), (10.0, False, 1.0 / 16)):
                xs = (x * np.float32(scale)).astype(np.float32)
                got = run_l2(T, xs, ld, eps, zero_one)
                ref = hr.l2_ref(xs, eps, zero_one)
                over = np.abs(got.astype(np.float64) - ref) - hr.l2_bound(d, ref)
                assert np.all(np.isfinite(got)) and over.max() <= 0, (x.shape, ld, eps, zero_one, over.max())
                if x.shape[0] == 37:
                    assert np.all(got[sp["zero"]] == 0)
                    sq = sp["square"]
                else:
                    sq = 0 if x is sets[2] else None
                if sq is not None and scale == 1.0:
                    want = xs[sq] / np.float32(3 * int(np.sqrt(d)))
                    assert want.dtype == np.float32 and np.array_equal(got[sq].view(np.int32), want.view(np.int32))
                if eps == 10.0:
                    assert np.array_equal(got, xs / np.float32(10.0))
