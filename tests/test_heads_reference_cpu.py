"""The conditions on the cases of tests/test_heads_paths_gpu.py, proved from the references alone (no device): the dispatch rule
places every VLAD case in its path and has a case on each side of every limit; every planted defect moves the float64 layer by at
least ten times the tolerance the kernels are held to; the float64 restatement agrees with the float32 oracle; no assignment is
small enough to underflow in float32 (the error measure would then compare a flushed zero with 1e-60); the projection's operands keep
every partial sum an exact integer and a dropped K term moves every row by a hundred times its bound; the normalisation's integer
rows have exact perfect-square sums.

Measured on the CPU: the yardstick err(vlad_seq32, vlad_f64) is 4.2e-7 .. 4.1e-6 on the gaussian kind and 6.8e-7 .. 7.2e-5 on the
trunk kind (the steep softmax multiplies logit errors by 100) at C > 1, and 2^-24 or 0 at C = 1; the smallest planted defect is 43
tolerances (the assignment sum missing one of 255 pixels at C = 500, gaussian kind); a dropped last K term moves a projected row
by at least 730 bounds.  test_vlad_case_conditions prints every figure."""
import numpy as np
import pytest

import heads_reference as hr
from oracle import heads_oracle as ho

CASES = hr.all_vlad_cases()


def test_err_measure():
    ref = np.zeros((1, 64 * 2))
    ref[0, :2] = (2.0, -4.0)
    ref[0, 2:4] = (1e-20, 0.0)
    y = ref.copy()
    assert hr.err(y, ref) == 0.0
    y[0, 0] += 0.4                                  # relative to the row's largest entry, not to the entry
    assert abs(hr.err(y, ref) - 0.1) < 1e-15
    y[0, 3] = 1e-21                                 # a tiny row counts on its own scale
    assert abs(hr.err(y, ref) - 0.1) < 1e-15
    y[0, 3] = 2e-21
    assert abs(hr.err(y, ref) - 0.2) < 1e-15
    y[0, 3] = 0
    y[0, 5] = 1e-30                                 # a row that is zero in the reference must be exactly zero
    assert hr.err(y, ref) == float("inf")


def test_dispatch_rule_places_every_case_and_has_both_sides_of_every_limit():
    seen = set()
    for path, case in CASES:
        lay = hr.vlad_layouts(path, case)
        if path in ("generic", "split"):
            assert lay == [(False, path)], (path, case)
        elif path == "fast":
            assert [p for _, p in lay] == ["fast", "fast_nhwc"], (path, case)     # no `fast` case has the matrix form's shape
        else:
            assert lay == [(True, path)], (path, case)
        B, C, P = case
        assert B * C * P <= 9 * 512 * 385 and 1 <= C <= 512
        for cl, p in lay:
            seen.add((p, B, C, P, cl))
    runs = lambda path, cl, cond: any(p == path and c == cl and cond(B, C, P) for p, B, C, P, c in seen)   # noqa: E731
    # B = 8 | 9 at P <= 256, NCHW
    assert runs("split", False, lambda B, C, P: B == 8) and runs("fast", False, lambda B, C, P: B == 9)
    # P = 256 | 257, for few and for many images
    assert runs("split", False, lambda B, C, P: P == 256) and runs("generic", False, lambda B, C, P: P == 257 and B <= 8)
    assert runs("fast", False, lambda B, C, P: P == 256) and runs("generic", False, lambda B, C, P: P > 256 and B > 8)
    assert runs("fast_nhwc", True, lambda B, C, P: P == 256 and C % 128 == 0)
    # the matrix form: P = 31 | 32, P = 200 | 201, C a multiple of 128 or not
    assert runs("fast_nhwc", True, lambda B, C, P: P == 31 and C % 128 == 0) and runs("matrix", True, lambda B, C, P: P == 32)
    assert runs("matrix", True, lambda B, C, P: P == 200) and runs("fast_nhwc", True, lambda B, C, P: P == 201 and C % 128 == 0)
    assert runs("fast_nhwc", True, lambda B, C, P: C % 128 != 0 and 32 <= P <= 200 and C > 128)
    assert {C for p, B, C, P, c in seen if p == "matrix"} == {128, 256, 384, 512}
    # the rule itself at its limits
    assert hr.vlad_path(8, 512, 196, True) == "split" and hr.vlad_path(9, 512, 196, True) == "matrix"
    assert hr.vlad_path(9, 512, 257, True) == "generic" and hr.vlad_path(9, 640, 196, False) == "fast"
    # no bias: a case in every path
    for path in hr.VLAD_CASES:
        assert any(case in hr.NO_BIAS for case in hr.VLAD_CASES[path]) or (
            path == "fast_nhwc" and any(case in hr.NO_BIAS for case in hr.VLAD_CASES["fast"])), path
    assert hr.NO_BIAS <= {case for _, case in CASES}


@pytest.mark.parametrize("path,case", CASES + [("pairs", c) for c in hr.PAIR_CASES],
                         ids=["%s-%dx%dx%d" % ((p,) + c) for p, c in CASES + [("pairs", c) for c in hr.PAIR_CASES]])
def test_vlad_case_conditions(path, case):
    B, C, P = case
    for kind in hr.KINDS:
        d = hr.vlad_case(B, C, P, kind)
        x, w, b, cent, ref, tol = d["x"], d["w"], d["b"], d["cent"], d["ref"], d["tol"]
        assert (b is None) == (kind == "gauss" and case in hr.NO_BIAS)
        assert np.all(np.isfinite(ref)) and (0 < tol < 1e-3 or C == 1), tol
        a = hr.vlad_assignment_f64(x, w, b, cent)
        # float32 keeps every assignment a normal number, with room for the factor 1 / |x_p| and the products with x
        assert a.min() > 1e-25, a.min()
        orc = hr.err(ho.vlad_forward(x.reshape(B, C, P, 1), w, b, cent), ref)
        assert orc <= tol, (orc, tol)
        line = "%s %s %s: yardstick %.3g, oracle %.3g" % (path, case, kind, d["yard"], orc)
        if kind == "trunk":
            assert x.min() >= 0 and np.all(x[:, 36::37] == 0)
            assert np.allclose(np.linalg.norm(cent.astype(np.float64), axis=1), 1.0, atol=1e-6)
            if P > 1:
                assert np.all(x[:, :, P // 2] == 0)
            if B > 1:
                assert np.all(x[0] == 0)
            if B > 2:
                keep = np.arange(P) != P // 2 if P > 1 else np.ones(1, bool)
                if C > 1:                                     # at C = 1 all unit centroids coincide: the assignment is uniform
                    assert np.all(a[-1].argmax(axis=0)[keep] == 5) and a[-1, 5][keep].min() > 0.9
        # P = 1: the assignment cancels in the intra-normalisation; C = 1: a cluster's row is one number and the
        # intra-normalisation leaves its sign, +- 1 / 8 after the global one.  These cases check the residual (its sign) and
        # the norms only: no defect in a sum's tail moves them.
        if P > 1 and C > 1:
            for which in hr.DEFECTS:
                de = hr.err(hr.vlad_defect(x, w, b, cent, which), ref)
                line += ", %s %.3g (%.0f tol)" % (which, de, de / tol if tol else np.inf)
                assert de >= 10 * tol and de > 0, (which, de, tol)
        print(line)


def test_every_path_sees_a_zero_frame_and_a_one_cluster_frame():
    for path, cases in hr.VLAD_CASES.items():
        assert any(B > 2 for B, C, P in cases), path


# ------------------------------------------------------------------------------------------------------------ projection ----
def test_projection_operands_are_exact_in_any_order():
    x, comp, mp, inv = hr.pca_operands()
    assert set(np.unique(x)) == {-2, -1, 0, 1, 2} and set(np.unique(comp)) == {-3, -2, -1, 1, 2, 3}
    assert np.all(x[hr.PCA_ZERO_ROW] == 0) and np.all(np.abs(np.delete(x, hr.PCA_ZERO_ROW, axis=0)) >= 1)
    assert np.all(mp == np.round(mp)) and np.all(np.log2(inv) == np.round(np.log2(inv)))
    # every partial sum of any subset of the products, in any order, is an integer of magnitude <= sum |x| |comp|
    top = float((np.abs(x).astype(np.float64) @ np.abs(comp).astype(np.float64).T).max()) + float(np.abs(mp).max())
    assert top < 2 ** 24
    # so float32 sums them exactly: here in the index order and in blocks of 32 (the tile's K step)
    v64 = x.astype(np.float64) @ comp.astype(np.float64).T
    seq = np.zeros((129, 130), np.float32)
    for k0 in range(0, 4128, 32):
        seq = seq + x[:, k0:k0 + 32] @ comp[:, k0:k0 + 32].T
    assert seq.dtype == np.float32 and np.array_equal(seq.astype(np.float64), v64)
    assert np.array_equal(np.cumsum(x[:8, :, None] * comp.T[None, :, :8], axis=1, dtype=np.float32)[:, -1].astype(np.float64), v64[:8, :8])
    for t in (hr.PCA_GEMV, hr.PCA_TILE):
        assert max(t["B"]) <= 129 and max(t["Din"]) <= 4128 and max(t["Dout"]) <= 130 and all(k % 32 == 0 for k in t["Din"])
    assert max(hr.PCA_GEMV["B"]) == 4 and min(hr.PCA_TILE["B"]) == 5              # cslam_pca_project_dev: B <= 4 is the matrix-vector kernel
    assert {hr.pca_epilogues(i) for i in range(4)} == {(False, False), (True, False), (False, True), (True, True)}


@pytest.mark.parametrize("table", ["gemv", "tile"])
def test_projection_dropped_term_moves_every_row(table):
    """Dout = 1 excepted: a single normalised output is its sign, which the case checks exactly."""
    t = hr.PCA_GEMV if table == "gemv" else hr.PCA_TILE
    worst = np.inf
    i = 0
    for B in t["B"]:
        for din in t["Din"]:
            for dout in t["Dout"]:
                mean, scale = hr.pca_epilogues(i)
                i += 1
                ref, raw = hr.pca_ref(B, din, dout, mean, scale)
                assert np.all(raw == np.round(raw * 8) / 8)
                if not mean and B > hr.PCA_ZERO_ROW:
                    assert np.all(ref[hr.PCA_ZERO_ROW] == 0)
                if dout == 1:
                    assert np.all(np.abs(ref[raw[:, 0] != 0]) == 1.0)
                    continue
                bad, _ = hr.pca_ref(B, din, dout, mean, scale, drop_last=True)
                rows = np.ones(B, bool)
                if B > hr.PCA_ZERO_ROW:
                    rows[hr.PCA_ZERO_ROW] = False                                   # the zero row has no last term to lose
                move = np.abs(bad - ref).max(axis=1)[rows]
                bound = hr.pca_bound(dout, ref).max(axis=1)[rows]
                worst = min(worst, float((move / bound).min()))
    print("%s: smallest move / bound of a dropped last K term = %.3g" % (table, worst))
    assert worst >= 100


# --------------------------------------------------------------------------------------------------------- normalisation ----
@pytest.mark.parametrize("d", hr.L2_D)
def test_normalisation_rows(d):
    x, sp = hr.l2_rows(37, d, d)
    sq = x[sp["square"]].astype(np.float64)
    s = float(np.sum(sq * sq))
    q = int(np.sqrt(d))
    assert s == (3.0 * q) ** 2 and s < 2 ** 24 and set(np.unique(sq)) <= {-3.0, 0.0, 3.0}
    assert np.all(x[sp["zero"]] == 0)
    tiny = x[sp["tiny"]].astype(np.float64)
    assert 0 < np.sqrt(np.sum(tiny * tiny)) < 1e-12 and np.all((tiny == 0) | (tiny * tiny > 1e-36))
    # eps = 10 lies above every norm of x / 16
    assert np.sqrt(np.sum((x.astype(np.float64) / 16) ** 2, axis=1)).max() < 10
    ref = hr.l2_ref(x, 1e-12, False)
    assert np.all(ref[sp["zero"]] == 0) and np.allclose(ref[sp["tiny"]], tiny / np.float64(np.float32(1e-12)))
    assert np.allclose(np.linalg.norm(ref[0]), 1.0) and np.all(hr.l2_ref(x, 1e-12, True)[sp["zero"]] == 0)
