"""CPU: the ScanContext oracle (oracle/sc_oracle.c) against the golden vectors recorded from the
reference (oracle/gen_golden_sc.py -> tests/golden/sc_g9.npz)."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, synth_scancontexts, synth_sc_revisits
from oracle import pyoracle


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(GOLDEN, "sc_g9.npz"))


def case(g, name):
    bank = g[name + "/bank_u16"].astype(np.float64) / 256.0
    q = g[name + "/q_u16"].astype(np.float64) / 256.0
    return bank, q, int(g[name + "/ncand"])


def test_golden_has_all_cases(g9):
    assert list(g9["names"]) == ["n3", "n12", "n150", "n150c4"]


@pytest.mark.parametrize("name", ["n3", "n12", "n150", "n150c4"])
def test_oracle_matches_reference(g9, name):
    bank, q, ncand = case(g9, name)
    n = len(bank)
    rk = np.stack([pyoracle.sc_ringkey(b) for b in bank])
    assert np.array_equal(rk, g9[name + "/ringkeys"])                 # numpy's summation order
    o = pyoracle.sc_search(bank, q, ncand)
    ref_c = g9[name + "/cands"].copy()
    ref_c[ref_c >= n] = -1                                            # KD-tree "missing neighbour" marker
    assert np.array_equal(o["cand"], ref_c)
    m = ref_c >= 0
    assert np.abs(o["cdist"] - g9[name + "/dists"])[m].max() <= 1e-12
    assert np.array_equal(o["cyaw"][m], g9[name + "/yaws"][m])
    items = np.where(o["best_idx"] >= 0, 1000 + 7 * o["best_idx"], 1000)
    assert np.array_equal(items, g9[name + "/items"])
    assert np.abs(o["best_sim"] - g9[name + "/sims"]).max() <= 1e-12


def test_oracle_distance_function_properties():
    rng = np.random.default_rng(5)
    bank = synth_scancontexts(rng, 4)
    for s in (1, 17, 59):
        d, yaw = pyoracle.sc_distance(bank[0], np.roll(bank[0], s, axis=1))
        assert abs(d) < 1e-15 and yaw == s
    d, yaw = pyoracle.sc_distance(bank[0], bank[0])                   # zero shift is found last (roll by 60)
    assert abs(d) < 1e-15 and yaw == 60
    d, yaw = pyoracle.sc_distance(bank[0], np.zeros_like(bank[0]))    # nothing engaged
    assert d == 1.0 and yaw == 1


def test_oracle_row_limit_and_revisits():
    rng = np.random.default_rng(6)
    bank = synth_scancontexts(rng, 60)
    q, place, shift = synth_sc_revisits(rng, bank, 6)
    o = pyoracle.sc_search(bank, q, 10)
    assert np.array_equal(o["best_idx"], place)
    assert np.array_equal(o["best_yaw"], np.where(shift == 0, 60, shift))
    lim = np.minimum(place, 5)                                        # hide the true place
    o2 = pyoracle.sc_search(bank, q, 10, row_limit=lim)
    assert np.all(o2["best_idx"] < np.maximum(lim, 1)) and np.all(o2["cand"] < lim[:, None])


def test_ptcloud2sc_oracle_matches_reference():
    g = np.load(os.path.join(GOLDEN, "sc_cloud_g11.npz"))
    assert list(g["names"]) == ["wall40k", "sparse6k", "tiny"]
    for name in g["names"]:
        sc = pyoracle.ptcloud2sc(g[name + "/pts"].astype(np.float64))
        assert np.array_equal(sc, g[name + "/sc"]), name
    # the 500-point storage cap is order dependent: the fixture has bins far above it
    pts = g["wall40k/pts"].astype(np.float64)
    assert not np.array_equal(pyoracle.ptcloud2sc(pts[::-1].copy()), g["wall40k/sc"])


# ---- constructed edges (oracle/gen_golden_sc.py edges -> tests/golden/sc_edges_g13.npz) ------------------
@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "sc_edges_g13.npz"))


def test_edge_fixture_descriptor_cases(g13):
    """Every recorded descriptor case: the oracle's descriptor is bit-equal, or it raises the recorded class."""
    names = [str(n) for n in g13["desc_names"]]
    assert len(set(names)) == len(names)
    # the cap's 500th point cannot sit before cloud index 499: the lane edge 63 | 64 is taken at 575 | 576
    expected = (["ring_on_0", "ring_on_20", "ring_on_24", "ring_below_0", "ring_below_20", "ring_below_24", "ring_far_0",
                 "ring_above80_0", "sector_multiples", "sector_diagonals", "axis_zero"]
                + ["axis_zero_%d" % i for i in range(14)]
                + [p % m for m in (499, 500, 501) for p in ("cap_%d", "cap_neg_%d")]
                + ["cappos_%s_%d" % (p, P) for P in (575, 576, 1023, 1024, 1025, 2047, 2048) for p in ("alt", "run")]
                + ["shape_1x1", "shape_3x7", "shape_32x64", "theta_360", "inf_x", "neg_inf_x", "inf_y", "neg_inf_y", "inf_xy",
                   "x_1e200", "neg_x_1e200", "y_1e200", "inf_x_then_360", "theta_360_then_inf_x", "inf_z", "neg_inf_z",
                   "nan_z_inf_x"])
    assert names == expected
    raised = {}
    for name in names:
        pts, shape = g13["desc/%s/pts" % name], tuple(int(v) for v in g13["desc/%s/shape" % name])
        ml = float(g13["desc/%s/max_length" % name])
        if "desc/%s/exc" % name in g13:
            exc = {"IndexError": IndexError, "ValueError": ValueError}[str(g13["desc/%s/exc" % name])]
            with pytest.raises(exc):
                pyoracle.ptcloud2sc(pts, shape, ml)
            raised[name] = exc
        else:
            assert np.array_equal(pyoracle.ptcloud2sc(pts, shape, ml), g13["desc/%s/sc" % name]), name
    assert raised == {"theta_360": IndexError, "theta_360_then_inf_x": IndexError, "inf_x": ValueError,
                      "neg_inf_x": ValueError, "inf_y": ValueError, "neg_inf_y": ValueError, "inf_xy": ValueError,
                      "x_1e200": ValueError, "neg_x_1e200": ValueError, "y_1e200": ValueError, "inf_x_then_360": ValueError}
    # what the cases are built for, read off the recorded reference outputs
    assert g13["desc/cap_500/sc"][3, 7] == 9.0 and g13["desc/cap_501/sc"][3, 7] == 2.0 + 499 / 1024.0
    assert g13["desc/cap_neg_499/sc"][3, 7] == 0.0 and g13["desc/cap_neg_500/sc"][3, 7] == -1.0 - 1 / 1024.0
    assert g13["desc/cap_neg_501/sc"][3, 7] == -1.0 - 2 / 1024.0
    assert g13["desc/inf_z/sc"][1, 7] == np.inf and g13["desc/neg_inf_z/sc"][1, 7] == 0.0
    for name in names:
        if name.startswith("cappos_"):
            assert g13["desc/%s/sc" % name][3, 7] == 7.0, name             # the 500th point, nothing after it


def tail_first_sum(a):
    """numpy's pairwise sum of 8 < n <= 128 values with the n % 8 tail added before the blocks instead of after."""
    n = len(a) - len(a) % 8
    r = a[:8].copy()
    for i in range(8, n, 8):
        r = r + a[i:i + 8]
    res = 0.0
    for v in a[n:]:
        res = res + v
    return res + (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))


def test_edge_fixture_ring_keys(g13):
    assert list(g13["rk_sectors"]) == [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128]
    for S in g13["rk_sectors"]:
        sc = g13["rk/%d/sc" % S]
        assert np.array_equal(pyoracle.sc_ringkey(sc), g13["rk/%d/rk" % S]), S
        if S >= 16:                                                      # the order shows: other sums of the same row differ
            assert not np.array_equal(np.cumsum(sc, axis=1)[:, -1] / S, g13["rk/%d/rk" % S]), S
        if S > 8 and S % 8 >= 2:                                         # (one tail value commutes)
            assert not np.array_equal(np.array([tail_first_sum(r) for r in sc]) / S, g13["rk/%d/rk" % S]), S


def test_edge_fixture_distances(g13):
    assert list(g13["dist_groups"]) == ["20x60", "5x1", "1x9"]
    for grp in g13["dist_groups"]:
        ctx, D, Y = g13["dist/%s/ctx" % grp], g13["dist/%s/D" % grp], g13["dist/%s/Y" % grp]
        for i in range(len(ctx)):
            for j in range(len(ctx)):
                d, y = pyoracle.sc_distance(ctx[i], ctx[j])
                assert abs(d - D[i, j]) <= 1e-12 and y == Y[i, j], (grp, i, j, d, D[i, j], y, Y[i, j])
    D, Y = g13["dist/20x60/D"], g13["dist/20x60/Y"]
    assert abs(D[0, 1]) <= 1e-12 and Y[0, 1] == 1                        # constant contexts: every shift ties
    assert [int(Y[2, k]) for k in (2, 3, 4, 5)] == [60, 1, 30, 59] and np.all(np.abs(D[2, 2:6]) <= 1e-12)
    assert np.all(D[8] == 1.0) and np.all(D[:, 8] == 1.0) and np.all(Y[8] == 1) and np.all(Y[:, 8] == 1)   # empty


def test_edge_fixture_duplicate_rows(g13):
    """Banks with identical rows.  Which member of a tie group the KD-tree names is not defined: those entries (and
    only those) are left out of the candidate comparison; distances, yaws and similarities are compared everywhere."""
    assert list(g13["dup_names"]) == ["inside", "straddle", "query_is_the_row", "standing_still"]
    for name in g13["dup_names"]:
        k = "dup/%s/" % name
        bank, q, ncand, tie = g13[k + "bank"], g13[k + "q"], int(g13[k + "ncand"]), g13[k + "tie"]
        assert np.all(bank[tie] == bank[tie[0]])
        o = pyoracle.sc_search(bank, q, ncand)
        ref_c = g13[k + "cands"]
        out = ref_c == -2
        assert np.all(out.sum(axis=1) <= len(tie))                       # no more left out than the tie group
        assert np.array_equal(o["cand"][~out], ref_c[~out])
        assert np.all(np.isin(o["cand"][out], tie))
        for j in range(len(q)):                                          # within the group: the smaller rows, in order
            inside = o["cand"][j][out[j]]
            assert np.array_equal(inside, tie[:len(inside)]), (name, j)
        assert np.abs(o["cdist"] - g13[k + "dists"]).max() <= 1e-12
        assert np.array_equal(o["cyaw"], g13[k + "yaws"])
        assert np.abs(o["best_sim"] - g13[k + "sims"]).max() <= 1e-12
