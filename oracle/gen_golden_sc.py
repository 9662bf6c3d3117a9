#!/usr/bin/env python
"""oracle/gen_golden_sc.py -- TEST INFRASTRUCTURE.  Generates tests/golden/sc_g9.npz, with `cloud`
tests/golden/sc_cloud_g11.npz, with `edges` tests/golden/sc_edges_g13.npz (constructed edge cases).

Runs ONLY in the build container: imports the real reference
(cslam/lidar_pr/scancontext_matching.py, scancontext_utils.py) from /root/reference and records,
for seeded synthetic scan contexts, what ScanContextMatching.search / search_best return plus the
intermediate quantities (KD-tree ring-key candidates, per-candidate distance_sc distance and yaw).
The fixture holds inputs (u16-quantised heights) and the reference's outputs only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, "/root/reference")
from helpers import synth_scancontexts, synth_sc_revisits  # noqa: E402


def main():
    from scipy import spatial
    import cslam.lidar_pr.scancontext_utils as sc_utils
    from cslam.lidar_pr.scancontext_matching import ScanContextMatching

    out = {}
    names = []
    for name, seed, n, m, ncand in (("n3", 11, 3, 3, 10), ("n12", 12, 12, 4, 10),
                                    ("n150", 13, 150, 8, 10), ("n150c4", 14, 150, 4, 4)):
        rng = np.random.default_rng(seed)
        bank = synth_scancontexts(rng, n)
        q, place, shift = synth_sc_revisits(rng, bank, m)
        q[-1] = synth_scancontexts(rng, 1)[0]            # one query that revisits nothing
        if name == "n12":
            q[0] = 0.0                                    # all-empty query -> "no match" branch
        matcher = ScanContextMatching(num_candidates=ncand)
        for i in range(n):
            matcher.add_item(bank[i].reshape(-1), 1000 + 7 * i)
        items, sims, cands, dists, yaws = [], [], [], [], []
        for j in range(m):
            it, s = matcher.search(q[j].reshape(-1), 1)
            it2, s2 = matcher.search_best(q[j].reshape(-1))
            assert it2 == it[0] and s2 == s[0]
            items.append(it[0]); sims.append(s[0])
            tree = spatial.KDTree(np.array(matcher.ringkeys[:n]))
            _, ci = tree.query(sc_utils.sc2rk(q[j]), k=ncand)
            ci = np.atleast_1d(ci)
            cands.append(ci)
            dd, yy = [], []
            for c in ci:
                d, y = sc_utils.distance_sc(matcher.scancontexts[c], q[j])
                dd.append(d); yy.append(y)
            dists.append(dd); yaws.append(yy)
        out[name + "/bank_u16"] = np.round(bank * 256.0).astype(np.uint16)
        out[name + "/q_u16"] = np.round(q * 256.0).astype(np.uint16)
        out[name + "/ringkeys"] = np.array(matcher.ringkeys[:n])
        out[name + "/items"] = np.array(items, dtype=np.int64)
        out[name + "/sims"] = np.array(sims, dtype=np.float64)
        out[name + "/cands"] = np.array(cands, dtype=np.int64)
        out[name + "/dists"] = np.array(dists, dtype=np.float64)
        out[name + "/yaws"] = np.array(yaws, dtype=np.int64)
        out[name + "/place"] = place
        out[name + "/shift"] = shift
        out[name + "/ncand"] = np.int64(ncand)
        names.append(name)
        print(name, "items", items, "sims", np.round(sims, 4), "place", 1000 + 7 * place, "shift", shift)
    # empty matcher behaviour (scancontext_matching.py:52-53, 96-97)
    e = ScanContextMatching()
    r = e.search(np.zeros(1200), 1)
    assert r == ([None], [None]) and e.search_best(np.zeros(1200)) == (None, None)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "..", "tests", "golden", "sc_g9.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main_cloud():
    """ptcloud2sc (scancontext_utils.py:46-75) on float64 point clouds -> tests/golden/sc_cloud_g11.npz."""
    import cslam.lidar_pr.scancontext_utils as sc_utils
    from helpers import synth_lidar_cloud
    out = {}
    for name, seed, n, dense in (("wall40k", 31, 40000, True), ("sparse6k", 32, 6000, False), ("tiny", 33, 40, False)):
        pts32 = synth_lidar_cloud(np.random.default_rng(seed), n, dense)
        pts = pts32.astype(np.float64)
        sc = sc_utils.ptcloud2sc(pts, [20, 60], 80)
        out[name + "/pts"] = pts32
        out[name + "/sc"] = sc
        cnt = np.zeros((20, 60), int)
        for p in pts:
            if not np.isnan(p).any():
                r, c = sc_utils.pt2rs(p, 4.0, 6.0, 20, 60)
                cnt[r, c] += 1
        print(name, "points", n, "bins over the 500 cap:", int((cnt > 500).sum()), "max", cnt.max(),
              "nonzero bins", int((sc != 0).sum()))
    out["names"] = np.array(["wall40k", "sparse6k", "tiny"])
    path = os.path.join(HERE, "..", "tests", "golden", "sc_cloud_g11.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


# ---- edges: constructed cases, one edge each -> tests/golden/sc_edges_g13.npz -----------------------------
TINY = 1e-200          # a coordinate whose square underflows to 0 and whose angle is 0: `far` is the other one exactly


def axis_point(far, direction, z):
    """A point at distance exactly `far` along +x, +y, -x or -y (the other coordinate is TINY, not 0.0, which the
    reference replaces by 0.001)."""
    far = far if far != 0.0 else TINY
    return [(far, TINY, z), (TINY, far, z), (-far, TINY, z), (TINY, -far, z)][direction % 4]


def cap_position_cloud(P, pattern):
    """Bin A's 500th point sits at cloud index P and is the highest of its first 500; every later A point is higher
    still and must be dropped.  pattern 'alt': A alternates with bin B lane by lane up to and past P (what is left of
    the prefix is bin C); 'run': A is one contiguous run that ends a whole 1024-point chunk after P."""
    A, B, Cc = (10.0, 10.0), (-30.0, 5.0), (3.0, -50.0)
    bins, n_fill = [], P - 499
    assert n_fill >= 0
    if pattern == "alt":
        alt = min(n_fill, 499)
        head = [Cc] * (n_fill - alt) + [A] * (499 - alt)
        body = [B, A] * alt
        bins = head + body + [A] + [B, A] * 40
    else:
        bins = [B if i % 3 else Cc for i in range(n_fill)] + [A] * 500
        bins += [A] * (2048 - len(bins) % 1024)
    pts = np.zeros((len(bins), 3))
    seen = {A: 0, B: 0, Cc: 0}
    for i, b in enumerate(bins):
        k = seen[b]
        seen[b] += 1
        # heights rise with the count: the kept maximum of a capped bin is its 500th point exactly
        z = (k / 1024.0 if k < 499 else (5.0 if k == 499 else 9.0 + k / 1024.0))
        pts[i] = (b[0], b[1], z if b == A else z - 1.0)
    assert seen[A] > 500 and bins[P] == A and bins[:P].count(A) == 499
    return pts


def descriptor_cases():
    """[(name, points float64 [n,3], (rings, sectors), max_length)]"""
    rng = np.random.default_rng(1301)
    cases = []

    def add(name, pts, shape=(20, 60), max_length=80):
        cases.append((name, np.asarray(pts, dtype=np.float64).reshape(-1, 3), shape, max_length))

    # ring edges: far exactly on 4k and one ulp below, one point per bin (direction cycles so that no two share one)
    fars = [(4.0 * k, "on") for k in range(26)] + [(np.nextafter(4.0 * k, 0.0), "below") for k in range(1, 26)]
    fars += [(80.0 * 1e6, "far"), (np.nextafter(80.0, 100.0), "above80")]
    for tag in ("on", "below", "far", "above80"):
        group = [f for f, t in fars if t == tag]
        for g0 in range(0, len(group), 4):            # ring 19 takes every far >= 76: at most four of them per frame
            chunk = group[g0:g0 + 4] if group[g0] >= 76.0 else group[g0:g0 + 20]
            if group[g0] < 76.0 and g0 % 20:
                continue
            add("ring_%s_%d" % (tag, g0), [axis_point(f, i, 0.5 + i / 64.0) for i, f in enumerate(chunk)])
    # sector edges: multiples of 6 degrees in all four quadrants, each in a ring of its own sector group
    ang = np.arange(60) * 6.0
    rad = 4.0 * (np.arange(60) % 20) + 2.0
    add("sector_multiples", np.stack([rad * np.cos(np.deg2rad(ang)), rad * np.sin(np.deg2rad(ang)),
                                      1.0 + np.arange(60) / 64.0], axis=1))
    exact = [(1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (3.0, 3.0), (-7.0, 7.0)]       # 45, 135, 225, 315
    add("sector_diagonals", [(5.0 * x, 5.0 * y, 0.25 * (i + 1)) for i, (x, y) in enumerate(exact)])
    zeros = [(0.0, 5.0), (0.0, -9.0), (13.0, 0.0), (-17.0, 0.0), (-0.0, 21.0), (25.0, -0.0), (-29.0, -0.0), (0.0, 0.0),
             (-0.0, -0.0), (0.0, -0.0), (-0.0, -33.0), (TINY, 37.0), (-TINY, -41.0), (5e-324, 5e-324)]
    add("axis_zero", [(x, y, 0.125 * (i + 1)) for i, (x, y) in enumerate(zeros)])
    for i, (x, y) in enumerate(zeros):                 # and alone: several of them share ring 0
        add("axis_zero_%d" % i, [(x, y, 1.5)])
    # the 500-point cap in one bin, the highest point last
    for m in (499, 500, 501):
        z = np.arange(m) / 1024.0
        z[-1] = 7.0
        add("cap_%d" % m, np.stack([np.full(m, 10.0), np.full(m, 10.0), z], axis=1))
        zn = -3.0 - (m - np.arange(m)) / 1024.0       # every height + 2 negative, rising, the highest last
        add("cap_neg_%d" % m, np.stack([np.full(m, 10.0), np.full(m, 10.0), zn], axis=1))
    # cap position.  The 500th point of a bin cannot sit before cloud index 499, so the lane edge 63 | 64 is taken
    # at the first wave edge past it: indices 575 (lane 63 of wave 8) and 576 (lane 0 of wave 9)
    for P in (575, 576, 1023, 1024, 1025, 2047, 2048):
        for pattern in ("alt", "run"):
            add("cappos_%s_%d" % (pattern, P), cap_position_cloud(P, pattern))
    # other shapes
    for name, shape, ml, n in (("shape_1x1", (1, 1), 80, 40), ("shape_3x7", (3, 7), 80, 300),
                               ("shape_32x64", (32, 64), 10.5, 2500)):
        r = rng.random(n) * ml * 1.2
        a = rng.random(n) * 2 * np.pi
        add(name, np.stack([r * np.cos(a), r * np.sin(a), rng.random(n) * 6 - 3], axis=1), shape, ml)
    # failures, each between ordinary points
    body = np.stack([np.linspace(2, 70, 30), np.linspace(-40, 40, 30), np.linspace(-1, 3, 30)], axis=1)
    for name, bad in (("theta_360", (1.0, -1e-300, 0.0)), ("inf_x", (np.inf, 1.0, 0.0)), ("neg_inf_x", (-np.inf, 1.0, 0.0)),
                      ("inf_y", (1.0, np.inf, 0.0)), ("neg_inf_y", (-2.0, -np.inf, 0.0)), ("inf_xy", (np.inf, np.inf, 0.0)),
                      ("x_1e200", (1e200, 1.0, 0.0)), ("neg_x_1e200", (-1e200, -1.0, 0.0)), ("y_1e200", (3.0, 1e200, 0.0)),
                      ("inf_x_then_360", None), ("theta_360_then_inf_x", None),
                      ("inf_z", (5.0, 5.0, np.inf)), ("neg_inf_z", (5.0, 5.0, -np.inf)), ("nan_z_inf_x", (np.inf, 1.0, np.nan))):
        if name == "inf_x_then_360":
            rows = [body[:10], [(np.inf, 1.0, 0.0)], body[10:20], [(1.0, -1e-300, 0.0)], body[20:]]
        elif name == "theta_360_then_inf_x":
            rows = [body[:10], [(1.0, -1e-300, 0.0)], body[10:20], [(np.inf, 1.0, 0.0)], body[20:]]
        else:
            rows = [body[:15], [bad], body[15:]]
        add(name, np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 3) for r in rows]))
    return cases


def binade_rows(rng, R, S):
    """Entries spread over 25 binades with both signs: the order of a sum shows in its last bits."""
    return (rng.random((R, S)) + 1.0) * np.exp2(rng.integers(-12, 13, size=(R, S))) * rng.choice([-1.0, 1.0], size=(R, S))


def distance_contexts():
    """{group: contexts [m, R, S]}; every ordered pair of a group is recorded."""
    rng = np.random.default_rng(1302)
    R, S = 20, 60
    cell = np.zeros((R, S)); cell[3, 5] = 2.0
    signed = np.round(rng.standard_normal((R, S)) * 512) / 256.0
    left = np.round(rng.random((R, S)) * 1024) / 256.0; left[:, 30:] = 0.0
    right = np.round(rng.random((R, S)) * 1024) / 256.0; right[:, :30] = 0.0
    sparse = (np.round(rng.random((R, S)) * 1024) / 256.0) * (rng.random((R, S)) > 0.9)
    big = [np.ones((R, S)), np.full((R, S), 2.5), cell, np.roll(cell, 1, axis=1), np.roll(cell, 30, axis=1),
           np.roll(cell, 59, axis=1), signed, -np.roll(signed, 7, axis=1), np.zeros((R, S)), left, right, sparse,
           -np.abs(sparse) - (sparse == 0) * 0.5]
    s1 = [np.arange(1.0, 6.0)[:, None], -np.arange(1.0, 6.0)[:, None], np.zeros((5, 1)), np.ones((5, 1)),
          np.array([0.0, 0.0, 3.0, 0.0, -1.0])[:, None]]
    c9 = np.zeros((1, 9)); c9[0, 2] = 4.0
    r1 = [np.ones((1, 9)), c9, np.roll(c9, 4, axis=1), np.zeros((1, 9)), np.round(rng.standard_normal((1, 9)) * 64) / 16.0,
          np.array([[1.0, 0, 0, -2.0, 0, 0, 3.0, 0, 0]])]
    return {"20x60": np.stack(big), "5x1": np.stack(s1), "1x9": np.stack(r1)}


RK_SECTORS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128)


def duplicate_cases():
    """[(name, bank [n,R,S], queries [nq,R,S], num_candidates, tie group rows)]: banks with identical rows."""
    rng = np.random.default_rng(1303)
    R, S = 6, 12

    def ctx(m):
        return (np.round(rng.random((m, R, S)) * 1024) / 256.0) * (rng.random((m, R, S)) > 0.25)

    cases = []
    bank = ctx(12)
    bank[4] = bank[5] = bank[3]
    near = np.roll(bank[3], 2, axis=1) + (rng.random((R, S)) < 0.1) * 0.25
    cases.append(("inside", bank, np.stack([near, np.roll(bank[9], 5, axis=1)]), 5, [3, 4, 5]))
    cases.append(("straddle", bank, np.stack([near, np.roll(bank[3], 1, axis=1)]), 2, [3, 4, 5]))
    cases.append(("query_is_the_row", bank, np.stack([bank[3], bank[0]]), 4, [3, 4, 5]))
    still = np.repeat(ctx(1), 6, axis=0)
    cases.append(("standing_still", still, np.stack([still[0], np.roll(still[0], 3, axis=1), ctx(1)[0]]), 4, list(range(6))))
    return cases


def main_edges():
    from scipy import spatial
    import cslam.lidar_pr.scancontext_utils as sc_utils
    from cslam.lidar_pr.scancontext_matching import ScanContextMatching
    out = {}
    names = []
    for name, pts, shape, ml in descriptor_cases():
        out["desc/%s/pts" % name] = pts
        out["desc/%s/shape" % name] = np.array(shape, dtype=np.int64)
        out["desc/%s/max_length" % name] = np.float64(ml)
        try:
            with np.errstate(all="ignore"):
                out["desc/%s/sc" % name] = sc_utils.ptcloud2sc(pts, list(shape), ml)
        except (IndexError, ValueError) as e:
            out["desc/%s/exc" % name] = np.array(type(e).__name__)
            print(name, "raises", type(e).__name__, e)
        names.append(name)
    out["desc_names"] = np.array(names)
    rng = np.random.default_rng(1304)
    for S in RK_SECTORS:
        sc = binade_rows(rng, 4, S)
        out["rk/%d/sc" % S] = sc
        out["rk/%d/rk" % S] = sc_utils.sc2rk(sc)
    out["rk_sectors"] = np.array(RK_SECTORS, dtype=np.int64)
    groups = distance_contexts()
    for g, ctx in groups.items():
        m = len(ctx)
        D = np.zeros((m, m)); Y = np.zeros((m, m), dtype=np.int64)
        for i in range(m):
            for j in range(m):
                D[i, j], Y[i, j] = sc_utils.distance_sc(ctx[i], ctx[j])        # candidate i, query j
        out["dist/%s/ctx" % g] = ctx
        out["dist/%s/D" % g] = D
        out["dist/%s/Y" % g] = Y
        print("distances", g, m, "contexts; constant pair", D[0, 0], Y[0, 0])
    out["dist_groups"] = np.array(list(groups))
    dnames = []
    for name, bank, q, ncand, tie in duplicate_cases():
        n, (R, S) = len(bank), bank.shape[1:]
        matcher = ScanContextMatching(shape=[R, S], num_candidates=ncand)
        for i in range(n):
            matcher.add_item(bank[i].reshape(-1), i)
        cands, dists, yaws, sims = [], [], [], []
        for j in range(len(q)):
            _, s = matcher.search(q[j].reshape(-1), 1)
            sims.append(s[0])
            tree = spatial.KDTree(np.array(matcher.ringkeys[:n]))
            _, ci = tree.query(sc_utils.sc2rk(q[j]), k=ncand)
            ci = np.atleast_1d(ci)
            dy = [sc_utils.distance_sc(matcher.scancontexts[c], q[j]) for c in ci]
            dists.append([d for d, _ in dy]); yaws.append([y for _, y in dy])
            cands.append(np.where(np.isin(ci, tie), -2, ci))                   # which duplicate was named is not kept
        for k, v in (("bank", bank), ("q", q), ("ncand", np.int64(ncand)), ("tie", np.array(tie, dtype=np.int64)),
                     ("cands", np.array(cands, dtype=np.int64)), ("dists", np.array(dists)),
                     ("yaws", np.array(yaws, dtype=np.int64)), ("sims", np.array(sims))):
            out["dup/%s/%s" % (name, k)] = v
        dnames.append(name)
        print("duplicates", name, "cands", np.array(cands).tolist(), "sims", np.round(sims, 4))
    out["dup_names"] = np.array(dnames)
    path = os.path.join(HERE, "..", "tests", "golden", "sc_edges_g13.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(names), "descriptor cases")


if __name__ == "__main__":
    if "edges" in sys.argv[1:]:
        main_edges()
    elif "cloud" in sys.argv[1:]:
        main_cloud()
    else:
        main()
