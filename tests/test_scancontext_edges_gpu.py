"""GPU: the ScanContext kernels (csrc/scancontext.hip) one at a time, at constructed edges.

Two references.  tests/golden/sc_edges_g13.npz holds what the reference itself answers at the edges
(oracle/gen_golden_sc.py edges): descriptors and ring keys are compared bit for bit, distances within 1e-12 (the
reference's dots go through BLAS), yaws and exception classes exactly.  The CPU oracle (oracle/sc_oracle.c), pinned
to that fixture by test_scancontext_cpu.py, carries the shapes the reference is too slow or too loosely defined for
(ties): every comparison with it is bit for bit.
"""
import os

import numpy as np
import pytest

from helpers import GOLDEN, synth_lidar_cloud, synth_scancontexts

pytestmark = pytest.mark.gpu

G13 = np.load(os.path.join(GOLDEN, "sc_edges_g13.npz"))
DESC_NAMES = [str(n) for n in G13["desc_names"]]
KEYS = ("cand", "cdist", "cyaw", "best_idx", "best_sim", "best_yaw")
EXC = {"IndexError": IndexError, "ValueError": ValueError}
# one call raises once: with a theta == 360 point and a NaN index in the same call the kernels' answer is ValueError,
# whichever comes first in the cloud (include/cslam_hip.h; the reference raises at the first of the two)
BOTH_BITS = ("theta_360_then_inf_x", "inf_x_then_360")
MESSAGE = {IndexError: "out of bounds", ValueError: "cannot convert float NaN to integer"}


def new_matcher(**kw):
    from cslam_amd.lidar_pr.scancontext_matching import ScanContextMatching
    return ScanContextMatching(**kw)


def assert_same(d, o, rows=slice(None), what=""):
    for key in KEYS:
        assert np.array_equal(d[key], o[key][rows]), (what, key)


def oracle_search(bank, q, C, row_limit=None):
    from oracle import pyoracle
    return pyoracle.sc_search(bank, q, C, row_limit=row_limit)


# ---- sc_from_cloud_kernel ----------------------------------------------------------------------------------
def desc_case(name):
    k = "desc/%s/" % name
    exc = EXC[str(G13[k + "exc"])] if k + "exc" in G13 else None
    if name in BOTH_BITS:
        exc = ValueError
    return (G13[k + "pts"], [int(v) for v in G13[k + "shape"]], float(G13[k + "max_length"]),
            G13[k + "sc"] if k + "sc" in G13 else None, exc)


@pytest.mark.parametrize("name", DESC_NAMES)
def test_descriptor_case_compute_embedding(name):
    from cslam_amd.lidar_pr.scancontext import ScanContext
    from oracle import pyoracle
    pts, shape, ml, sc, exc = desc_case(name)
    ex = ScanContext({}, None)
    ex.shape, ex.max_length = shape, ml
    if exc is not None:
        with pytest.raises(exc, match=MESSAGE[exc]):
            ex.compute_embedding(pts)
        with pytest.raises(EXC[str(G13["desc/%s/exc" % name])]):       # the oracle follows the cloud's order
            pyoracle.ptcloud2sc(pts, shape, ml)
        return
    d = ex.compute_embedding(pts).reshape(shape)
    assert np.array_equal(d, sc)
    assert np.array_equal(d, pyoracle.ptcloud2sc(pts, shape, ml))


def test_descriptor_cases_through_ingest():
    """The same upload feeds the voxel filter: every case of the default shape, the good ones as one batch.  `ingest` has
    the paper's 20 x 60 bins and 80 m built in, so the three cases of another shape cannot go through it."""
    from cslam_amd.lidar_pr import keyframes
    good, bad, left_out = [], [], []
    for name in DESC_NAMES:
        pts, shape, ml, sc, exc = desc_case(name)
        if shape == [20, 60] and ml == 80:
            (good if exc is None else bad).append((name, pts, sc, exc))
        else:
            left_out.append(name)
    assert left_out == ["shape_1x1", "shape_3x7", "shape_32x64"]
    assert len(good) == 48 and len(bad) == 11
    desc, down = keyframes.ingest([c[1] for c in good], 100.0)           # voxels of 100 m: the far points fit 2^21 of them
    assert len(down) == len(good)
    for i, (name, _, sc, _) in enumerate(good):
        assert np.array_equal(desc[i].reshape(20, 60), sc), name
    for name, pts, _, exc in bad:
        with pytest.raises(exc, match=MESSAGE[exc]):
            keyframes.ingest([good[0][1], pts, good[1][1]], 100.0)
    desc1, _ = keyframes.ingest([good[0][1]], 100.0)                     # a failed call leaves nothing behind
    assert np.array_equal(desc1[0].reshape(20, 60), good[0][2])


def test_descriptor_batch_equals_singles_and_oracle():
    """Empty frames first, in the middle and last; one point; 1023 / 1024 / 1025 points (the kernel's chunk); frames
    that start at offsets which are no multiple of 1024."""
    from cslam_amd.lidar_pr.scancontext import ScanContext
    from cslam_amd.lidar_pr import keyframes
    from oracle import pyoracle
    sizes = [0, 1, 1023, 0, 1025, 1024, 3000, 0]
    clouds = []
    for i, n in enumerate(sizes):
        rng = np.random.default_rng(700 + i)
        c = synth_lidar_cloud(rng, n, True).astype(np.float64) if n > 3 else np.array([[3.0, -4.0, 1.0]])[:n]
        clouds.append(c + rng.random(c.shape) * 1e-7 * (n > 3))            # genuine float64 coordinates
    starts = np.cumsum([0] + sizes[:-1])
    assert starts[2] % 1024 and starts[4] % 1024 == 0 and starts[5] % 1024 and starts[6] % 1024
    ex = ScanContext({}, None)
    batch = ex.compute_embeddings(clouds)
    desc, _ = keyframes.ingest(clouds, 0.5)
    assert batch.shape == (8, 1200)
    for i, c in enumerate(clouds):
        assert np.array_equal(batch[i], ex.compute_embedding(c)), i
        assert np.array_equal(batch[i].reshape(20, 60), pyoracle.ptcloud2sc(c.reshape(-1, 3))), i
        assert np.array_equal(batch[i], desc[i]), i
    assert not batch[0].any() and not batch[3].any() and not batch[7].any()
    assert np.count_nonzero(batch[1]) == 1 and batch[1].reshape(20, 60)[1, 51] == 3.0


# ---- sc_prep_kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [int(s) for s in G13["rk_sectors"]])
def test_ring_keys_equal_numpy_mean(S):
    from oracle import pyoracle
    sc, rk = G13["rk/%d/sc" % S], G13["rk/%d/rk" % S]
    rng = np.random.default_rng(800 + S)
    more = (rng.random((40, 4, S)) + 1.0) * np.exp2(rng.integers(-12, 13, size=(40, 4, S))) * \
        rng.choice([-1.0, 1.0], size=(40, 4, S))
    more[3] = 0.0
    more[4, :, S // 2:] = 0.0
    m = new_matcher(shape=[4, S], num_candidates=3)
    m.add_item(sc[None].reshape(-1), "fixture")
    m.add_items(more, range(40))
    got = m.ringkeys[:41]
    assert np.array_equal(got[0], rk)                                    # the recorded np.mean(sc, axis=1)
    assert np.array_equal(got[1:], np.stack([np.mean(x, axis=1) for x in more]))
    assert np.array_equal(got[1:], np.stack([pyoracle.sc_ringkey(x) for x in more]))
    bank = np.concatenate([sc[None], more])
    assert np.array_equal(m.scancontexts[:41], bank)
    assert_same(m.search_diagnostics(bank[:5]), oracle_search(bank, bank[:5], 3), what=S)   # column norms, too


# ---- sc_distance_kernel and sc_pick_kernel -----------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 63, 64])
@pytest.mark.parametrize("group", [str(g) for g in G13["dist_groups"]])
def test_recorded_distances_at_every_candidate_count(group, C):
    ctx, D, Y = G13["dist/%s/ctx" % group], G13["dist/%s/D" % group], G13["dist/%s/Y" % group]
    m_ctx, (R, S) = len(ctx), ctx.shape[1:]
    seen = set()
    for n in sorted({1, C - 1, C, C + 1}):
        bank = ctx[np.arange(n) % m_ctx]
        m = new_matcher(shape=[R, S], num_candidates=C)
        m.add_items(bank, range(n))
        d = m.search_diagnostics(ctx)
        assert_same(d, oracle_search(bank, ctx, C), what=(group, C, n))
        assert np.all((d["cand"] >= 0).sum(axis=1) == min(n, C))
        for j in range(m_ctx):
            for c in range(C):
                row = d["cand"][j, c]
                if row < 0:
                    assert d["cdist"][j, c] == 1.0 and d["cyaw"][j, c] == 0
                    continue
                i = int(row) % m_ctx
                seen.add((i, j))
                assert abs(d["cdist"][j, c] - D[i, j]) <= 1e-12, (group, C, n, i, j)
                assert d["cyaw"][j, c] == Y[i, j], (group, C, n, i, j)
            # sc_pick: the first strict minimum below 1.0 in candidate order
            ok = d["cand"][j] >= 0
            dist = np.where(ok, d["cdist"][j], 1.0)
            if dist.min() < 1.0:
                c0 = int(np.argmin(dist))
                assert d["best_idx"][j] == d["cand"][j, c0] and d["best_yaw"][j] == d["cyaw"][j, c0]
                assert d["best_sim"][j] == 1.0 - dist[c0]
            else:
                assert d["best_idx"][j] == -1 and d["best_sim"][j] == 0.0 and d["best_yaw"][j] == 0
    if C >= m_ctx:
        assert len(seen) == m_ctx * m_ctx                                # every recorded pair was met


# ---- stage 1 (sc_knn_kernel, sc_knn_tile_kernel<20,8>) and the merge ----------------------------------------
STAGE1_C = 10


def chunk_rows(n):
    """Rows per stage-1 workgroup: ceil(n / G) with G = ceil(n / 2048) (the chip has more CUs than that)."""
    G = -(-n // 2048)
    return -(-n // G)


def stage1_limits(n, C):
    per = chunk_rows(n)
    return [-3, 0, 1, C - 1, C, per - 1, per, per + 1, n, n + 5]


@pytest.fixture(scope="module", params=[2047, 2048, 2049, 4097, 6145])
def stage1(request):
    """One bank per size, 17 queries, the oracle's answers without and with row limits: shared by the tests below."""
    n = request.param
    rng = np.random.default_rng(n)
    bank = synth_scancontexts(rng, n, 20, 4)
    q = bank[rng.integers(0, n, size=17)] + rng.random((17, 20, 4)) * 1e-3
    q[5] = bank[n - 1]
    q[6] = bank[chunk_rows(n) - 1] if n > 2048 else bank[0]
    lims = stage1_limits(n, STAGE1_C)
    lim = np.array([lims[(3 * j) % 10] for j in range(17)], dtype=np.int64)      # 3 and 10 coprime: all ten are used
    m = new_matcher(shape=[20, 4], num_candidates=STAGE1_C)
    m.add_items(bank, range(n))
    return dict(n=n, q=q, lim=lim, m=m, free=oracle_search(bank, q, STAGE1_C),
                limited=oracle_search(bank, q, STAGE1_C, row_limit=lim))


@pytest.mark.parametrize("nq", [1, 7, 8, 9, 15, 17])
def test_stage1_batch_sizes(stage1, nq):
    """nq < 8 runs sc_knn_kernel, nq >= 8 the 8-query tiles, 9 / 15 / 17 with a partial last tile."""
    m, q, lim = stage1["m"], stage1["q"], stage1["lim"]
    for off in (0, 17 - nq):                                             # the first nq queries, and the last nq
        rows = slice(off, off + nq)
        assert_same(m.search_diagnostics(q[rows]), stage1["free"], rows, (nq, off))
        assert_same(m.search_diagnostics(q[rows], row_limit=lim[rows]), stage1["limited"], rows, (nq, off, "limit"))


def test_stage1_alone_equals_batch(stage1):
    m, q, lim = stage1["m"], stage1["q"], stage1["lim"]
    batch = m.search_diagnostics(q)
    batch_lim = m.search_diagnostics(q, row_limit=lim)
    for j in range(17):
        assert_same(m.search_diagnostics(q[j:j + 1]), batch, slice(j, j + 1), j)
        assert_same(m.search_diagnostics(q[j:j + 1], row_limit=lim[j:j + 1]), batch_lim, slice(j, j + 1), (j, "limit"))
    assert_same(batch, stage1["free"])
    assert_same(batch_lim, stage1["limited"])


def test_stage1_every_row_limit_on_every_path(stage1):
    """Each of the ten limits on the same query, so that whole chunks are hidden from both kernels."""
    n, m, q = stage1["n"], stage1["m"], stage1["q"]
    lims = np.array(stage1_limits(n, STAGE1_C), dtype=np.int64)
    for j in (5, 6):                                                     # the queries that sit on a chunk's last row
        qq = np.repeat(q[j:j + 1], 10, axis=0)
        o = oracle_search(m.scancontexts[:n], qq, STAGE1_C, row_limit=lims)
        assert_same(m.search_diagnostics(qq, row_limit=lims), o, what=("tiled", j))
        assert_same(m.search_diagnostics(qq[:7], row_limit=lims[:7]), o, slice(0, 7), ("plain", j))
        assert_same(m.search_diagnostics(qq[3:], row_limit=lims[3:]), o, slice(3, 10), ("plain", j))
        visible = np.clip(lims, 0, n)
        assert np.array_equal((o["cand"] >= 0).sum(axis=1), np.minimum(visible, STAGE1_C))
        assert np.all(o["cand"] < np.maximum(visible, 1)[:, None])


# ---- ties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 10, 64])
def test_standing_still_bank_of_identical_rows(C):
    rng = np.random.default_rng(31)
    row = synth_scancontexts(rng, 1, 6, 12)[0] + 0.125
    bank = np.repeat(row[None], 300, axis=0)
    q = np.stack([row, np.roll(row, 5, axis=1), synth_scancontexts(rng, 1, 6, 12)[0] + 0.125] * 3)     # 9: no tiles at R = 6
    m = new_matcher(shape=[6, 12], num_candidates=C)
    m.add_items(bank, range(300))
    lim = np.array([300, 300, 300, 299, 65, 64, C, 1, 256], dtype=np.int64)
    for row_limit in (None, lim):
        d = m.search_diagnostics(q, row_limit=row_limit)
        assert_same(d, oracle_search(bank, q, C, row_limit=row_limit), what=C)
        vis = np.full(9, 300) if row_limit is None else lim
        for j in range(9):
            k = min(C, int(vis[j]))
            assert np.array_equal(d["cand"][j, :k], np.arange(k)) and np.all(d["cand"][j, k:] == -1)
            assert np.all(d["cdist"][j, :k] == d["cdist"][j, 0]) and np.all(d["cyaw"][j, :k] == d["cyaw"][j, 0])
        assert np.all(d["best_idx"] == 0)                                # the first of the equal minima
        assert d["best_sim"][0] == 1.0 - d["cdist"][0, 0] and d["cdist"][0, 0] < 1e-15 and d["best_yaw"][0] == 12
        assert d["best_yaw"][1] == 5


@pytest.mark.parametrize("C", [3, 10])
def test_ties_across_lanes_waves_and_chunks(C):
    """Identical rows straddling rows 63|64 (lanes), 255|256 (the four waves' stride), per-1|per and 2per-1|2per (chunks),
    n-2|n-1, and one copy a chunk away; queried by the duplicated row itself (d2 = 0) and by a neighbour of it (equal
    non-zero distances), through both stage-1 kernels, with limits that cut the runs."""
    n = 4097
    per = chunk_rows(n)
    assert per == 1366
    rng = np.random.default_rng(41)
    bank = synth_scancontexts(rng, n, 20, 4) + 0.25
    groups = [[63, 64, 3000], [255, 256], list(range(per - 2, per + 3)), list(range(2 * per - 2, 2 * per + 2)),
              [n - 2, n - 1, 0]]
    for g in groups:
        bank[g] = bank[g[0]]
    q = np.stack([bank[g[0]] for g in groups] + [bank[g[0]] + rng.random((20, 4)) * 1e-6 for g in groups])
    m = new_matcher(shape=[20, 4], num_candidates=C)
    m.add_items(bank, range(n))
    o = oracle_search(bank, q, C)
    for j, g in enumerate(groups):                                       # the tie group first, smaller rows first
        k = min(C, len(g))
        assert list(o["cand"][j, :k]) == sorted(g)[:k] and list(o["cand"][j + 5, :k]) == sorted(g)[:k]
        assert o["best_idx"][j] == min(g)
    assert_same(m.search_diagnostics(q), o, what="tiled")
    assert_same(m.search_diagnostics(q[:5]), o, slice(0, 5), "plain")
    assert_same(m.search_diagnostics(q[5:]), o, slice(5, 10), "plain")
    lim = np.array([64, 256, per, 2 * per, n - 1, 3000, 255, per - 1, 2 * per + 1, n], dtype=np.int64)
    ol = oracle_search(bank, q, C, row_limit=lim)
    assert ol["cand"][0, 0] == 63 and ol["cand"][0, 1] != 64 and ol["cand"][2, 1] == per - 1
    assert_same(m.search_diagnostics(q, row_limit=lim), ol, what="tiled, limits")
    assert_same(m.search_diagnostics(q[:5], row_limit=lim[:5]), ol, slice(0, 5), "plain, limits")
    assert_same(m.search_diagnostics(q[5:], row_limit=lim[5:]), ol, slice(5, 10), "plain, limits")


@pytest.mark.parametrize("name", [str(n) for n in G13["dup_names"]])
def test_recorded_duplicate_rows(name):
    """The reference's own answers on banks with identical rows; which duplicate it names is not defined, so those
    entries are compared with the rule (smaller row first) through the oracle, everything else with the record."""
    k = "dup/%s/" % name
    bank, q, C, tie = G13[k + "bank"], G13[k + "q"], int(G13[k + "ncand"]), G13[k + "tie"]
    m = new_matcher(shape=list(bank.shape[1:]), num_candidates=C)
    m.add_items(bank, range(len(bank)))
    d = m.search_diagnostics(q)
    assert_same(d, oracle_search(bank, q, C), what=name)
    out = G13[k + "cands"] == -2
    assert np.all(out.sum(axis=1) <= len(tie))
    assert np.array_equal(d["cand"][~out], G13[k + "cands"][~out]) and np.all(np.isin(d["cand"][out], tie))
    assert np.abs(d["cdist"] - G13[k + "dists"]).max() <= 1e-12
    assert np.array_equal(d["cyaw"], G13[k + "yaws"])
    assert np.abs(d["best_sim"] - G13[k + "sims"]).max() <= 1e-12
    for j in range(len(q)):
        items, sims = m.search(q[j].reshape(-1), 1)
        assert abs(sims[0] - G13[k + "sims"][j]) <= 1e-12


# ---- cslam_scbank_search_host: chunks of 16384 queries -------------------------------------------------------
def test_host_search_second_chunk_offsets():
    rng = np.random.default_rng(51)
    nq = 16385
    bank = np.round(rng.random((5, 2, 3)) * 64) / 16.0
    pool = np.round(rng.random((11, 2, 3)) * 64) / 16.0
    pool[3] = 0.0
    q = pool[np.arange(nq) % 11]
    q[-1] = bank[4]                                                      # the one query of the second chunk
    lim = (np.arange(nq) % 8 - 1).astype(np.int64)                       # -1 .. 6
    lim[-1] = 5
    m = new_matcher(shape=[2, 3], num_candidates=3)
    m.add_items(bank, range(5))
    assert_same(m.search_diagnostics(q, row_limit=lim), oracle_search(bank, q, 3, row_limit=lim))
    d = m.search_diagnostics(q)
    assert_same(d, oracle_search(bank, q, 3))
    assert d["best_idx"][-1] == 4 and d["cand"][-1, 0] == 4 and d["best_yaw"][-1] == 3


# ---- growth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["add_item", "add_items"])
def test_growth_keeps_the_bank(how):
    """1000 -> 2000 -> 4000 rows of capacity: nothing stored is lost and a search right after growing is right."""
    rng = np.random.default_rng(61)
    bank = np.round(rng.random((2001, 2, 3)) * 1024) / 256.0
    q = bank[[0, 998, 999, 1000, 1999, 2000]] + rng.random((6, 2, 3)) * 1e-3
    m = new_matcher(shape=[2, 3], num_candidates=4)
    have = 0
    for n, cap in ((999, 1000), (1000, 1000), (1001, 2000), (2000, 2000), (2001, 4000)):
        if how == "add_item":
            for i in range(have, n):
                m.add_item(bank[i].reshape(-1), i)
        else:
            m.add_items(bank[have:n], range(have, n))
        have = n
        sc, rk = m.scancontexts, m.ringkeys
        assert m.nb_items == n and sc.shape == (cap, 2, 3) and rk.shape == (cap, 2)
        assert np.array_equal(sc[:n], bank[:n]) and not sc[n:].any()
        assert np.array_equal(rk[:n], np.stack([np.mean(x, axis=1) for x in bank[:n]]))
        assert_same(m.search_diagnostics(q), oracle_search(bank[:n], q, 4), what=(how, n))


# ---- the shapes a search can serve -------------------------------------------------------------------------
def lds_bytes(R, S):
    return 8 * (2 * R * S + 3 * S + S * (S + 1))


@pytest.mark.parametrize("R,S", [(64, 64), (8, 128), (14, 128), (64, 91)])
def test_largest_shapes_are_searched(R, S):
    assert lds_bytes(R, S) <= 160 * 1024
    rng = np.random.default_rng(R * 1000 + S)
    bank = synth_scancontexts(rng, 6, R, S)
    bank[5] = bank[2]
    q = np.stack([np.roll(bank[2], S - 1, axis=1), np.roll(bank[4], 1, axis=1), np.zeros((R, S))])
    m = new_matcher(shape=[R, S], num_candidates=4)
    m.add_items(bank, range(6))
    d = m.search_diagnostics(q)
    assert_same(d, oracle_search(bank, q, 4), what=(R, S))
    assert d["best_idx"][0] == 2 and d["best_yaw"][0] == S - 1 and d["best_yaw"][1] == 1 and d["best_idx"][2] == -1


@pytest.mark.parametrize("R,S", [(20, 128), (64, 128), (15, 128), (64, 92), (0, 60), (65, 4), (20, 0), (2, 129)])
def test_unsearchable_shapes_are_refused_at_create(R, S):
    from cslam_amd._lib import CslamHipError
    assert not (1 <= R <= 64 and 1 <= S <= 128) or lds_bytes(R, S) > 160 * 1024
    with pytest.raises(CslamHipError, match="invalid argument") as e:
        new_matcher(shape=[R, S])
    if 1 <= R <= 64 and 1 <= S <= 128:
        assert "LDS" in str(e.value) and "163840" in str(e.value)
