"""The contract of the candidate stage of the batched descriptor search, as a plain float64 checker.

Stage 1 (csrc/sim_topk_mfma.hip, sim_topk_pair.hip, sim_topk_ring.hip) writes, for every query and bank segment, a sorted list
of 16 (key, row) pairs and one drop bound: "upper bound of the key of every row of the segment NOT in the list" (csrc/sim_topk.h).
rescore_kernel builds its certificate on exactly that, so a stage that breaks it is either slow (bounds too high: the exact scan
answers) or wrong (bounds too low: a row of the true top-k can go missing).  `check_stage1` states the contract clause by clause
against x[j, r] = q_j . b_r / ||b_r|| in float64 and names the first violation.

The only tolerance is the stage's own error bound `eb` (|key - x| <= eb ||q||, the value the library hands to the certificate)
plus 1e-12 ||q|| for the rounding of the float64 reference itself.
"""
import ctypes as C

import numpy as np

KP = 16          # merged list length per (query, segment): SIM_KP of csrc/sim_topk.h
MIN_KEPT = 8     # every form keeps per-lane lists of at least 8 entries (KPL), so nothing above a segment's 8th best is dropped

CLAUSES = ("missing-list", "kept-tail", "kept-in-segment", "kept-distinct", "kept-order", "kept-count", "key-error",
           "bound-sound", "bound-loss")


class Stage1Violation(AssertionError):
    def __init__(self, clause, query, lst, detail):
        assert clause in CLAUSES
        self.clause, self.query, self.list = clause, int(query), int(lst)
        super().__init__(f"stage 1 contract, clause '{clause}' at query {int(query)}, list {int(lst)}: {detail}")


# ---- the formulas of the bound the library reports (csrc/sim_topk_pair.hip pair_err_bound, csrc/sim_topk_mfma.hip) -----------
def pair_err_bound(kd, nprod):
    u24, u23 = 2.0 ** -24, 2.0 ** -23
    keyr = 3.0 * u24
    floor_ = np.sqrt(float(kd)) * 2.0 ** -38
    if nprod == 1:
        rep = 2.0 / 2048.0 + 2.0 ** -22 + u24
        accum = 1.002 * (kd + 64.0) * u23
        return 1.0625 * (rep + accum + keyr + floor_)
    u16 = 2.0 ** -22
    rep = 2.0 * (u16 + u24)
    dropped = u16 * (1.0 + 1.0 / 1024.0)
    accum = 1.002 * (3.0 * kd + 64.0) * u23
    return 1.0625 * (rep + dropped + accum + keyr + floor_)


def stage_err_bound(dim, nprod, persistent):
    """|key - exact| / ||q|| of the form `info` names, for descriptors of `dim` channels."""
    kd, kh = (dim + 31) // 32 * 32, (dim + 63) // 64 * 64
    if nprod == 0:
        eb = 1.0625 * (kd + 8.0) * 2.0 ** -24
    else:
        eb = pair_err_bound(kh if nprod == 1 else kd, nprod)
    return eb + (1.02 * 2.0 ** -16 if persistent else 0.0)


# ---- segments: the bank rows of every (query tile, list) ----------------------------------------------------------------------
def tiled_segments(nqt, n, nseg, tps, tile):
    """One workgroup per (query tile, segment): list s covers rows [s tps tile, min((s + 1) tps tile, n))."""
    one = [np.arange(min(s * tps * tile, n), min((s + 1) * tps * tile, n), dtype=np.int64) for s in range(nseg)]
    return [one for _ in range(nqt)]


def ring_schedule(lib, nqt, n, n_xcd, wpx):
    """cslam_ring_schedule_describe -> (tasks [., 8] int32, qt_nseg [nqt])."""
    from cslam_amd import _lib
    info = (C.c_int32 * 6)()
    _lib.check(lib.cslam_ring_schedule_describe(nqt, n, n_xcd, wpx, C.byref(info), None, 0, None, None, None))
    ntask = int(info[2])
    assert int(info[5]) == 8
    tasks = np.zeros((max(ntask, 1), 8), dtype=np.int32)
    qn = np.zeros(nqt, dtype=np.int32)
    _lib.check(lib.cslam_ring_schedule_describe(nqt, n, n_xcd, wpx, C.byref(info), tasks.ctypes.data_as(C.c_void_p), tasks.size,
                                                None, qn.ctypes.data_as(C.c_void_p), None))
    return tasks[:ntask], qn


def ring_segments(lib, nqt, n, n_xcd, wpx):
    """The persistent stage: list `seg` of query tile `qt` covers the rows of the one task (qt, seg):
    [row0 + i stride, min(+ 256, row_end)) for i < n_tiles."""
    tasks, qn = ring_schedule(lib, nqt, n, n_xcd, wpx)
    segs = [[None] * int(qn[qt]) for qt in range(nqt)]
    for qt, row0, ntiles, seg, _run, stride, row_end, _ in tasks:
        assert segs[qt][seg] is None, "two tasks write one list"
        parts = [np.arange(row0 + i * stride, min(row0 + i * stride + 256, row_end), dtype=np.int64) for i in range(ntiles)]
        segs[qt][seg] = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    assert all(s is not None for per_qt in segs for s in per_qt), "a list without a task"
    return segs


def segments_from_info(lib, info, nq, n):
    """info of cslam_debug_last_candidate_bounds -> (segments per (query tile, list), tile edge)."""
    nseg, tile, _nprod, persistent, tps, n_xcd, wpx = (int(v) for v in info[:7])
    nqt = -(-nq // tile)
    if persistent:
        return ring_segments(lib, nqt, n, n_xcd, wpx), tile
    return tiled_segments(nqt, n, nseg, tps, tile), tile


def exact_keys(b64, bn, q64):
    """x[j, r] = q_j . b_r / ||b_r|| in float64 (b64 = the float32 bank in float64, bn = its row norms)."""
    return (q64 @ b64.T) / bn[None, :]


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def check_stage1(bank, queries, lim, segs, tile, keys, rows, bounds, eb):
    """bank [n, d] float32; queries [nq, d]; lim [nq] visible-row limits or None; segs[qt][l] = sorted bank rows of list l of
    query tile qt (`tile` queries per tile); keys / rows [nq, nseg, 16]; bounds [nq, nseg]; eb = the stage's error bound.
    Raises Stage1Violation at the first (clause, query, list) that breaks the contract; returns what it measured:
    max |key - x| / ||q||, the smallest slack of the soundness clause and of the no-needless-loss clause, in units of e_j."""
    b64 = np.asarray(bank, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(queries).astype(np.float64)
    n, nq = b64.shape[0], q64.shape[0]
    bn = np.sqrt((b64 * b64).sum(axis=1))
    qn = np.sqrt((q64 * q64).sum(axis=1))
    e = eb * qn + 1e-12 * qn
    lim = np.full(nq, n, dtype=np.int64) if lim is None else np.clip(np.asarray(lim, dtype=np.int64), 0, n)
    keys = np.asarray(keys, dtype=np.float32).astype(np.float64)
    rows = np.asarray(rows).astype(np.int64)
    bounds = np.asarray(bounds, dtype=np.float32).astype(np.float64)
    nseg = keys.shape[1]
    assert keys.shape == (nq, nseg, KP) and rows.shape == keys.shape and bounds.shape == (nq, nseg)
    stats = {"max_err": 0.0, "min_slack_sound": np.inf, "min_slack_loss": np.inf}

    def fail(clause, bad, j0, l, detail):
        j = int(np.argmax(bad))
        raise Stage1Violation(clause, j0 + j, l, detail(j))

    for qt in range(-(-nq // tile)):
        j0, j1 = qt * tile, min((qt + 1) * tile, nq)
        nj = j1 - j0
        x_qt = exact_keys(b64, bn, q64[j0:j1])
        e_j, lim_j = e[j0:j1], lim[j0:j1]
        assert len(segs[qt]) <= nseg
        for l in range(nseg):
            k_, r_, bd = keys[j0:j1, l], rows[j0:j1, l], bounds[j0:j1, l]
            valid = r_ >= 0
            if l >= len(segs[qt]):          # uniform layout of the persistent stage: a list this query tile does not have
                bad = valid.any(axis=1) | (k_ != -np.inf).any(axis=1) | (bd != -np.inf)
                if bad.any():
                    fail("missing-list", bad, j0, l, lambda j: f"rows {r_[j]}, bound {bd[j]}")
                continue
            R = segs[qt][l]
            xs = x_qt[:, R]                                         # [nj, |R|]
            vis = R[None, :] < lim_j[:, None]
            nv = vis.sum(axis=1)
            # 1. kept rows
            bad = (valid[:, 1:] & ~valid[:, :-1]).any(axis=1) | (~valid & (k_ != -np.inf)).any(axis=1) | (r_ < -1).any(axis=1)
            if bad.any():
                fail("kept-tail", bad, j0, l, lambda j: f"rows {r_[j]}, keys {k_[j]}: -1 only at the tail, with key -inf")
            pos = np.searchsorted(R, r_) if len(R) else np.zeros_like(r_)
            pos_c = np.minimum(pos, max(len(R) - 1, 0))
            in_seg = (R[pos_c] == r_) if len(R) else np.zeros_like(valid)
            outside = valid & ~(in_seg & (r_ < lim_j[:, None]) & (r_ < n))
            if outside.any():
                bad = outside.any(axis=1)
                fail("kept-in-segment", bad, j0, l,
                     lambda j: f"row {r_[j][outside[j]][0]} (limit {lim_j[j]}, n {n}, segment rows {R[0] if len(R) else '-'}"
                               f"..{R[-1] if len(R) else '-'})")
            srt = np.sort(np.where(valid, r_, -1 - np.arange(KP)[None, :]), axis=1)
            bad = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
            if bad.any():
                fail("kept-distinct", bad, j0, l, lambda j: f"rows {r_[j]}")
            bad = (k_[:, 1:] > k_[:, :-1]).any(axis=1) | np.isnan(k_).any(axis=1)
            if bad.any():
                fail("kept-order", bad, j0, l, lambda j: f"keys {k_[j]}")
            nkept = valid.sum(axis=1)
            bad = nkept < np.minimum(MIN_KEPT, nv)
            if bad.any():
                fail("kept-count", bad, j0, l, lambda j: f"{nkept[j]} rows kept of {nv[j]} visible")
            # 2. the keys of the kept rows
            xk = np.take_along_axis(xs, pos_c, axis=1) if len(R) else np.zeros_like(k_)
            err = np.where(valid, np.abs(k_ - xk), 0.0)
            bad = (err > e_j[:, None]).any(axis=1)
            if valid.any():
                stats["max_err"] = max(stats["max_err"], float((err / qn[j0:j1, None]).max()))
            if bad.any():
                fail("key-error", bad, j0, l, lambda j: f"|key - exact| = {err[j].max():.3e} > e = {e_j[j]:.3e}")
            # 3. soundness: nothing visible and unkept lies above the bound
            kept = np.zeros((nj, len(R)), dtype=bool)
            jj, cc = np.nonzero(valid)
            kept[jj, pos_c[jj, cc]] = True
            unkept = vis & ~kept
            has_unkept = unkept.any(axis=1)
            top_unkept = np.where(unkept, xs, -np.inf).max(axis=1) if len(R) else np.full(nj, -np.inf)
            bad = has_unkept & ~np.isfinite(bd)
            if bad.any():
                fail("bound-sound", bad, j0, l, lambda j: f"bound {bd[j]} with {int(unkept[j].sum())} visible rows not kept")
            with np.errstate(invalid="ignore"):                    # -inf - -inf where nothing is unkept
                slack = np.where(has_unkept, bd - (top_unkept - e_j), np.inf)
            bad = slack < 0.0
            if has_unkept.any():
                stats["min_slack_sound"] = min(stats["min_slack_sound"], float((slack / e_j)[has_unkept].min()))
            if bad.any():
                fail("bound-sound", bad, j0, l,
                     lambda j: f"bound {bd[j]!r} < best unkept key {top_unkept[j]!r} - e ({e_j[j]:.3e}): row "
                               f"{R[int(np.argmax(np.where(unkept[j], xs[j], -np.inf)))]}")
            # 4. no needless loss: whatever a correct stage drops lies at or below the 8th best of the segment
            few = nv <= MIN_KEPT
            bad = few & (bd != -np.inf)
            if bad.any():
                fail("bound-loss", bad, j0, l, lambda j: f"bound {bd[j]} with only {nv[j]} visible rows: nothing can be dropped")
            if len(R) >= MIN_KEPT and (~few).any():
                x8 = -np.partition(np.where(vis, -xs, np.inf), MIN_KEPT - 1, axis=1)[:, MIN_KEPT - 1]
                with np.errstate(invalid="ignore"):
                    slack = np.where(few, np.inf, (x8 + e_j) - bd)
                bad = slack < 0.0
                stats["min_slack_loss"] = min(stats["min_slack_loss"], float((slack / e_j)[~few].min()))
                if bad.any():
                    fail("bound-loss", bad, j0, l, lambda j: f"bound {bd[j]!r} > 8th best of the segment {x8[j]!r} + e ({e_j[j]:.3e})")
    return stats


def certification_gap(bank, queries, lim, eb, chunk=256):
    """The precondition of the k = 1 certification test, in float64 alone: for every query that sees at least 8 rows,
    ((best key) - (8th best key over ALL visible rows)) / e_j; returns the smallest (inf when no query sees 8 rows)."""
    b64 = np.asarray(bank, dtype=np.float32).astype(np.float64)
    q64 = np.asarray(queries).astype(np.float64)
    n, nq = b64.shape[0], q64.shape[0]
    bn = np.sqrt((b64 * b64).sum(axis=1))
    qn = np.sqrt((q64 * q64).sum(axis=1))
    e = eb * qn + 1e-12 * qn
    lim = np.full(nq, n, dtype=np.int64) if lim is None else np.clip(np.asarray(lim, dtype=np.int64), 0, n)
    gap = np.inf
    for j0 in range(0, nq, chunk):
        j1 = min(j0 + chunk, nq)
        x = exact_keys(b64, bn, q64[j0:j1])
        x = np.where(np.arange(n)[None, :] < lim[j0:j1, None], x, -np.inf)
        top = -np.partition(-x, MIN_KEPT - 1, axis=1)[:, :MIN_KEPT]
        sees = lim[j0:j1] >= MIN_KEPT
        if sees.any():
            gap = min(gap, float(((top[sees].max(axis=1) - top[sees].min(axis=1)) / e[j0:j1][sees]).min()))
    return gap
