"""The candidate stage of the batched descriptor search, held to its written contract on the GPU (run with -m gpu on an MI355X).

Every form of stage 1 -- the f32-input MFMA kernel, the fp16-pair kernel with three products and with one, each on 128- and
256-row tiles, and the persistent one-product kernel with its packed lists -- writes per (query, bank segment) a sorted list of
16 (key, row) pairs and a drop bound.  The end-to-end tests cannot see a wrong stage 1: lost rows or high bounds make the
certificate refuse and the exact scan answers; a low bound is wrong only for the rare query whose top-k holds the dropped row.
Here every (query, list) of every case is checked by tests/stage1_reference.py against float64: the kept rows, their keys, the
soundness of the bound and that it is no higher than a correct stage can make it.  The only tolerance is the error bound the
library itself hands to the certificate, and that value is asserted to equal its formula.

Forms are reached by shape alone (CSLAM_MFMA_TILE is latched once per process and is left alone); which form ran is read from
cslam_debug_last_candidate_bounds' info words and asserted.  The one-product kernel on 256-row tiles WITHOUT the persistent
schedule cannot be reached in the default build (it needs a chip of fewer than 8 CUs or the measurement build's switch) and is
left out.

Every line printed here (run with -s) is one search: form, measured max |key - exact| / ||q|| next to the bound, the smallest
slack of the soundness clause and of the no-needless-loss clause in units of e_j, and the certification precondition's gap.
"""
import functools

import numpy as np
import pytest

from helpers import assert_topk_equal, stage1_bounds, stage1_candidates, unit_rows
from oracle import pyoracle
import stage1_reference as s1

pytestmark = pytest.mark.gpu

SEED = 5
# (n, d, nq): the smallest shapes at which each form's edges exist
S_128_ONE = (300, 96, 130)          # 128-row tiles, one tile per segment, ragged last bank tile (44 rows) and second query tile, d % 64 != 0
S_128_MANY = (40037, 64, 130)       # 128-row tiles, segments of several tiles
S_256_D17 = (1100, 17, 300)         # 256-row tiles (h1: persistent), five bank tiles, the last of 76 rows, 44 queries in the second tile
S_256_D96 = (1100, 96, 300)
S_256_MANY = (20011, 64, 1100)      # 256-row tiles, tasks of several tiles, several lists per query tile
SHAPES = (S_128_ONE, S_128_MANY, S_256_D17, S_256_D96, S_256_MANY)
NPROD = {"h1": 1, "pair": 3, "f32": 0}
CASES = [(shape, kind, False) for shape in SHAPES for kind in ("unit", "scaled", "ties")] + [(S_256_D96, "unit", True)]


@pytest.fixture(scope="module")
def nnm():
    from cslam_amd import nns_matching
    return nns_matching


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, f64):
    """(bank, queries, limits): finite, non-zero rows (zero and non-finite rows have their own tests in test_nns_gpu.py)."""
    n, d, nq = shape
    rng = np.random.default_rng(SEED)
    bank, q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    lim = rng.integers(0, n + 1, size=nq).astype(np.int64)
    lim[:11] = [0, 1, 7, 8, 9, 33, 255, 256, 257, n - 1, n]
    if kind == "scaled":            # rows of very different norms, values spread over six binades inside a row (keys are scale-free)
        bank = bank * np.exp2(rng.integers(-5, 1, size=(n, d))).astype(np.float32)
        bank = bank * np.exp2(rng.integers(-20, 21, size=(n, 1))).astype(np.float32)
        q = q * np.exp2(rng.integers(-20, 21, size=(nq, 1))).astype(np.float32)
    if kind == "ties":              # 40 exact ties across the 256-row boundary, eight queries that rank them first
        bank[250:290] = bank[250]
        q[20:28] = bank[250]
    if f64:                         # queries that are not float32 numbers
        q = np.random.default_rng(SEED + 1).standard_normal((nq, d))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    for a in (bank, q, lim):
        a.setflags(write=False)
    return bank, q, lim


@functools.lru_cache(maxsize=None)
def oracle(shape, kind, f64, run, k):
    bank, q, lim = inputs(shape, kind, f64)
    return pyoracle.nns_search(bank, q, k, row_limit=limits_of(run, lim))


def limits_of(run, lim):
    if run == "all":
        return None
    if run == "limits":
        return lim
    lim0 = lim.copy()               # "tile0": the whole second query tile sees nothing
    lim0[256:] = 0
    return lim0


_banks = {}


def bank_of(nnm, shape, kind, f64):
    key = (shape, kind)
    if key not in _banks:
        _banks.clear()              # one bank on the device at a time
        nn = nnm.NearestNeighborsMatching()
        bank = inputs(shape, kind, f64)[0]
        nn.add_items(bank, range(bank.shape[0]))
        _banks[key] = nn
    return _banks[key]


@pytest.mark.parametrize("stage", ["h1", "pair", "f32"])
@pytest.mark.parametrize("shape,kind,f64", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_lists_and_drop_bounds_meet_the_contract(nnm, monkeypatch, shape, kind, f64, stage):
    """Clauses 1-4 of tests/stage1_reference.py on every (query, list); the reported error bound equals its formula; the search
    result equals the oracle's; on unit-norm Gaussian input with k = 1 every query is certified (stats[0] == 0) -- given, in
    float64 alone, that its best key leads the 8th best over all visible rows by 3 e_j (the worst segmentation any form could
    use: a correct stage drops nothing above the 8th best + e in key units, 2e in exact score, so the certificate must hold)."""
    monkeypatch.setenv("CSLAM_MFMA_STAGE1", stage)      # read on every call; pinning it also switches the back-off off
    n, d, nq = shape
    bank, q, lim = inputs(shape, kind, f64)
    nn = bank_of(nnm, shape, kind, f64)
    lib = nn._lib
    k = 1 if kind == "unit" else 5
    runs = ["all", "limits"] + (["tile0"] if (shape, kind, f64) == (S_256_D96, "unit", False) else [])
    for run in runs:
        lim_run = limits_of(run, lim)
        idx, sims, cnt = nn.search_batch(q, k, row_limit=lim_run, mode=nnm.MODE_MFMA)
        uncertified, mode = nn.last_stats()[:2]
        assert mode == nnm.MODE_MFMA
        keys, rows, eb = stage1_candidates(nn, nq)
        bounds, info = stage1_bounds(nn, nq)
        nseg, tile, nprod, persistent, tps, n_xcd, wpx = info[:7]
        assert keys.shape[1] == nseg and nprod == NPROD[stage]

        # which form ran
        if shape in (S_128_ONE, S_128_MANY):
            assert (tile, persistent) == (128, 0), info
            if shape == S_128_ONE:
                assert tps == 1 and nseg == 3, info
            else:
                assert tps >= 2, f"{info}: this chip's CU count gives one tile per segment at n = {n}: raise n"
        else:
            assert tile == 256 and persistent == (1 if stage == "h1" else 0), info
            if persistent and shape == S_256_MANY:
                tasks, qn = s1.ring_schedule(lib, -(-nq // 256), n, n_xcd, wpx)
                assert tasks[:, 2].max() >= 2 and qn.max() > 1, "no task of several tiles, or one list per query tile: raise n"

        # the bound handed to the certificate is the formula's, not a looser one
        want_eb = s1.stage_err_bound(d, nprod, persistent)
        assert abs(eb - want_eb) <= 1e-12 * want_eb, (eb, want_eb)

        segs, tile_ = s1.segments_from_info(lib, info, nq, n)
        gap = s1.certification_gap(bank, q, lim_run, eb) if kind == "unit" else float("nan")
        try:
            st = s1.check_stage1(bank, q, lim_run, segs, tile_, keys, rows, bounds, eb)
        except s1.Stage1Violation as v:
            print(f"STAGE1 {stage} {shape} {kind} f64={f64} {run} info={info} VIOLATION {v}")
            raise
        print(f"STAGE1 {stage} {shape} {kind} f64={f64} {run} info={info} max_err={st['max_err']:.4e} eb={eb:.4e} "
              f"slack_sound={st['min_slack_sound']:.4f}e slack_loss={st['min_slack_loss']:.4f}e gap={gap:.2f}e "
              f"uncertified={uncertified}")
        if run == "tile0":
            assert np.all(rows[256:] == -1) and np.all(keys[256:] == -np.inf) and np.all(bounds[256:] == -np.inf)

        oi, os_, oc = oracle(shape, kind, f64, run, k)
        assert_topk_equal(idx, sims, cnt, oi, os_, oc, 1e-12)
        if kind == "unit":
            assert gap >= 3.0, f"precondition: best - 8th best = {gap:.2f} e < 3 e: change SEED (never the 3 e)"
            assert uncertified == 0, f"{uncertified} queries left uncertified by a stage whose input allows every certificate"
