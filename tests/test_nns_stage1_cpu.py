"""The float64 checker of the candidate stage's contract (tests/stage1_reference.py) must bite: a model stage 1 built in numpy
from the exact keys (the true top 16 of every segment, the 17th as the drop bound) passes, and every single mutation of it that
a wrong kernel could produce is rejected, with its own clause named.  Runs without a GPU; tests/test_nns_stage1_gpu.py then
holds the real kernels to the same checker."""
import numpy as np
import pytest

from cslam_amd import _lib
from helpers import unit_rows
import stage1_reference as s1

EB = 1e-5           # the model's keys are the exact ones rounded to float32 (2^-24 relative): far inside this


def model_stage1(bank, q, lim, segs, tile, nseg):
    b64, q64 = bank.astype(np.float64), q.astype(np.float64)
    bn = np.sqrt((b64 * b64).sum(axis=1))
    nq = q.shape[0]
    keys = np.full((nq, nseg, s1.KP), -np.inf, dtype=np.float32)
    rows = np.full((nq, nseg, s1.KP), -1, dtype=np.int32)
    bounds = np.full((nq, nseg), -np.inf, dtype=np.float32)
    for j in range(nq):
        x = s1.exact_keys(b64, bn, q64[j:j + 1])[0]
        for l, R in enumerate(segs[j // tile]):
            V = R[R < lim[j]]
            o = V[np.argsort(-x[V], kind="stable")]
            m = min(len(o), s1.KP)
            keys[j, l, :m], rows[j, l, :m] = x[o[:m]], o[:m]
            if len(o) > s1.KP:
                bounds[j, l] = np.nextafter(np.float32(x[o[s1.KP]]), np.float32(np.inf))      # rounded up: still a bound
    return keys, rows, bounds


@pytest.fixture(scope="module")
def model():
    rng = np.random.default_rng(11)
    n, d, nq, tile = 1100, 48, 200, 128
    bank = unit_rows(rng, n, d) * np.exp2(rng.integers(-6, 7, size=(n, 1))).astype(np.float32)
    q = unit_rows(rng, nq, d) * np.float32(3.0)
    lim = rng.integers(0, n + 1, size=nq).astype(np.int64)
    lim[:6] = [0, 1, 8, 9, 300, n]
    lim[130], lim[131] = n, 450
    segs = s1.tiled_segments(2, n, 4, 1, 300)              # rows [0, 300) [300, 600) [600, 900) [900, 1100)
    keys, rows, bounds = model_stage1(bank, q, lim, segs, tile, 4)
    b64, q64 = bank.astype(np.float64), q.astype(np.float64)
    x = s1.exact_keys(b64, np.sqrt((b64 * b64).sum(axis=1)), q64)
    e = (EB + 1e-12) * np.sqrt((q64 * q64).sum(axis=1))
    return dict(bank=bank, q=q, lim=lim, segs=segs, tile=tile, keys=keys, rows=rows, bounds=bounds, x=x, e=e)


def run(m, keys=None, rows=None, bounds=None):
    return s1.check_stage1(m["bank"], m["q"], m["lim"], m["segs"], m["tile"], m["keys"] if keys is None else keys,
                           m["rows"] if rows is None else rows, m["bounds"] if bounds is None else bounds, EB)


def test_the_model_stage_passes(model):
    st = run(model)
    assert st["max_err"] < 2.0 ** -23 and st["min_slack_sound"] >= 1.0 and st["min_slack_loss"] > 1.0
    # without limits, and on the lists of the persistent stage's schedule (five query tiles of 256, per-tile list counts)
    lib = _lib.load()
    rng = np.random.default_rng(12)
    bank, q = unit_rows(rng, 1500, 20), unit_rows(rng, 1100, 20)
    segs = s1.ring_segments(lib, 5, 1500, 8, 32)
    nseg = max(len(s) for s in segs)
    lim = np.full(1100, 1500, dtype=np.int64)
    keys, rows, bounds = model_stage1(bank, q, lim, segs, 256, nseg)
    s1.check_stage1(bank, q, None, segs, 256, keys, rows, bounds, EB)
    if min(len(s) for s in segs) < nseg:                    # a list a query tile does not have must stay empty
        qt = int(np.argmin([len(s) for s in segs]))
        bounds[qt * 256 + 3, nseg - 1] = 0.0
        with pytest.raises(s1.Stage1Violation) as ei:
            s1.check_stage1(bank, q, None, segs, 256, keys, rows, bounds, EB)
        assert ei.value.clause == "missing-list" and ei.value.query == qt * 256 + 3


J, L = 130, 1           # a query of the second tile that sees everything, the 300-row segment [300, 600)


def _dropped_row(m, keys, rows, bounds):
    keys[J, L, :-1], rows[J, L, :-1] = m["keys"][J, L, 1:], m["rows"][J, L, 1:]
    keys[J, L, -1], rows[J, L, -1] = -np.inf, -1
    return J, "bound-sound"


def _kept_row_at_the_limit(m, keys, rows, bounds):
    assert m["lim"][131] == 450
    rows[131, L, -1] = 450
    return 131, "kept-in-segment"


def _kept_row_of_the_neighbour(m, keys, rows, bounds):
    rows[J, L, -1] = 600
    return J, "kept-in-segment"


def _row_twice(m, keys, rows, bounds):
    rows[J, L, -1] = rows[J, L, -2]
    return J, "kept-distinct"


def _key_off(m, keys, rows, bounds):
    keys[J, L, 0] = np.float32(m["x"][J, rows[J, L, 0]] + 2.0 * m["e"][J])
    return J, "key-error"


def _out_of_order(m, keys, rows, bounds):
    keys[J, L, [2, 3]], rows[J, L, [2, 3]] = m["keys"][J, L, [3, 2]], m["rows"][J, L, [3, 2]]
    return J, "kept-order"


def _bound_raised(m, keys, rows, bounds):
    x8 = np.sort(m["x"][J, 300:600])[-8]
    bounds[J, L] = np.float32(x8 + 2.0 * m["e"][J])
    return J, "bound-loss"


def _list_cut_to_five(m, keys, rows, bounds):
    bounds[J, L] = keys[J, L, 5]                           # the cut list's bound is sound: only the count is wrong
    keys[J, L, 5:], rows[J, L, 5:] = -np.inf, -1
    return J, "kept-count"


@pytest.mark.parametrize("mutate", [_dropped_row, _kept_row_at_the_limit, _kept_row_of_the_neighbour, _row_twice, _key_off,
                                    _out_of_order, _bound_raised, _list_cut_to_five], ids=lambda f: f.__name__.strip("_"))
def test_every_single_mutation_is_rejected_for_its_own_reason(model, mutate):
    keys, rows, bounds = model["keys"].copy(), model["rows"].copy(), model["bounds"].copy()
    j, clause = mutate(model, keys, rows, bounds)
    with pytest.raises(s1.Stage1Violation) as ei:
        run(model, keys, rows, bounds)
    assert (ei.value.clause, ei.value.query, ei.value.list) == (clause, j, L), str(ei.value)


@pytest.mark.parametrize("nqt,n", [(2, 1100), (5, 20011)])
def test_segment_builders_partition_the_bank_per_query_tile(nqt, n):
    lib = _lib.load()
    cases = [s1.ring_segments(lib, nqt, n, 8, 32), s1.ring_segments(lib, nqt, n, 1, 304)]
    for tile in (128, 256):
        nb = -(-n // tile)
        for tps in (1, 2, 3, nb):
            cases.append(s1.tiled_segments(nqt, n, -(-nb // tps), tps, tile))
    for segs in cases:
        assert len(segs) == nqt
        for per_qt in segs:
            allrows = np.concatenate(per_qt)
            assert np.array_equal(np.sort(allrows), np.arange(n)), "the lists of a query tile do not partition [0, n)"
            assert all(np.all(np.diff(R) > 0) for R in per_qt)
    # segments_from_info reads the same two builders off the library's info words
    segs, tile = s1.segments_from_info(lib, [5, 128, 0, 0, 2, 0, 0, 0], 130, n)
    assert tile == 128 and len(segs) == 2 and segs[0][1][0] == 256 and len(segs[0]) == 5
    segs, tile = s1.segments_from_info(lib, [0, 256, 1, 1, 0, 8, 32, 0], nqt * 256 - 3, n)
    assert tile == 256 and len(segs) == nqt and np.array_equal(np.sort(np.concatenate(segs[-1])), np.arange(n))


def test_bound_formulas_restate_the_library():
    # the values the kernels' comments quote at 4096-D: 1.582e-3 (one product, persistent) against 1.570e-3 (pairs)
    assert abs(s1.stage_err_bound(4096, 1, True) - 1.582e-3) < 2e-6 and abs(s1.stage_err_bound(4096, 3, False) - 1.570e-3) < 2e-6
    assert abs(s1.stage_err_bound(4096, 0, False) - 1.0625 * 4104 * 2.0 ** -24) < 1e-18
    assert s1.stage_err_bound(17, 1, True) - s1.stage_err_bound(64, 1, False) == pytest.approx(1.02 * 2.0 ** -16, rel=1e-9)
