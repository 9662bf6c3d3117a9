"""GPU tests of the Winograd transform kernels, one kernel at a time, against the float64 transform of tests/wino_reference.py (-m gpu):
the F(2x2) and F(4x4) input and output transforms of csrc/winograd.hip, the pair-layout input transform of csrc/wino_gemm.hip, the
chained transform of csrc/wino_chain.hip, the direct layers' epilogue and the max |x| reduction.  M is fed as random numbers (no GEMM),
so any channel count an entry point accepts and maps of a few tiles are reachable, and tiles that hang over the map hold non-zero M.

Every output is a slice from the middle of a buffer pre-filled with a sentinel bit pattern: after the launch the guards are untouched
(nothing stored outside) and no sentinel is left inside (nothing skipped).

Tolerances are derived, not measured.  u = 2^-24.  A 1-D pass of wino4_bt / wino4_at is at most three roundings deep (the products by
2, 4 and 8 are exact, contraction into FMAs only removes roundings), two passes give (1 + u)^6 - 1 < 6.5 u relative to
mag = |B^T| |d| |B|; the output transforms add one rounding each for the bias and the residual: 8.5 u (|A^T| |M| |A| inv + |bias| +
|res|).  ReLU and max-pool are 1-Lipschitz.  The F(2x2) forms are shallower and take the same bars.  A pair store adds the dropped
2^-22 |V| of hi + lo and fp16's subnormal spacing (2^-25)."""
import ctypes as C

import numpy as np
import pytest

import wino_reference as wr

pytestmark = pytest.mark.gpu

U = wr.U32
IN_BAR, OUT_BAR, Z_EXTRA = 6.5, 8.5, 3.0
GUARD_BYTES = 64 * 1024                      # on either side of every output: more than a tile row of the widest map here
SENT32, SENT16 = 0x7FC5A5A5, 0x7E5A          # NaNs: a sentinel left in the output also fails every comparison
A0 = np.float32(327.68) / np.float32(8.0)    # the slot value at which scale_le_327_68 is exactly 8

IN_MAPS = [(1, 1, 1), (1, 4, 4), (2, 5, 7), (3, 9, 2), (1, 3, 61)]
OUT_MAPS = IN_MAPS + [(2, 6, 6), (1, 7, 5)]
BIG = (5, 13, 15, 160)                       # 80 tiles x 160 channels: 13 (4 per thread) or 25 (2 per thread) workgroups in grids of 16 / 32


class _Env(object):
    def __init__(self):
        import torch
        from cslam_amd import _lib
        self.torch, self._lib, self.lib, self.ck = torch, _lib, _lib.load(), _lib.check
        self.st = torch.cuda.current_stream().cuda_stream

    def dev(self, a, dtype=np.float32):
        """host array -> device tensor (None stays None); the caller holds it until the launch that reads it has been issued"""
        if a is None:
            return None
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()

    def slot(self, value):
        return self.dev(np.array([value], dtype=np.float32))


@pytest.fixture(scope="module")
def E():
    return _Env()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(x):
    return int(np.array(x, dtype=np.float32).reshape(1).view(np.uint32)[0])


def _slot_bits(t):
    return int(t.cpu().numpy().view(np.uint32)[0])


def _slot_value(t):
    return float(t.cpu().numpy()[0])


class _Guarded(object):
    """n elements of float32 / float16 in the middle of a sentinel-filled buffer."""

    def __init__(self, E, n, half=False):
        torch = E.torch
        self.np_int, self.np_float = (np.int16, np.float16) if half else (np.int32, np.float32)
        self.sent = SENT16 if half else SENT32
        self.g = GUARD_BYTES // (2 if half else 4)
        self.n = int(n)
        self.raw = torch.full((self.n + 2 * self.g,), self.sent, dtype=torch.int16 if half else torch.int32, device="cuda")
        self.ptr = C.c_void_p(self.raw.data_ptr() + GUARD_BYTES)

    def fill(self, E, a):
        """puts `a` into the slice (for the in-place forms)"""
        self.raw[self.g:self.g + self.n] = E.dev(a, self.np_float).view(self.raw.dtype).reshape(-1)

    def result(self, what):
        raw = self.raw.cpu().numpy()
        g, n = self.g, self.n
        before, body, after = raw[:g], raw[g:g + n], raw[g + n:]
        assert (before == self.sent).all(), "%s: stored %d elements before the output" % (what, int((before != self.sent).sum()))
        assert (after == self.sent).all(), "%s: stored %d elements past the output (first at +%d)" % (
            what, int((after != self.sent).sum()), int(np.argmax(after != self.sent)))
        skipped = body == self.sent
        assert not skipped.any(), "%s: %d of %d output elements never written (first at %d)" % (what, int(skipped.sum()), n, int(np.argmax(skipped)))
        return body.view(self.np_float)


def _within(got, ref, bar, what):
    """|got - ref| <= bar for every element; the message names the worst one.  Returns the largest err / bar."""
    got, ref, bar = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert got.shape == ref.shape == bar.shape, (what, got.shape, ref.shape, bar.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    bad = ~(err <= bar)                      # NaN counts as bad
    if bad.any():
        k = tuple(int(i) for i in np.unravel_index(int(np.argmax(np.where(bad, np.where(np.isnan(err), np.inf, err - bar), -np.inf))), err.shape))
        raise AssertionError("%s: %d of %d elements outside the bar; worst at %s: got %r, reference %r, error %.3e, bar %.3e" % (
            what, int(bad.sum()), bad.size, k, float(got[k]), float(ref[k]), err[k], bar[k]))
    return float((err / np.maximum(bar, 1e-300)).max())


def _binades(rng, shape):
    """normal numbers times a per-channel power of two (2^-3 .. 2^3), channels last"""
    c = shape[-1]
    return (rng.standard_normal(shape) * 2.0 ** (np.arange(c) % 7 - 3)).astype(np.float32)


def _tiles(B, H, W, tile):
    th, tw = wr.tiles_of(H, W, tile)
    return B * th * tw


def _seed(*k):
    return int(sum((i + 1) * 1009 * int(v) for i, v in enumerate(k)))


# ---------------------------------------------------------------------------------------------------- a. F(4x4) input transforms

def _check_pairs(hi, lo, V_ref, bar_v, what):
    r = _within(hi + lo, V_ref, bar_v + 2.0 ** -22 * np.abs(V_ref) + 2.0 ** -25, what + " hi + lo")
    lim = np.maximum(wr.ulp_fp16(hi) / 2, 2.0 ** -24)
    bad = ~(np.abs(lo) <= lim)
    assert not bad.any(), "%s: |lo| above half an ulp of hi at %s (hi %r, lo %r): halves swapped or lo not the remainder" % (
        what, np.argwhere(bad)[0].tolist(), float(hi[tuple(np.argwhere(bad)[0])]), float(lo[tuple(np.argwhere(bad)[0])]))
    return r


def _input_x(B, H, W, Cn, peak=None):
    rng = np.random.default_rng(_seed(B, H, W, Cn))
    x = _binades(rng, (B, H, W, Cn))
    if peak is not None:
        x = (x.astype(np.float64) * (peak / np.abs(x).max())).astype(np.float32)
    return x


def _run_input_f32(E, x):
    B, H, W, Cn = x.shape
    out = _Guarded(E, 36 * _tiles(B, H, W, 4) * Cn)
    dx = E.dev(x)
    E.ck(E.lib.cslam_wino4_input_dev(_p(dx), B, H, W, Cn, out.ptr, E.st))
    return out.result("wino4_input %s" % (x.shape,)).reshape(36, -1, Cn)


def _run_input_pairs(E, form, x, slot_value):
    """form 'h2' / 'h3' -> (hi, lo) float64 [36, T, C]; the h3 form's second hi block is compared bit for bit here"""
    B, H, W, Cn = x.shape
    T = _tiles(B, H, W, 4)
    slot, dx = E.slot(slot_value), E.dev(x)
    what = "wino4_input_%s %s slot %r" % (form, x.shape, float(slot_value))
    if form == "h2":
        out = _Guarded(E, 36 * T * 2 * Cn, half=True)
        E.ck(E.lib.cslam_wino4_input_h2_dev(_p(dx), B, H, W, Cn, _p(slot), out.ptr, E.st))
        return wr.pair_layout(out.result(what), T, Cn)
    out = _Guarded(E, 36 * T * 3 * Cn, half=True)
    E.ck(E.lib.cslam_wino4_input_h3_dev(_p(dx), B, H, W, Cn, _p(slot), out.ptr, E.st))
    hi, lo, hi2 = wr.h3_layout(out.result(what), T, Cn)
    assert np.array_equal(hi.view(np.int16), hi2.view(np.int16)), what + ": the third block is not the first bit for bit"
    return hi.astype(np.float64), lo.astype(np.float64)


def _slots_for(x):
    """(slot value, expected scale or None): exactly 327.68f / 8, the next float32 above it, a bound 1.7 x the true maximum"""
    return [(A0, 8.0), (np.nextafter(A0, np.float32(np.inf), dtype=np.float32), 4.0), (np.float32(1.7 * np.abs(x).max()), None)]


def _check_input_pairs(E, form, x):
    worst = 0.0
    for slot_value, sc_want in _slots_for(x):
        sc = wr.scale_le_327_68(slot_value)
        assert sc_want is None or sc == sc_want
        V_ref, mag = wr.input_transform(x.astype(np.float64) * sc, 4)
        assert np.abs(V_ref).max() < 32768.0
        hi, lo = _run_input_pairs(E, form, x, slot_value)
        worst = max(worst, _check_pairs(hi, lo, V_ref, IN_BAR * U * mag, "wino4_input_%s %s slot %r" % (form, x.shape, float(slot_value))))
    z = np.zeros_like(x)
    hi, lo = _run_input_pairs(E, form, z, 0.0)          # an all-zero map with slot 0: the clamped scale times zero
    assert np.isfinite(hi).all() and np.isfinite(lo).all() and not hi.any() and not lo.any()
    print("wino4_input_%s %s: largest error / bar = %.3f" % (form, x.shape, worst))


@pytest.mark.parametrize("Cn", [2, 6, 4, 12])
@pytest.mark.parametrize("B,H,W", IN_MAPS)
def test_wino4_input_equals_float64(E, B, H, W, Cn):
    """cslam_wino4_input_dev (two channels per thread) against B^T d B in float64, 6.5 u |B^T| |d| |B| per element."""
    x = _input_x(B, H, W, Cn)
    V_ref, mag = wr.input_transform(x, 4)
    r = _within(_run_input_f32(E, x), V_ref, IN_BAR * U * mag, "wino4_input %s" % (x.shape,))
    print("wino4_input %s: largest error / bar = %.3f" % (x.shape, r))


@pytest.mark.parametrize("Cn", [2, 6, 4, 12])
@pytest.mark.parametrize("B,H,W", IN_MAPS)
def test_wino4_input_h3_equals_float64(E, B, H, W, Cn):
    """cslam_wino4_input_h3_dev: C % 4 == 2 runs wino4_input_h3_kernel (two channels per thread), C % 4 == 0 the four-channel kernel.
    hi + lo against the float64 transform of sV x at three slot values around a step of the scale rule, lo the remainder of hi, the
    [36][T][hi | lo | hi] layout with both hi blocks bit-equal."""
    _check_input_pairs(E, "h3", _input_x(B, H, W, Cn, peak=20.0))


@pytest.mark.parametrize("Cn", [32, 96])
@pytest.mark.parametrize("B,H,W", IN_MAPS)
def test_wino4_input_h2_equals_float64(E, B, H, W, Cn):
    """cslam_wino4_input_h2_dev: the [36][T][C/32][hi 32 | lo 32] layout written through the lane-pair exchange, as above."""
    _check_input_pairs(E, "h2", _input_x(B, H, W, Cn, peak=20.0))


@pytest.mark.parametrize("form", ["f32", "h3", "h2"])
def test_wino4_input_over_more_than_eight_workgroups(E, form):
    """13 (25 for the two-channel kernel) workgroups in a grid rounded up to a multiple of eight: the XCD block permutation maps every
    workgroup to its own run of tiles, the surplus workgroups store nothing."""
    B, H, W, Cn = BIG
    if form == "f32":
        x = _input_x(B, H, W, Cn)
        V_ref, mag = wr.input_transform(x, 4)
        _within(_run_input_f32(E, x), V_ref, IN_BAR * U * mag, "wino4_input %s" % (x.shape,))
    else:
        _check_input_pairs(E, form, _input_x(B, H, W, Cn, peak=20.0))


# ---------------------------------------------------------------------------------------------------- b. F(4x4) output transforms

def _run_output4(E, entry, M, bias, res, B, H, W, Cn, relu, pool, amax, inv_su, amax_out, what):
    """entry 'plain' / 'scaled' / 'z' (fed the float32 rounding of the float64 column fold of M); amax / amax_out: device slots or None"""
    n_out = B * (H // 2) * (W // 2) * Cn if pool else B * H * W * Cn
    out = _Guarded(E, n_out)
    dM, db, dr = E.dev(wr.z_fold(M) if entry == "z" else M), E.dev(bias), E.dev(res)
    if entry == "plain":
        E.ck(E.lib.cslam_wino4_output_dev(_p(dM), _p(db), _p(dr), B, H, W, Cn, relu, pool, out.ptr, E.st))
    elif entry == "scaled":
        E.ck(E.lib.cslam_wino4_output_scaled_dev(_p(dM), _p(db), _p(dr), B, H, W, Cn, relu, pool, _p(amax), inv_su, _p(amax_out), out.ptr, E.st))
    else:
        assert res is None
        E.ck(E.lib.cslam_wino4_output_z_dev(_p(dM), _p(db), B, H, W, Cn, relu, pool, _p(amax), inv_su, _p(amax_out), out.ptr, E.st))
    return out.result(what).reshape((B, H // 2, W // 2, Cn) if pool else (B, H, W, Cn))


def _output_inputs(B, H, W, Cn, tile, with_res, key=0):
    """random M over all tiles (the hanging-over ones included), bias and residual across several binades; without ReLU the
    largest-magnitude output is made negative (the transform is linear: flip every input)"""
    rng = np.random.default_rng(_seed(B, H, W, Cn, tile, key))
    n = tile + 2
    M = _binades(rng, (n * n, _tiles(B, H, W, tile), Cn))
    bias = _binades(rng, (Cn,))
    res = _binades(rng, (B, H, W, Cn)) * np.float32(4.0) if with_res else None
    return M, bias, res


def _negate_if_top_is_positive(M, bias, res, B, H, W, tile, inv):
    y, _, _ = wr.output_transform(M, bias, res, B, H, W, tile, inv, False, False)
    if y.flat[np.argmax(np.abs(y))] > 0:
        return -M, (None if bias is None else -bias), (None if res is None else -res)
    return M, bias, res


def _bar_of(entry):
    return (OUT_BAR + (Z_EXTRA if entry == "z" else 0.0)) * U


@pytest.mark.parametrize("Cn", [2, 6, 32])
@pytest.mark.parametrize("B,H,W", OUT_MAPS)
@pytest.mark.parametrize("entry", ["plain", "scaled", "z"])
def test_wino4_output_equals_float64(E, entry, B, H, W, Cn):
    """A^T M A inv + bias (ReLU) (MaxPool2d) per element: bias present / NULL, ReLU on / off, pool on / off, inv_su 1 and 2^-3."""
    worst = 0.0
    amax = None if entry == "plain" else E.slot(A0)
    for inv_su in ((1.0,) if entry == "plain" else (1.0, 0.125)):
        inv = 1.0 if entry == "plain" else inv_su / wr.scale_le_327_68(A0)
        for with_bias in (True, False):
            for relu in (1, 0):
                M, bias, _ = _output_inputs(B, H, W, Cn, 4, False)
                bias = bias if with_bias else None
                if not relu:
                    M, bias, _ = _negate_if_top_is_positive(M, bias, None, B, H, W, 4, inv)
                for pool in (0, 1):
                    what = "wino4_output[%s] %s inv_su %g bias %d relu %d pool %d" % (entry, (B, H, W, Cn), inv_su, with_bias, relu, pool)
                    y_ref, mag, _ = wr.output_transform(M, bias, None, B, H, W, 4, inv, relu, pool)
                    y = _run_output4(E, entry, M, bias, None, B, H, W, Cn, relu, pool, amax, inv_su, None, what)
                    worst = max(worst, _within(y, y_ref, _bar_of(entry) * mag, what))
    print("wino4_output[%s] %s: largest error / bar = %.3f" % (entry, (B, H, W, Cn), worst))


@pytest.mark.parametrize("Cn", [2, 6, 32])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (3, 9, 2), (1, 3, 61), (1, 7, 5)])
@pytest.mark.parametrize("entry", ["plain", "scaled"])
def test_wino4_output_residual_on_ragged_maps(E, entry, B, H, W, Cn):
    """The residual (same NHWC shape as y, four times the transform's magnitude) is added to exactly the map's pixels of every tile,
    the hanging-over ones included."""
    amax = None if entry == "plain" else E.slot(A0)
    inv_su = 0.125
    inv = 1.0 if entry == "plain" else inv_su / wr.scale_le_327_68(A0)
    for relu in (1, 0):
        for with_bias in (True, False):
            M, bias, res = _output_inputs(B, H, W, Cn, 4, True, key=1)
            bias = bias if with_bias else None
            if not relu:
                M, bias, res = _negate_if_top_is_positive(M, bias, res, B, H, W, 4, inv)
            what = "wino4_output[%s] %s residual, bias %d relu %d" % (entry, (B, H, W, Cn), with_bias, relu)
            y_ref, mag, _ = wr.output_transform(M, bias, res, B, H, W, 4, inv, relu, False)
            y = _run_output4(E, entry, M, bias, res, B, H, W, Cn, relu, 0, amax, inv_su, None, what)
            _within(y, y_ref, OUT_BAR * U * mag, what)


# (3, 9, 10, 32): 27 tiles x 16 threads = 432 threads: the second workgroup's 80 idle threads pass both barriers
@pytest.mark.parametrize("B,H,W,Cn", [(2, 5, 7, 6), (1, 7, 5, 2), (2, 6, 6, 32), (3, 9, 10, 32), (1, 1, 1, 2)])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("entry", ["scaled", "scaled_no_amax", "z"])
def test_wino4_output_max_slot(E, entry, B, H, W, Cn, relu):
    """The max |y| slot of a pooled run equals the largest |y| of the kernel's own un-pooled in-map output bit for bit, lies within
    the output bar of the reference maximum, is left alone when it holds more and raised when it holds less.  'scaled_no_amax':
    d_amax NULL with d_amax_out set (no descale)."""
    kern = "z" if entry == "z" else "scaled"
    amax = None if entry == "scaled_no_amax" else E.slot(A0)
    inv_su = 0.125
    inv = 1.0 if amax is None else inv_su / wr.scale_le_327_68(A0)
    M, bias, _ = _output_inputs(B, H, W, Cn, 4, False, key=2)
    if not relu:
        M, bias, _ = _negate_if_top_is_positive(M, bias, None, B, H, W, 4, inv)
    what = "wino4_output[%s] %s relu %d slot" % (entry, (B, H, W, Cn), relu)
    y_ref, mag, ymax_ref = wr.output_transform(M, bias, None, B, H, W, 4, inv, relu, False)
    own = _run_output4(E, kern, M, bias, None, B, H, W, Cn, relu, 0, amax, inv_su, None, what)      # the kernel's own un-pooled output
    _within(own, y_ref, _bar_of(kern) * mag, what)
    own_max = np.abs(own).max()
    for pool in (1, 0):
        for preload, want in ((0.0, own_max), (np.float32(0.5) * own_max, own_max), (np.float32(2.0) * own_max, np.float32(2.0) * own_max)):
            slot = E.slot(preload)
            y = _run_output4(E, kern, M, bias, None, B, H, W, Cn, relu, pool, amax, inv_su, slot, what)
            assert _slot_bits(slot) == _bits(want), (what, pool, float(preload), _slot_value(slot), float(want))
            assert pool or np.array_equal(y.view(np.int32), own.view(np.int32)), what + ": asking for the slot changed the output"
    assert abs(float(own_max) - ymax_ref) <= _bar_of(kern) * mag.max(), (what, float(own_max), ymax_ref)


# ---------------------------------------------------------------------------------------------------- c. F(2x2)

F2_MAPS = [(1, 1, 1), (1, 2, 2), (2, 3, 5), (1, 7, 4)]


@pytest.mark.parametrize("Cn", [4, 12])
@pytest.mark.parametrize("B,H,W", F2_MAPS)
def test_wino2_input_equals_float64(E, B, H, W, Cn):
    x = _input_x(B, H, W, Cn)
    V_ref, mag = wr.input_transform(x, 2)
    out = _Guarded(E, 16 * _tiles(B, H, W, 2) * Cn)
    dx = E.dev(x)
    E.ck(E.lib.cslam_wino_input_dev(_p(dx), B, H, W, Cn, out.ptr, E.st))
    what = "wino_input %s" % (x.shape,)
    r = _within(out.result(what).reshape(16, -1, Cn), V_ref, IN_BAR * U * mag, what)
    print("%s: largest error / bar = %.3f" % (what, r))


@pytest.mark.parametrize("Cn", [4, 12])
@pytest.mark.parametrize("B,H,W", F2_MAPS)
def test_wino2_output_equals_float64(E, B, H, W, Cn):
    """cslam_wino_output_dev: bias present / NULL, ReLU on / off, then either the pool (odd sides floor) or the residual."""
    worst = 0.0
    for with_bias in (True, False):
        for relu in (1, 0):
            for pool, with_res in ((0, False), (1, False), (0, True)):
                M, bias, res = _output_inputs(B, H, W, Cn, 2, with_res)
                bias = bias if with_bias else None
                if not relu:
                    M, bias, res = _negate_if_top_is_positive(M, bias, res, B, H, W, 2, 1.0)
                what = "wino_output %s bias %d relu %d pool %d residual %d" % ((B, H, W, Cn), with_bias, relu, pool, with_res)
                y_ref, mag, _ = wr.output_transform(M, bias, res, B, H, W, 2, 1.0, relu, pool)
                out = _Guarded(E, y_ref.size)
                dM, db, dr = E.dev(M), E.dev(bias), E.dev(res)
                E.ck(E.lib.cslam_wino_output_dev(_p(dM), _p(db), _p(dr), B, H, W, Cn, relu, pool, out.ptr, E.st))
                worst = max(worst, _within(out.result(what).reshape(y_ref.shape), y_ref, OUT_BAR * U * mag, what))
    print("wino_output %s: largest error / bar = %.3f" % ((B, H, W, Cn), worst))


# ---------------------------------------------------------------------------------------------------- d. the chained transform

WL1, BMAX = 3.25, 0.5
# (B, H, W, C): one per dispatch corner -- channel group (128 / 64 / 32), threads = tile columns x group / 4, tile rows
CHAIN_SHAPES = [(2, 4, 4, 128),      # group 128,  32 threads, one tile row
                (1, 9, 10, 256),     # group 128,  96 threads, three tile rows
                (2, 16, 16, 128),    # group 128, 128 threads
                (2, 6, 20, 64),      # group 64,   80 threads, two tile rows: the first and the last step only
                (1, 8, 32, 192),     # group 64,  128 threads, three groups of a count that is no multiple of 128
                (1, 5, 33, 96),      # group 32,   72 threads
                (3, 7, 13, 32),      # group 32,   32 threads: four or fewer tile columns but C % 64 != 0
                (1, 2, 64, 32),      # group 32,  128 threads, 16 tile columns, one tile row
                (1, 1, 1, 32)]       # a single pixel


def _round_up_12_bits(v):
    m, e = np.frexp(v)
    return float(np.ldexp(np.ceil(m * 4096.0) / 4096.0, e))


def _check_chain(E, B, H, W, Cn, inv_su, with_bias):
    rng = np.random.default_rng(_seed(B, H, W, Cn, 4))
    T = _tiles(B, H, W, 4)
    M = _binades(rng, (36, T, Cn))
    bias = (np.abs(_binades(rng, (Cn,))) + np.float32(0.01)) if with_bias else None          # positive: the clip has something to clip
    inv = inv_su / wr.scale_le_327_68(A0)
    y_ref, magY, ymax_ref = wr.output_transform(M, bias, None, B, H, W, 4, inv, True, False)
    # an a-priori bound above the maximum: amax_x of 12 significant bits, so that amax_x wl1 + bmax is exact in float64 and the slot is
    # its single rounding to float32
    amax_x = _round_up_12_bits(max((1.25 * ymax_ref - BMAX) / WL1, 2.0 ** -6))
    bound_want = np.float32(np.float64(amax_x) * WL1 + BMAX)
    assert float(bound_want) >= 1.2 * ymax_ref
    sc = wr.scale_le_327_68(bound_want)
    V_ref, magV = wr.input_transform(y_ref * sc, 4)
    _, magE = wr.input_transform(magY * sc, 4)                     # |B^T| magY |B| sc: what an error of y becomes in V
    assert np.abs(V_ref).max() < 32768.0
    what = "wino4_chain %s inv_su %g bias %d" % ((B, H, W, Cn), inv_su, with_bias)
    out = _Guarded(E, 36 * T * 2 * Cn, half=True)
    vscale, ax, ay, bound = E.slot(A0), E.slot(amax_x), E.slot(0.0), E.slot(0.0)
    assert _slot_value(ax) == amax_x
    dM, db = E.dev(M), E.dev(bias)
    E.ck(E.lib.cslam_wino4_chain_h2_dev(_p(dM), _p(db), B, H, W, Cn, _p(vscale), inv_su, _p(ax),
                                        WL1, BMAX, _p(ay), _p(bound), out.ptr, E.st))
    hi, lo = wr.pair_layout(out.result(what), T, Cn)
    assert _slot_bits(bound) == _bits(bound_want), (what, _slot_value(bound), float(bound_want))
    r = _check_pairs(hi, lo, V_ref, U * (IN_BAR * magV + OUT_BAR * magE), what)
    ymax = _slot_value(ay)
    assert abs(ymax - ymax_ref) <= OUT_BAR * U * magY.max() and ymax <= float(bound_want), (what, ymax, ymax_ref, float(bound_want))
    print("%s: largest error / bar = %.3f" % (what, r))


@pytest.mark.parametrize("inv_su", [1.0, 0.125])
@pytest.mark.parametrize("B,H,W,Cn", CHAIN_SHAPES)
def test_chained_transform_equals_float64(E, B, H, W, Cn, inv_su):
    """cslam_wino4_chain_h2_dev against the reference alone: output transform + bias + ReLU, zeros outside the map's pixels although M
    and a positive bias there are not zero, then the input transform of y sc in the pair layout.  Bar per element of hi + lo:
    u (6.5 |B^T| |y sc| |B| + 8.5 |B^T| magY |B| sc) + 2^-22 |V| + 2^-25."""
    _check_chain(E, B, H, W, Cn, inv_su, True)


def test_chained_transform_without_bias(E):
    _check_chain(E, 2, 6, 20, 64, 0.125, False)


def test_chained_transform_refuses_a_map_of_65_columns(E):
    z = E.torch.zeros(64, device="cuda")
    with pytest.raises(E._lib.CslamHipError, match="wider than 64"):
        E.ck(E.lib.cslam_wino4_chain_h2_dev(_p(z), None, 1, 8, 65, 32, _p(z), 1.0, _p(z), 1.0, 0.0, _p(z), _p(z), _p(z), None))


# ---------------------------------------------------------------------------------------------------- e. bias + ReLU + pool epilogue

@pytest.mark.parametrize("relu,pool,in_place", [(0, 0, False), (1, 0, False), (0, 1, False), (1, 1, False), (0, 0, True), (1, 0, True)])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 6, 10)])
@pytest.mark.parametrize("Cn", [4, 12])
def test_bias_act_pool_is_exact(E, Cn, B, H, W, relu, pool, in_place):
    """cslam_bias_act_pool_dev is one addition and a maximum per element: bit-equal to numpy in float32, bias present and NULL.  In
    place (y = x) exists without the pool only: the pooled output is a quarter of the input."""
    rng = np.random.default_rng(_seed(B, H, W, Cn, relu, pool))
    x = _binades(rng, (B, H, W, Cn))
    for bias in (_binades(rng, (Cn,)), None):
        b = np.zeros(Cn, dtype=np.float32) if bias is None else bias
        v = x.reshape(B, H // 2, 2, W // 2, 2, Cn).max(axis=(2, 4)) if pool else x
        want = v + b
        if relu:
            want = np.maximum(want, np.float32(0.0))
        assert want.dtype == np.float32
        what = "bias_act_pool %s relu %d pool %d in place %d" % ((B, H, W, Cn), relu, pool, in_place)
        dx, db = E.dev(x), E.dev(bias)
        if in_place:
            out = _Guarded(E, x.size)
            out.fill(E, x)
            E.ck(E.lib.cslam_bias_act_pool_dev(out.ptr, _p(db), B, H, W, Cn, relu, pool, out.ptr, E.st))
        else:
            out = _Guarded(E, want.size)
            E.ck(E.lib.cslam_bias_act_pool_dev(_p(dx), _p(db), B, H, W, Cn, relu, pool, out.ptr, E.st))
        got = out.result(what).reshape(want.shape)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (what, np.argwhere(got.view(np.int32) != want.view(np.int32))[:4])


def test_bias_act_pool_refusals(E):
    buf = E.torch.zeros(2 * 3 * 4 * 4 + 16, device="cuda")
    p0 = C.c_void_p(buf.data_ptr())
    with pytest.raises(E._lib.CslamHipError, match="even H and W"):
        E.ck(E.lib.cslam_bias_act_pool_dev(p0, None, 1, 3, 4, 4, 1, 1, p0, None))
    with pytest.raises(E._lib.CslamHipError, match="even H and W"):
        E.ck(E.lib.cslam_bias_act_pool_dev(p0, None, 1, 4, 3, 4, 1, 1, p0, None))
    with pytest.raises(E._lib.CslamHipError, match="not overlap"):
        E.ck(E.lib.cslam_bias_act_pool_dev(p0, None, 2, 3, 4, 4, 1, 0, C.c_void_p(buf.data_ptr() + 64), None))
    with pytest.raises(E._lib.CslamHipError, match="not overlap"):
        E.ck(E.lib.cslam_bias_act_pool_dev(C.c_void_p(buf.data_ptr() + 64), None, 2, 3, 4, 4, 1, 0, p0, None))


# ---------------------------------------------------------------------------------------------------- f. max |x|

@pytest.mark.parametrize("n,at", [(4, 3), (4, 0), (4096 * 1024 + 4, -1), (4096 * 1024 + 4, -4), (4096 * 1024 + 4, 0), (4096 * 1024 + 4, 4096 * 1024 - 1)])
def test_absmax_equals_abs_max(E, n, at):
    """cslam_absmax_dev at the smallest size and at one vector more than the capped grid (4096 workgroups x 256 threads x 4) covers in
    one pass of its grid-stride loop: the maximum, a negative number, planted in the last vector, in the first, and at the end of the
    first pass.  The slot is non-zero before the call (the entry point zeroes it); the result is abs().max() bit for bit."""
    torch = E.torch
    g = torch.Generator(device="cuda").manual_seed(n + at % 7)
    x = torch.randn(n, generator=g, device="cuda")
    x[at] = -7.5 - x.abs().max()
    slot = E.slot(1e30)
    E.ck(E.lib.cslam_absmax_dev(_p(x), n, _p(slot), E.st))
    want = x.abs().max().cpu().numpy()
    assert float(want) == -float(x[at].item())
    assert _slot_bits(slot) == _bits(want), (_slot_value(slot), float(want))
