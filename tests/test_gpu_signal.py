"""The device 2-D correlation (np_signal.hip: np_correlate2d; NDArray.convolve2d / correlate2d).

The reference is tests/signal_family.ref2d (float64 numpy, held against SciPy by tests/test_signal_reference_cpu.py).

Exact tests.  Integer-valued operands (|a| <= 8, |b| <= 4, integer fill, taps * 32 < 2^24): every partial sum in any order
is an exact integer, so results compare with array_equal — through the C ABI, signal_bodies and NDArray.  The shapes sit
around the kernel's constants: a workgroup owns TILE_H x TILE_W = 64 x 64 outputs (4 waves x 16 rows, a lane per column),
windows up to SMALL x SMALL = 15 x 15 are staged once (path 1), larger ones run in chunks of CHUNK x CHUNK = 16 x 16 taps
(path 2).  Sizes a dense reference cannot reach use the separable family (a[r][c] = u[r] + v[c]) and its closed form.

Bound tests.  Standard-normal data: |out - ref64| <= gamma (|a| (*) |b|) elementwise, gamma = (K + 1) u / (1 - (K + 1) u),
K = bh bw, u = 2^-24: the bound of a K-term inner product in any order, with or without FMA — derived, not measured.
Each case prints its figure before it asserts."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import signal_family as F

pytestmark = pytest.mark.gpu
TILE_H, TILE_W, SMALL, CHUNK = 64, 64, 15, 16      # np_signal.hip: kTileH, kTileW, kSmallMax, kChunk
COMBOS = list(itertools.product(F.MODES, F.BOUNDARIES, (0, 1)))      # 18: mode x boundary x (correlate, convolve)


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _c2d(hip, a, b, mode, boundary="fill", fill=0.0, flip=0):
    """np_correlate2d on host arrays -> host result"""
    _l, lib = _lib()
    oh, ow = C.c_size_t(), C.c_size_t()
    _l.check(lib.np_correlate2d_shape(a.shape[0], a.shape[1], b.shape[0], b.shape[1], F.MODE_FLAG[mode], C.byref(oh), C.byref(ow)))
    assert (oh.value, ow.value) == F.out_shape(a.shape, b.shape, mode)
    da, db = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b)
    do = hip.DeviceArray((oh.value, ow.value))
    try:
        _l.check(lib.np_correlate2d(da.ptr, a.shape[0], a.shape[1], db.ptr, b.shape[0], b.shape[1], F.MODE_FLAG[mode],
                                    F.BOUNDARY_FLAG[boundary], C.c_float(fill), flip, do.ptr))
        return do.to_host()
    finally:
        for d in (da, db, do):
            d.free()


def _nd2d(a, b, mode, boundary="fill", fill=0.0, flip=0):
    nd = _nd()
    call = nd.convolve2d if flip else nd.correlate2d
    return call(_gpu(a), _gpu(b), mode, boundary, fill).cpu().numpy()


def _last_path():
    _l, lib = _lib()
    p = C.c_int(-1)
    _l.check(lib.np_debug_conv2d_last_path(C.byref(p)))
    return p.value


def _fill_for(boundary, k):
    return (5.0, -3.0)[k % 2] if boundary == "fill" else 0.0


def _check_exact(run, a, b, combos=COMBOS, tag=""):
    for k, (mode, boundary, flip) in enumerate(combos):
        try:
            want = F.ref2d(a, b, mode, boundary, _fill_for(boundary, k), flip)
        except ValueError:
            continue
        got = run(a, b, mode, boundary, _fill_for(boundary, k), flip)
        assert got.shape == want.shape, (tag, a.shape, b.shape, mode, boundary, flip)
        assert np.array_equal(got, want.astype(np.float32)), (tag, a.shape, b.shape, mode, boundary, flip)


# image, window: ragged and full tiles (63 / 64 / 65 rows and columns), windows on both sides of the path switch
# (15 | 16), ragged chunks (17 x 33), even extents, a 1 x 1 window
PAIRS = [((TILE_H + 1, TILE_W + 1), (3, 3)), ((TILE_H, TILE_W), (SMALL, SMALL)), ((TILE_H - 1, TILE_W - 1), (CHUNK, CHUNK)),
         ((2 * TILE_H + 1, 2 * TILE_W + 1), (SMALL, CHUNK)), ((40, 70), (CHUNK + 1, 2 * CHUNK + 1)), ((33, 65), (2, 4)),
         ((64, 65), (1, 1)), ((70, 40), (CHUNK, SMALL)), ((9, 130), (7, 8))]


@pytest.mark.parametrize("sa,sb", PAIRS)
def test_exact_all_18_combinations_c_abi(hip, sa, sb):
    rng = np.random.default_rng(sa[0] * 1000 + sb[1])
    a, b = F.exact(rng, sa, sb)
    _check_exact(lambda *args: _c2d(hip, *args), a, b, tag="abi")
    assert _last_path() == (1 if max(sb) <= SMALL else 2)


@pytest.mark.parametrize("sa,sb", [PAIRS[0], PAIRS[3], PAIRS[4]])
def test_exact_all_18_combinations_ndarray(hip, sa, sb):
    rng = np.random.default_rng(sa[1] * 1000 + sb[0])
    a, b = F.exact(rng, sa, sb)
    _check_exact(_nd2d, a, b, tag="NDArray")


def test_signal_bodies_gpu_operands_never_reach_the_reference_code(hip):
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "signal_bodies"
    proc = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "signal_bodies gpu: 0 calls reached the reference's own code, 0 failures" in proc.stdout


@pytest.mark.parametrize("sa,sb", [((5, 7), (5, 7)), ((5, 7), (11, 3)), ((5, 7), (3, 23)), ((5, 7), (21, 40)), ((3, 3), (40, 50)),
                                   ((1, 1), (1, 1)), ((1, 1), (9, 9)), ((2, 3), (35, 2)), ((1000, 3), (3, 3)), ((3, 40), (1000, 3))])
def test_window_equal_to_and_larger_than_the_image(hip, sa, sb):
    """wrap / symm indices several image lengths away, 'valid' with the operands swapped for both functions"""
    rng = np.random.default_rng(7 + sa[0] + sb[0])
    a, b = F.exact(rng, sa, sb)
    _check_exact(lambda *args: _c2d(hip, *args), a, b)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4097])
def test_image_widths_and_heights(hip, n):
    rng = np.random.default_rng(n)
    combos = [("same", "fill", 0), ("same", "wrap", 1), ("same", "symm", 0), ("full", "symm", 1), ("full", "fill", 0), ("valid", "fill", 1)]
    for sa in ((5, n), (n, 5), (1, n), (n, 1)):
        for sb in ((3, 3), (CHUNK, CHUNK + 1)):
            a, b = F.exact(rng, sa, sb)
            _check_exact(lambda *args: _c2d(hip, *args), a, b, combos)


def test_fill_value_through_every_layer(hip):
    nd = _nd()
    rng = np.random.default_rng(11)
    a, b = F.exact(rng, (20, 30), (5, 4))
    for fill in (7.0, -6.0, 0.0):
        want = F.ref2d(a, b, "same", "fill", fill, 1).astype(np.float32)
        assert np.array_equal(_c2d(hip, a, b, "same", "fill", fill, 1), want)
        assert np.array_equal(_nd2d(a, b, "same", "fill", fill, 1), want)
        assert np.array_equal(nd.convolve2d(_gpu(a), _gpu(b), "same", "fill", _gpu(np.full((1, 1), fill, np.float32))).cpu().numpy(), want)
        assert np.array_equal(nd.convolve2d(_gpu(a), _gpu(b), "same", "fill", nd.array(np.full((1,), fill, np.float32))).cpu().numpy(), want)
        # a one-element view as fill_value: row 1 of a 3 x 1 array (its data pointer is the view's first element), a transposed 1 x 1
        column = _gpu(np.array([[99.0], [fill], [-99.0]], np.float32))
        assert np.array_equal(nd.convolve2d(_gpu(a), _gpu(b), "same", "fill", column.slice([1, 2])).cpu().numpy(), want)
        assert np.array_equal(nd.convolve2d(_gpu(a), _gpu(b), "same", "fill", nd.transpose(_gpu(np.full((1, 1), fill, np.float32)))).cpu().numpy(), want)
    # fill_value is not looked at under the other boundaries
    assert np.array_equal(_nd2d(a, b, "full", "wrap", 9.0, 0), F.ref2d(a, b, "full", "wrap", 0.0, 0).astype(np.float32))
    assert np.array_equal(_nd2d(a, b, "full"), F.ref2d(a, b, "full").astype(np.float32))          # the default is 0


def test_valid_swaps_for_both_functions(hip):
    rng = np.random.default_rng(12)
    for sa, sb in (((3, 4), (40, 70)), ((20, 3), (20, 90)), ((4, 4), (4, 4))):
        a, b = F.exact(rng, sa, sb)
        for flip in (0, 1):
            want = F.ref2d(a, b, "valid", flip=flip).astype(np.float32)
            assert np.array_equal(_c2d(hip, a, b, "valid", flip=flip), want)
            assert np.array_equal(_nd2d(a, b, "valid", flip=flip), want)
    a, b = F.exact(rng, (3, 4), (40, 70))                                        # 'same' never swaps: shaped like a
    assert _c2d(hip, a, b, "same").shape == (3, 4)
    assert np.array_equal(_c2d(hip, a, b, "same"), F.ref2d(a, b, "same").astype(np.float32))


def _run_device(hip, da, sa, b, mode, boundary, fill, flip):
    """np_correlate2d on an image that is already on the device -> host result"""
    _l, lib = _lib()
    oh, ow = F.out_shape(sa, b.shape, mode)
    db, do = hip.DeviceArray.from_host(b), hip.DeviceArray((oh, ow))
    try:
        _l.check(lib.np_correlate2d(da.ptr, sa[0], sa[1], db.ptr, b.shape[0], b.shape[1], F.MODE_FLAG[mode], F.BOUNDARY_FLAG[boundary],
                                    C.c_float(fill), flip, do.ptr))
        return do.to_host()
    finally:
        db.free()
        do.free()


@pytest.mark.parametrize("n", [8192, 16384])
def test_large_images_by_the_separable_closed_form(hip, n):
    rng = np.random.default_rng(n)
    a, u, v = F.separable(rng, n, n)
    da = hip.DeviceArray.from_host(a)
    try:
        for sb, mode, boundary, flip in (((3, 3), "same", "wrap", 0), ((7, 7), "full", "symm", 1), ((7, 7), "valid", "fill", 0),
                                         ((3, 3), "same", "symm", 1)):
            b = rng.integers(-4, 5, size=sb).astype(np.float32)
            got = _run_device(hip, da, a.shape, b, mode, boundary, 0.0, flip)
            want = F.separable_expected(u, v, b, mode, boundary, flip)
            assert got.shape == want.shape and np.array_equal(got, want), (n, sb, mode, boundary, flip)
            del got, want
        # 'same' under 'fill' is not separable at the border: the interior by the closed form, the four border strips densely
        # (the first / last 32 output rows or columns see no more than the first / last 40 image rows or columns of a 7 x 7 window)
        b = rng.integers(-4, 5, size=(7, 7)).astype(np.float32)
        got = _run_device(hip, da, a.shape, b, "same", "fill", -2.0, 0)
        inner = F.separable_expected(u, v, b, "valid", "fill", 0)                  # output (m, n) of 'same' = 'valid' (m - 3, n - 3)
        assert np.array_equal(got[3:n - 3, 3:n - 3], inner)
        assert np.array_equal(got[:32], F.ref2d(a[:40], b, "same", "fill", -2.0, 0)[:32].astype(np.float32))
        assert np.array_equal(got[-32:], F.ref2d(a[-40:], b, "same", "fill", -2.0, 0)[-32:].astype(np.float32))
        assert np.array_equal(got[:, :32], F.ref2d(a[:, :40], b, "same", "fill", -2.0, 0)[:, :32].astype(np.float32))
        assert np.array_equal(got[:, -32:], F.ref2d(a[:, -40:], b, "same", "fill", -2.0, 0)[:, -32:].astype(np.float32))
    finally:
        da.free()


def test_a_255_x_255_window_on_2048_squared(hip):
    rng = np.random.default_rng(255)
    a, u, v = F.separable(rng, 2048, 2048)
    b = rng.integers(-4, 5, size=(255, 255)).astype(np.float32)                    # 65025 taps * 32 < 2^24
    got = _c2d(hip, a, b, "same", "wrap", 0.0, 0)
    assert _last_path() == 2
    assert np.array_equal(got, F.separable_expected(u, v, b, "same", "wrap", 0))


def test_inf_under_a_zero_tap_is_nan(hip):
    rng = np.random.default_rng(21)
    for sb in ((5, 5), (CHUNK + 3, CHUNK)):
        a, b = F.exact(rng, (70, 90), sb)
        b[1, 2] = 0.0
        b[sb[0] - 1, 0] = 0.0
        a[33, 44] = np.inf
        a[0, 0] = -np.inf
        for mode, boundary, flip in (("same", "fill", 0), ("full", "wrap", 1), ("valid", "fill", 0), ("same", "symm", 1)):
            want = F.ref2d(a, b, mode, boundary, 0.0, flip)
            got = _c2d(hip, a, b, mode, boundary, 0.0, flip)
            assert np.isnan(want).any()
            assert np.array_equal(np.isnan(got), np.isnan(want)), (sb, mode, boundary, flip)
            assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)].astype(np.float32))
    # a zero window over an infinite fill value: NaN exactly where the window leaves the image
    a, b = F.exact(rng, (20, 20), (3, 3))
    b[:] = 0.0
    got = _c2d(hip, a, b, "same", "fill", np.inf, 0)
    assert np.isnan(got[0]).all() and np.isnan(got[:, -1]).all() and (got[1:-1, 1:-1] == 0.0).all()


def test_a_nan_poisons_exactly_its_footprint_and_a_nan_fill_exactly_the_border(hip):
    rng = np.random.default_rng(22)
    for sb in ((3, 5), (CHUNK + 4, CHUNK + 1)):
        a, b = F.exact(rng, (80, 100), sb)
        b[b == 0] = 1.0
        a[40, 50] = np.nan
        for mode, flip in (("same", 0), ("full", 1), ("valid", 1), ("same", 1)):
            got = _c2d(hip, a, b, mode, "fill", 0.0, flip)
            want = F.ref2d(a, b, mode, "fill", 0.0, flip)
            assert np.isnan(want).sum() == sb[0] * sb[1]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (sb, mode, flip)
        a[40, 50] = 1.0
        got = _c2d(hip, a, b, "same", "fill", np.nan, 0)
        want = F.ref2d(a, b, "same", "fill", np.nan, 0)
        top, left = (sb[0] - 1) // 2, (sb[1] - 1) // 2
        inner = np.zeros(a.shape, bool)
        inner[top:a.shape[0] - (sb[0] - 1 - top), left:a.shape[1] - (sb[1] - 1 - left)] = True
        assert np.array_equal(np.isnan(want), ~inner)
        assert np.array_equal(np.isnan(got), ~inner)
        assert np.array_equal(got[inner], want[inner].astype(np.float32))


@pytest.mark.parametrize("sa,sb", [((257, 300), (3, 3)), ((257, 300), (SMALL, SMALL)), ((130, 200), (31, 29)), ((100, 90), (64, 64)),
                                   ((64, 64), (100, 90)), ((300, 257), (1, 40))])
def test_error_bound_on_standard_normal_data(hip, sa, sb):
    rng = np.random.default_rng(sa[0] + sb[0])
    a = rng.standard_normal(sa).astype(np.float32)
    b = rng.standard_normal(sb).astype(np.float32)
    g = F.gamma(sb[0] * sb[1])
    for mode, boundary, flip, fill in (("same", "fill", 0, 1.5), ("full", "wrap", 1, 0.0), ("valid", "fill", 0, 0.0), ("same", "symm", 1, 0.0)):
        got = _c2d(hip, a, b, mode, boundary, fill, flip).astype(np.float64)
        ref = F.ref2d(a, b, mode, boundary, fill, flip)
        scale = F.abs_ref2d(a, b, mode, boundary, fill, flip)
        ratio = np.max(np.abs(got - ref) / (g * scale))
        print("bound %s * %s %s %s flip %d: max |err| / (gamma |a|*|b|) = %.4f (gamma = %.3g)" % (sa, sb, mode, boundary, flip, ratio, g))
        assert np.all(np.abs(got - ref) <= g * scale)


def test_two_runs_are_bit_identical_and_the_inputs_are_untouched(hip):
    rng = np.random.default_rng(31)
    _l, lib = _lib()
    for sb in ((7, 7), (40, 33)):
        a = rng.standard_normal((300, 500)).astype(np.float32)
        b = rng.standard_normal(sb).astype(np.float32)
        da, db, do = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b), hip.DeviceArray((300, 500))
        outs = []
        for _ in range(2):
            _l.check(lib.np_correlate2d(da.ptr, 300, 500, db.ptr, sb[0], sb[1], 1, 4, C.c_float(0.0), 1, do.ptr))
            outs.append(do.to_host())
        assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
        assert np.array_equal(_bits(da.to_host()), _bits(a)) and np.array_equal(_bits(db.to_host()), _bits(b))
        for d in (da, db, do):
            d.free()


@pytest.mark.parametrize("sb", [(7, 7), (20, 20), (3, 40)])
def test_translation_bit_for_bit(hip, sb):
    """The same image at two offsets inside a zero field, under 'fill': the same interior, whatever tile, wave and lane an
    element falls on — the summation order does not depend on the launch geometry."""
    rng = np.random.default_rng(sb[0])
    img = rng.standard_normal((50, 70)).astype(np.float32)
    b = rng.standard_normal(sb).astype(np.float32)
    pieces = []
    for oy, ox in ((45, 41), (77, 131), (64, 64)):
        field = np.zeros((200, 300), np.float32)
        field[oy:oy + 50, ox:ox + 70] = img
        out = _c2d(hip, field, b, "same", "fill", 0.0, 0)
        pieces.append(out[oy - sb[0]:oy + 50 + sb[0], ox - sb[1]:ox + 70 + sb[1]])
    assert np.abs(pieces[0]).max() > 1.0
    assert np.array_equal(_bits(pieces[0]), _bits(pieces[1])) and np.array_equal(_bits(pieces[0]), _bits(pieces[2]))


def test_convolution_is_correlation_with_the_reversed_window_bit_for_bit(hip):
    rng = np.random.default_rng(41)
    a = rng.standard_normal((120, 150)).astype(np.float32)
    for sb, modes in (((5, 7), F.MODES), ((4, 6), ("full", "valid")), ((33, 17), F.MODES), ((16, 20), ("full", "valid"))):
        b = rng.standard_normal(sb).astype(np.float32)
        for mode in modes:                      # 'same' with an even extent centres the two differently (as in SciPy): odd only
            for boundary in F.BOUNDARIES:
                conv = _c2d(hip, a, b, mode, boundary, 0.5, 1)
                corr = _c2d(hip, a, np.ascontiguousarray(b[::-1, ::-1]), mode, boundary, 0.5, 0)
                assert np.array_equal(_bits(conv), _bits(corr)), (sb, mode, boundary)


def test_the_path_switch_and_the_two_paths_agree(hip):
    _l, lib = _lib()
    rng = np.random.default_rng(51)
    a, _ = F.exact(rng, (90, 140), (1, 1))
    for sb, path in (((SMALL, SMALL), 1), ((CHUNK, SMALL), 2), ((SMALL, CHUNK), 2), ((1, CHUNK), 2), ((CHUNK, 1), 2), ((1, 1), 1), ((3, SMALL), 1)):
        b = rng.integers(-4, 5, size=sb).astype(np.float32)
        got = _c2d(hip, a, b, "same", "symm")
        assert _last_path() == path, sb
        assert np.array_equal(got, F.ref2d(a, b, "same", "symm").astype(np.float32))
    try:
        for sb in ((SMALL, SMALL), (3, 3), (8, 2), (1, 1)):
            b = rng.integers(-4, 5, size=sb).astype(np.float32)
            for mode, boundary, flip in COMBOS:
                _l.check(lib.np_debug_conv2d_staged_path(1))
                staged = _c2d(hip, a, b, mode, boundary, 3.0, flip)
                assert _last_path() == 1
                _l.check(lib.np_debug_conv2d_staged_path(0))
                chunked = _c2d(hip, a, b, mode, boundary, 3.0, flip)
                assert _last_path() == 2
                assert np.array_equal(staged, chunked), (sb, mode, boundary, flip)
                assert np.array_equal(chunked, F.ref2d(a, b, mode, boundary, 3.0, flip).astype(np.float32))
    finally:
        _l.check(lib.np_debug_conv2d_staged_path(1))


def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    rng = np.random.default_rng(61)
    a, b = F.exact(rng, (40, 70), (6, 5))
    want = F.ref2d(a, b, "same", "symm", 0.0, 1).astype(np.float32)
    at, bt = _gpu(np.ascontiguousarray(a.T)), _gpu(np.ascontiguousarray(b.T))
    keep_a, keep_b = at.cpu().numpy().copy(), bt.cpu().numpy().copy()
    got = nd.convolve2d(nd.transpose(at), nd.transpose(bt), "same", "symm")        # strided views of both operands
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_bits(at.cpu().numpy()), _bits(keep_a)) and np.array_equal(_bits(bt.cpu().numpy()), _bits(keep_b))
    x, y = _gpu(a), _gpu(b)
    nd.set_lazy_binding(True)
    try:
        chain = (x * 2.0) * 0.5                                                     # pending until a consumer needs it
        wchain = (y + 1.0) - 1.0
        assert np.array_equal(nd.convolve2d(chain, wchain, "same", "symm").cpu().numpy(), want)
    finally:
        nd.set_lazy_binding(False)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(a)) and np.array_equal(_bits(y.cpu().numpy()), _bits(b))


def test_every_message_and_live_allocations(hip):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    nd = _nd()
    a, b = _gpu(np.ones((6, 8), np.float32)), _gpu(np.ones((3, 3), np.float32))
    wide, vec, cube = _gpu(np.ones((2, 9), np.float32)), _gpu(np.ones((4,), np.float32)), _gpu(np.ones((2, 2, 2), np.float32))
    two = _gpu(np.ones((1, 2), np.float32))
    host = nd.array(np.ones((3, 3), np.float32))
    live = nd.live_device_allocations()
    r = nd.correlate2d(a, b, "same", "fill", 2.0)
    assert nd.live_device_allocations() == live + 1
    del r
    assert nd.live_device_allocations() == live
    for call, msg in ((lambda: nd.correlate2d(a, vec, "same", "fill"), "NDArray::correlate2d inputs must be both 2-D arrays"),
                      (lambda: nd.convolve2d(cube, b, "same", "fill"), "NDArray::correlate2d inputs must be both 2-D arrays"),
                      (lambda: nd.correlate2d(a, wide, "valid", "fill"),
                       "For 'valid' mode, one input must be at least as large as the other in every dimension"),
                      (lambda: nd.convolve2d(a, b, "same", "fill", two), "fillValue must be a scalar or an array with one element."),
                      (lambda: nd.convolve2d(a, host, "same", "fill"), "correlate2d not implemented for GPU computation."),
                      (lambda: nd.convolve2d(host, b, "full", "wrap"), "correlate2d not implemented for GPU computation."),
                      (lambda: nd.convolve2d(host, host, "full", "wrap"), "only computes on the GPU"),
                      (lambda: nd.convolve2d(a, b, "", "fill"), "mode must begin with"),
                      (lambda: nd.convolve2d(a, b, "same", "x"), "boundary must begin with")):
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert msg in str(e.value), msg
        assert nd.live_device_allocations() == before, msg
    h = __import__("numpower_amd.ndarray", fromlist=["_load_host"])._load_host()
    before = nd.live_device_allocations()
    assert not h.NDArray_Correlate2D(a._p, b._p, 3, 0, None, 0)
    assert h.numpower_host_last_error() == b"invalid mode."
    h.numpower_host_clear_error()
    assert not h.NDArray_Correlate2D(a._p, b._p, 1, 5, None, 0)                    # an unknown boundary: np_correlate2d refuses
    assert b"unknown boundary 5" in h.numpower_host_last_error()
    h.numpower_host_clear_error()
    assert nd.live_device_allocations() == before == live
    # the C ABI refuses before any launch
    d = hip.DeviceArray((16,))
    launches0, launches1 = C.c_ulonglong(), C.c_ulonglong()
    _l.check(lib.np_debug_launch_count(C.byref(launches0)))
    assert lib.np_correlate2d(None, 4, 4, d.ptr, 2, 2, 1, 0, C.c_float(0), 0, d.ptr) == -1
    assert lib.np_correlate2d(d.ptr, 4, 4, d.ptr, 2, 2, 3, 0, C.c_float(0), 0, d.ptr) == -1
    assert lib.np_correlate2d(d.ptr, 4, 4, d.ptr, 2, 2, 1, 1, C.c_float(0), 0, d.ptr) == -1
    assert lib.np_correlate2d(d.ptr, 4, 1, d.ptr, 2, 2, 0, 0, C.c_float(0), 0, d.ptr) == -1 and b"'valid' mode" in lib.np_last_error()
    assert lib.np_correlate2d(d.ptr, 0, 4, d.ptr, 2, 2, 1, 0, C.c_float(0), 0, d.ptr) == -1
    assert lib.np_correlate2d(d.ptr, 2 ** 31, 1, d.ptr, 1, 1, 1, 0, C.c_float(0), 0, d.ptr) == -1
    _l.check(lib.np_debug_launch_count(C.byref(launches1)))
    assert launches1.value == launches0.value
    d.free()
