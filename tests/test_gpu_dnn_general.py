"""GPU tests of the strided / dilated convolution layer (np_dnn.hip: np_conv2d_*_ex; NDArray.dnn_conv2d_forward / _backward with
stride, padding and dilation), through the C ABI and through NDArray.

1. exact: integer operands (tests/dnn_general_family.py over tests/dnn_family.py's exact family), y, dW and dX compared with
   array_equal for every stride, dilation, padding and window below, floor remainders 0 and s - 1, oh = ow = 1 and ow = 1; then
   one constant at a time around the kernel's constants with a stride of 2;
2. bit identities on standard-normal data, every element: _ex at (1, 1, 1, 1) against the old entry points, the strided y against
   the subsample of the unit y, the dilated y against the unit y of the stuffed filter, the strided dX against the old
   backward_data on the stuffed dy, three runs, an image alone against the same image in a batch of 5;
3. the form probe: 0 for unit geometry through either entry point, 1 for a strided forward / dW, 2 for dX of a strided layer;
4. the bound |got - ref64| <= gamma(K) (|a| (*) |b|) on four Gaussian layers (derived, tests/dnn_family.gamma);
5. NaN footprints: exactly the family's for a cell that is read, nothing for a cell no window reads, dy's dX and dW footprint;
6. the surface: keyword forms, views and pending chains, every new message, no leak, the defaults bit for bit;
7. one host path: the plain call, the _ex call at (1, 1, 1, 1) and np_conv2d_forward_act with NULL / NP_ACT_NONE return the same bits
   and leave the same probes, on every tile height and with dW in two slices."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import dnn_general_family as G

pytestmark = pytest.mark.gpu
TN, TK, TMS = 128, 32, (32, 64, 128)                       # np_dnn.hip: kTN, kTK, kTMSmall / kTMMid / kTMLarge
MIN_STEPS, TARGET_GROUPS, MAX_SLICES = 8, 512, 256         # np_dnn.hip: kWgradMinSteps, kWgradTargetGroups, kWgradMaxSlices
UNIT = G.Geo()


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _tm(rows):
    return next((t for t in TMS if rows <= t), TMS[-1])


def _slices(F, K, NP):
    """np_conv2d_backward_filter's S, from the extents alone"""
    tiles = -(-F // _tm(F)) * -(-K // TN)
    steps = -(-NP // TK)
    want = max(1, min(steps // MIN_STEPS, -(-TARGET_GROUPS // tiles), MAX_SLICES))
    per = -(-steps // want)
    return -(-steps // per)


def _last():
    """(TM, S, form) of the last launch"""
    _l, lib = _lib()
    tm, s, form = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _l.check(lib.np_debug_dnn_last_path(C.byref(tm), C.byref(s)))
    _l.check(lib.np_debug_dnn_last_form(C.byref(form)))
    return tm.value, s.value, form.value


def _abi(hip, op, a, b, xs, ws, g=None):
    """op 'y': a = x, b = w; 'dx': a = dy, b = w; 'dw': a = x, b = dy.  Host arrays in, host result out.  g None: the OLD entry
    points (stride 1, dilation 1, no padding); a Geo: the _ex ones."""
    _l, lib = _lib()
    (N, Cc, H, W), (F, _, kh, kw) = xs, ws
    oh, ow = C.c_size_t(), C.c_size_t()
    if g is None:
        _l.check(lib.np_conv2d_shape(H, W, kh, kw, 0, 0, C.byref(oh), C.byref(ow)))
        calls, geometry = (lib.np_conv2d_forward, lib.np_conv2d_backward_data, lib.np_conv2d_backward_filter), (0, 0)
    else:
        _l.check(lib.np_conv2d_shape_ex(H, W, kh, kw, *g, C.byref(oh), C.byref(ow)))
        assert (oh.value, ow.value) == G.out_hw(H, W, kh, kw, g)
        calls, geometry = (lib.np_conv2d_forward_ex, lib.np_conv2d_backward_data_ex, lib.np_conv2d_backward_filter_ex), tuple(g)
    call, shape = {"y": (calls[0], (N, F, oh.value, ow.value)), "dx": (calls[1], tuple(xs)), "dw": (calls[2], tuple(ws))}[op]
    da, db, do = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b), hip.DeviceArray(shape)
    try:
        _l.check(call(da.ptr, db.ptr, N, Cc, H, W, F, kh, kw, *geometry, do.ptr))
        return do.to_host()
    finally:
        for d in (da, db, do):
            d.free()


def _all_abi(hip, x, w, dy, g):
    xs, ws = x.shape, w.shape
    return _abi(hip, "y", x, w, xs, ws, g), _abi(hip, "dw", x, dy, xs, ws, g), _abi(hip, "dx", dy, w, xs, ws, g)


def _all_ref(x, w, dy, g, blas=False):
    return G.forward(x, w, g, blas), G.grad_w(x, dy, w.shape[2], w.shape[3], g, blas), G.grad_x(dy, w, x.shape[2], x.shape[3], g, blas)


def _check_exact(hip, xs, ws, g, seed=0, only=("y", "dW", "dX")):
    x, w, dy = G.exact(np.random.default_rng(seed + 131 * xs[3] + ws[0]), xs, ws, g)
    want = dict(zip(("y", "dW", "dX"), _all_ref(G.as_int(x), G.as_int(w), G.as_int(dy), g)))
    for name, op, a, b in (("y", "y", x, w), ("dW", "dw", x, dy), ("dX", "dx", dy, w)):
        if name in only:
            got = _abi(hip, op, a, b, xs, ws, g)
            assert got.shape == want[name].shape, (name, xs, ws, g)
            assert np.array_equal(got, want[name].astype(np.float32)), (name, xs, ws, g)


# ---- 1a. exact: strides, dilations, paddings, windows, remainders ---------------------------------------------------------------

def _extent(k_eff, pad, s, rem, steps=3):
    """an input extent with (extent + 2 pad - k_eff) mod s == rem and at least `steps` + 1 outputs (more where the padding asks)"""
    steps = max(steps, -(-(2 * pad - k_eff + 2 - rem) // s))
    return k_eff - 2 * pad + s * steps + rem


@pytest.mark.parametrize("stride", [(2, 2), (2, 3), (3, 1), (4, 4)])
@pytest.mark.parametrize("pad", [0, 1, 2])                          # 0, 1, keh - 1 of the 3 x 3 window
def test_exact_strides_with_a_3x3_window(hip, stride, pad):
    for rem in ("zero", "most"):                                        # the floor's remainder: 0 and s - 1 (cells no window reads)
        r = (0, 0) if rem == "zero" else (stride[0] - 1, stride[1] - 1)
        xs = (2, 3, _extent(3, pad, stride[0], r[0]), _extent(3, pad, stride[1], r[1]))
        g = G.geo(stride, pad)
        assert G.out_hw(xs[2], xs[3], 3, 3, g) == (4, 4)
        assert ((xs[2] + 2 * pad - 3) % stride[0], (xs[3] + 2 * pad - 3) % stride[1]) == r
        _check_exact(hip, xs, (4, 3, 3, 3), g, seed=pad)
    if stride == (4, 4) and pad == 0:
        assert G.never_read(xs[2], xs[3], 3, 3, g).sum() > xs[2] + xs[3]     # gaps between the windows and the remainder


@pytest.mark.parametrize("dilation", [(2, 2), (3, 2), (1, 3)])
@pytest.mark.parametrize("window", [(1, 1), (3, 3), (2, 3), (1, 5)])
@pytest.mark.parametrize("stride", [1, 2])
def test_exact_dilations_and_windows(hip, dilation, window, stride):
    keh, kew = G.effective(*window, G.geo(1, 0, dilation))
    for ph, pw in sorted({(0, 0), (min(1, keh - 1), min(1, kew - 1)), (keh - 1, kew - 1)}):
        g = G.geo(stride, (ph, pw), dilation)
        xs = (2, 3, _extent(keh, ph, stride, stride - 1, 2), _extent(kew, pw, stride, 0, 3))
        assert ((xs[2] + 2 * ph - keh) % stride, (xs[3] + 2 * pw - kew) % stride) == (stride - 1, 0) and min(xs) >= 2
        _check_exact(hip, xs, (4, 3) + window, g, seed=ph + 3 * pw)


@pytest.mark.parametrize("xs,ws,g", [((2, 2, 3, 3), (2, 2, 3, 3), G.geo(2)), ((2, 2, 4, 4), (2, 2, 3, 3), G.geo(2)),            # oh = ow = 1
                                     ((2, 2, 5, 5), (3, 2, 3, 3), G.geo(4, 1)), ((1, 1, 1, 1), (1, 1, 1, 1), G.geo(3)),
                                     ((2, 2, 8, 3), (2, 2, 3, 3), G.geo((2, 3), (1, 0))), ((3, 2, 9, 5), (2, 2, 2, 3), G.geo((1, 4), 0, (1, 2))),   # ow = 1
                                     ((1, 3, 23, 23), (8, 3, 7, 7), G.geo(2, 3)), ((2, 2, 6, 12), (3, 2, 2, 3), G.geo((2, 3), (0, 2), (1, 3))),
                                     ((5, 3, 9, 9), (6, 3, 3, 3), G.geo((1, 2), 1))])                                             # one axis strided
def test_exact_single_outputs_and_mixed_axes(hip, xs, ws, g):
    _check_exact(hip, xs, ws, g)


# ---- 1b. exact: one constant at a time around the kernel's constants, stride 2 ------------------------------------------------

ROWS = (31, 32, 33, 64, 65, 128, 129)
S2 = G.geo(2)


@pytest.mark.parametrize("F", ROWS)
def test_exact_filters_around_every_tile_height(hip, F):
    xs, ws = (2, 3, 7, 8), (F, 3, 3, 2)                                # oh, ow = 3, 4
    _check_exact(hip, xs, ws, S2, only=("y",))
    assert _last() == (_tm(F), 0, 1)
    _check_exact(hip, xs, ws, S2, only=("dW",))
    assert _last() == (_tm(F), 1, 1)


@pytest.mark.parametrize("Cc", ROWS)
def test_exact_channels_around_every_tile_height_for_the_data_gradient(hip, Cc):
    _check_exact(hip, (1, Cc, 5, 6), (3, Cc, 3, 3), S2, only=("dX",))
    assert _last() == (_tm(Cc), 0, 2)


@pytest.mark.parametrize("npix", [TK - 1, TK, TK + 1, TN - 1, TN, TN + 1])
def test_exact_pixels_around_the_tile_width_and_the_step(hip, npix):
    """N.oh.ow = npix: a tile's columns for y (TN), a step of dW's reduction (TK)"""
    xs, ws = (1, 2, 3, 2 * (npix - 1) + 2), (5, 2, 3, 2)               # oh = 1, ow = npix
    assert G.out_hw(3, xs[3], 3, 2, S2) == (1, npix)
    _check_exact(hip, xs, ws, S2, only=("y", "dW"))


@pytest.mark.parametrize("nhw", [TN - 1, TN, TN + 1])
def test_exact_input_pixels_around_the_tile_width_for_the_data_gradient(hip, nhw):
    _check_exact(hip, (1, 2, 1, nhw), (3, 2, 1, 2), S2, only=("dX",))   # N.H.W = nhw: the columns of dX's tile
    assert _last()[2] == 2


@pytest.mark.parametrize("Cc,F", [(TK - 1, 3), (TK, 3), (TK + 1, 3), (3, TK - 1), (3, TK), (3, TK + 1)])
def test_exact_reduction_lengths_around_the_step(hip, Cc, F):
    _check_exact(hip, (2, Cc, 4, 5), (F, Cc, 1, 1), S2)                # K = C for y, F for dX


def test_exact_filter_gradient_with_one_slice_and_with_many(hip):
    for xs, ws in (((1, 3, 13, 13), (4, 3, 3, 3)), ((4, 3, 121, 121), (4, 3, 3, 3))):
        NP = xs[0] * np.prod(G.out_hw(xs[2], xs[3], 3, 3, S2))
        _check_exact(hip, xs, ws, S2, only=("dW",))
        tm, s, form = _last()
        assert (tm, s, form) == (32, _slices(4, 27, int(NP)), 1)
        assert (s == 1) == (xs[2] == 13)


# ---- 2. bit identities on standard-normal data ----------------------------------------------------------------------------------

XS, WS = (2, 5, 33, 67), (33, 5, 3, 3)


def test_unit_geometry_through_ex_equals_the_old_entry_points(hip):
    x, w, dy = G.gaussian(XS, WS, seed=1)
    old = (_abi(hip, "y", x, w, XS, WS), _abi(hip, "dw", x, dy, XS, WS), _abi(hip, "dx", dy, w, XS, WS))
    assert all(_same(a, b) for a, b in zip(old, _all_abi(hip, x, w, dy, UNIT)))
    g = G.geo(1, (2, 1))                                               # and with padding: the old calls take it in the C ABI
    _l, lib = _lib()
    x, w, dy = G.gaussian(XS, WS, g, seed=2)
    N, Cc, H, W = XS
    for op, a, b, old_call in (("y", x, w, lib.np_conv2d_forward), ("dw", x, dy, lib.np_conv2d_backward_filter), ("dx", dy, w, lib.np_conv2d_backward_data)):
        new = _abi(hip, op, a, b, XS, WS, g)
        da, db, do = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b), hip.DeviceArray(new.shape)
        try:
            _l.check(old_call(da.ptr, db.ptr, N, Cc, H, W, WS[0], 3, 3, g.ph, g.pw, do.ptr))
            assert _same(do.to_host(), new), op
        finally:
            for d in (da, db, do):
                d.free()


@pytest.mark.parametrize("stride", [(2, 2), (3, 2), (1, 4)])
def test_a_strided_forward_is_the_subsample_of_the_unit_forward(hip, stride):
    x, w, _ = G.gaussian(XS, WS, seed=3)
    for pad in (0, 1):
        unit = _abi(hip, "y", x, w, XS, WS, G.geo(1, pad))
        assert _same(_abi(hip, "y", x, w, XS, WS, G.geo(stride, pad)), unit[:, :, ::stride[0], ::stride[1]])


@pytest.mark.parametrize("dilation", [(2, 2), (3, 1), (1, 3)])
def test_a_dilated_forward_is_the_unit_forward_with_the_stuffed_filter(hip, dilation):
    x, w, _ = G.gaussian(XS, WS, seed=4)
    ws = G.stuffed(w, *dilation)
    assert _same(_abi(hip, "y", x, w, XS, WS, G.geo(1, 1, dilation)), _abi(hip, "y", x, ws, XS, ws.shape, G.geo(1, 1)))


@pytest.mark.parametrize("stride,pad", [((2, 2), 0), ((2, 2), 1), ((3, 2), (0, 1)), ((4, 4), 2)])
def test_a_strided_data_gradient_is_the_old_one_on_the_stuffed_gradient(hip, stride, pad):
    """the divisible case: the stuffed dy has the unit layer's output extents"""
    g = G.geo(stride, pad)
    xs = (2, 5, _extent(3, g.ph, g.sh, 0, 7), _extent(3, g.pw, g.sw, 0, 9))
    _, w, dy = G.gaussian(xs, WS, g, seed=5)
    big = G.stuffed(dy, g.sh, g.sw)
    assert big.shape[2:] == (xs[2] + 2 * g.ph - 2, xs[3] + 2 * g.pw - 2)
    _l, lib = _lib()
    da, db, do = hip.DeviceArray.from_host(big), hip.DeviceArray.from_host(w), hip.DeviceArray(xs)
    try:
        _l.check(lib.np_conv2d_backward_data(da.ptr, db.ptr, *xs, WS[0], 3, 3, g.ph, g.pw, do.ptr))
        assert _last()[2] == 0
        want = do.to_host()
    finally:
        for d in (da, db, do):
            d.free()
    assert _same(_abi(hip, "dx", dy, w, xs, WS, g), want)
    assert _last()[2] == 2


def test_three_runs_are_bit_identical(hip):
    g = G.geo((2, 3), 1, (1, 2))
    x, w, dy = G.gaussian(XS, WS, g, seed=6)
    first = _all_abi(hip, x, w, dy, g)
    for _ in range(2):
        assert all(_same(a, b) for a, b in zip(first, _all_abi(hip, x, w, dy, g)))


@pytest.mark.parametrize("g", [G.geo(2, 1), G.geo((3, 2), 0, (1, 2))])
def test_an_image_gives_the_same_bits_alone_and_in_a_batch(hip, g):
    xs, ws = (5, 6, 17, 19), (7, 6, 3, 3)
    x, w, dy = G.gaussian(xs, ws, g, seed=7)
    y, dx = _abi(hip, "y", x, w, xs, ws, g), _abi(hip, "dx", dy, w, xs, ws, g)
    for n in range(5):
        one = (1,) + xs[1:]
        assert _same(_abi(hip, "y", x[n:n + 1], w, one, ws, g), y[n:n + 1])
        assert _same(_abi(hip, "dx", dy[n:n + 1], w, one, ws, g), dx[n:n + 1])


# ---- 3. the form probe ------------------------------------------------------------------------------------------------------------

def test_the_form_probe(hip):
    xs, ws = (2, 3, 9, 9), (4, 3, 3, 3)
    form = lambda op, g: (_abi(hip, op, *_operands[op], xs, ws, g), _last()[2])[1]
    for g, want in ((None, (0, 0, 0)), (UNIT, (0, 0, 0)), (G.geo(1, 1), (0, 0, 0)), (G.geo(2), (1, 1, 2)), (G.geo((1, 2), 1), (1, 1, 2)),
                    (G.geo(1, 2, 2), (1, 1, 1)), (G.geo(2, 2, 2), (1, 1, 2))):
        x, w, dy = G.exact(np.random.default_rng(0), xs, ws, g or UNIT)
        _operands = {"y": (x, w), "dw": (x, dy), "dx": (dy, w)}
        assert (form("y", g), form("dw", g), form("dx", g)) == want, g


# ---- 4. the bound -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xs,ws,g", [((2, 5, 34, 67), (33, 5, 3, 3), G.geo(2, 1)), ((1, 64, 28, 28), (64, 64, 3, 3), G.geo(2, 1)),
                                     ((2, 3, 64, 64), (16, 3, 7, 7), G.geo(2, 3)), ((2, 32, 20, 20), (32, 32, 3, 3), G.geo(1, 2, 2))])
def test_gaussian_operands_stay_inside_the_bound(hip, xs, ws, g):
    x, w, dy = G.gaussian(xs, ws, g, seed=xs[2])
    ref = _all_ref(x, w, dy, g, blas=True)
    absref = _all_ref(np.abs(x), np.abs(w), np.abs(dy), g, blas=True)
    got = _all_abi(hip, x, w, dy, g)
    ratios = [G.worst_ratio(a, r, b) for a, r, b in zip(got, ref, absref)]
    Ks = G.reductions(xs, ws, g)
    print("\n%s * %s stride (%d, %d) pad (%d, %d) dilation (%d, %d): worst |err| / (u sum|a||b|)  y %.2f (K %d)  dW %.2f (K %d)  dX %.2f (K %d)"
          % (xs, ws, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw, ratios[0], Ks[0], ratios[1], Ks[1], ratios[2], Ks[2]), flush=True)
    for name, a, r, b, K in zip(("y", "dW", "dX"), got, ref, absref, Ks):
        assert np.all(np.abs(a.astype(np.float64) - r) <= G.gamma(K) * b), name


# ---- 5. footprints ----------------------------------------------------------------------------------------------------------------

NXS, NWS = (3, 4, 13, 14), (5, 4, 3, 3)


def _clean(g):
    x, w, dy = G.exact(np.random.default_rng(3), NXS, NWS, g)
    return x, w, dy, [r.astype(np.float32) for r in _all_ref(G.as_int(x), G.as_int(w), G.as_int(dy), g)]


def _only(got, mask, clean):
    """got is NaN exactly on mask and equals clean elsewhere"""
    return np.array_equal(np.isnan(got), mask) and np.array_equal(got[~mask], clean[~mask])


@pytest.mark.parametrize("g,cell", [(G.geo(2, 1), (1, 2, 4, 5)), (G.geo(2, 1), (0, 0, 0, 0)), (G.geo((2, 3), 0, (2, 1)), (2, 3, 6, 7)),
                                    (G.geo(4), (1, 1, 4, 4)), (G.geo(1, 2, 2), (2, 0, 12, 13))])
def test_one_nan_in_a_cell_that_is_read_marks_exactly_the_family_footprint(hip, g, cell):
    x, w, dy, (y0, dw0, _) = _clean(g)
    assert not G.never_read(NXS[2], NXS[3], 3, 3, g)[cell[2], cell[3]]
    x[cell] = np.nan
    mask, wmask = np.isnan(G.forward(x, w, g)), np.isnan(G.grad_w(x, dy, 3, 3, g))
    assert mask.any() and not mask.all() and not mask[:, :, :, :].all(axis=(1, 2, 3)).any() and mask.sum() % NWS[0] == 0
    assert wmask.any() and not wmask.all() and not wmask[:, [c for c in range(4) if c != cell[1]]].any()
    assert _only(_abi(hip, "y", x, w, NXS, NWS, g), mask, y0)
    assert _only(_abi(hip, "dw", x, dy, NXS, NWS, g), wmask, dw0)


@pytest.mark.parametrize("cell", [(1, 2, 3, 3), (0, 0, 12, 0), (2, 3, 7, 11), (1, 1, 11, 13)])
def test_one_nan_in_a_cell_no_window_reads_reaches_nothing(hip, cell):
    g = G.geo(4)                                                       # windows of 3 every 4: row and column 3, 7, 11 and the remainder
    x, w, dy, (y0, dw0, dx0) = _clean(g)
    assert G.never_read(NXS[2], NXS[3], 3, 3, g)[cell[2], cell[3]]
    x[cell] = np.nan
    assert np.array_equal(_abi(hip, "y", x, w, NXS, NWS, g), y0) and np.array_equal(_abi(hip, "dw", x, dy, NXS, NWS, g), dw0)
    got = _abi(hip, "dx", dy, w, NXS, NWS, g)
    assert np.array_equal(got, dx0) and got[cell] == 0 and not np.signbit(got[cell])      # the chain over stored zeros: +0


@pytest.mark.parametrize("g,cell", [(G.geo(2, 1), (1, 2, 3, 4)), (G.geo(4), (0, 0, 0, 0)), (G.geo((2, 3), 0, (2, 1)), (2, 4, 4, 3)),
                                    (G.geo(3, 2, 1), (1, 1, 4, 5))])
def test_one_nan_in_dy_marks_exactly_its_window_and_its_filter(hip, g, cell):
    x, w, dy, (_, dw0, dx0) = _clean(g)
    assert cell[2] < dy.shape[2] and cell[3] < dy.shape[3]
    dy[cell] = np.nan
    xmask, wmask = np.isnan(G.grad_x(dy, w, NXS[2], NXS[3], g)), np.isnan(G.grad_w(x, dy, 3, 3, g))
    assert xmask.any() and not xmask.all() and 1 <= xmask[cell[0], 0].sum() <= 9 and not xmask[[n for n in range(3) if n != cell[0]]].any()
    assert np.array_equal(wmask.all(axis=(1, 2, 3)), np.arange(NWS[0]) == cell[1]) and wmask.sum() == dw0[0].size
    assert _only(_abi(hip, "dx", dy, w, NXS, NWS, g), xmask, dx0)
    assert _only(_abi(hip, "dw", x, dy, NXS, NWS, g), wmask, dw0)


def test_one_nan_tap_reaches_exactly_its_filter_and_its_input_channel(hip):
    g = G.geo(2, 1)
    x, w, dy, (y0, _, dx0) = _clean(g)
    w[3, 2, 1, 2] = np.nan
    mask = np.zeros(y0.shape, bool)
    mask[:, 3] = True
    assert _only(_abi(hip, "y", x, w, NXS, NWS, g), mask, y0)
    xmask = np.zeros(dx0.shape, bool)      # dX is the forward pass over the dilated dy: every element of input channel 2 meets the
    xmask[:, 2] = True                     # NaN tap, over a gradient or over a stored zero, the cells no window reads included
    assert _only(_abi(hip, "dx", dy, w, NXS, NWS, g), xmask, dx0)


# ---- 6. the surface ---------------------------------------------------------------------------------------------------------------

def test_keyword_forms(hip):
    nd = _nd()
    xs, ws = (2, 3, 10, 12), (5, 3, 3, 3)
    for kw, g in (({"stride": 2}, G.geo(2)), ({"stride": (2, 3), "padding": 1}, G.geo((2, 3), 1)), ({"padding": "same"}, G.geo(1, 1)),
                  ({"padding": "same", "dilation": (2, 1)}, G.geo(1, (2, 1), (2, 1))), ({"stride": [3, 1], "padding": "valid", "dilation": 2}, G.geo((3, 1), 0, 2)),
                  ({"stride": 2, "padding": (2, 0), "dilation": (1, 2)}, G.geo(2, (2, 0), (1, 2)))):
        x, w, dy = G.exact(np.random.default_rng(len(kw)), xs, ws, g)
        y, dw, dx = (r.astype(np.float32) for r in _all_ref(G.as_int(x), G.as_int(w), G.as_int(dy), g))
        got = nd.dnn_conv2d_forward(_gpu(x), _gpu(w), **kw)
        assert got.shape() == list(y.shape) and np.array_equal(got.cpu().numpy(), y), kw
        if kw.get("padding") == "same":
            assert got.shape()[2:] == list(xs[2:])
        gw, gx = nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), **kw)                 # the reference's order: dW first
        assert gw.shape() == list(ws) and np.array_equal(gw.cpu().numpy(), dw), kw
        assert gx.shape() == list(xs) and np.array_equal(gx.cpu().numpy(), dx), kw


def test_the_defaults_give_todays_results_bit_for_bit(hip):
    nd = _nd()
    xs, ws = (2, 3, 10, 12), (5, 3, 3, 2)
    x, w, dy = G.gaussian(xs, ws, seed=2)
    y, dw, dx = _abi(hip, "y", x, w, xs, ws), _abi(hip, "dw", x, dy, xs, ws), _abi(hip, "dx", dy, w, xs, ws)
    for kw in ({}, {"stride": 1, "padding": 0, "dilation": 1}, {"stride": (1, 1), "padding": "valid", "dilation": (1, 1)}):
        assert _same(nd.dnn_conv2d_forward(_gpu(x), _gpu(w), **kw).cpu().numpy(), y)
        assert _last()[2] == 0
        gw, gx = nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), **kw)
        assert _same(gw.cpu().numpy(), dw) and _same(gx.cpu().numpy(), dx)


def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    xs, ws, g, kw = (2, 3, 10, 12), (5, 3, 3, 2), G.geo((2, 3), 1, (2, 1)), {"stride": (2, 3), "padding": 1, "dilation": (2, 1)}
    x, w, dy = G.gaussian(xs, ws, g, seed=2)
    y, dw, dx = _all_abi(hip, x, w, dy, g)
    xt = nd.transpose(_gpu(np.ascontiguousarray(x.transpose(3, 2, 1, 0))))               # a strided view: all axes reversed
    assert _same(nd.dnn_conv2d_forward(xt, _gpu(w), **kw).cpu().numpy(), y)
    big = np.full((2, 3, 13, 17), 9.0, np.float32)
    big[:, :, 1:11, 2:14] = x
    sliced = _gpu(big).slice([0, 2], [0, 3], [1, 11], [2, 14])                           # a strided slice
    assert _same(nd.dnn_conv2d_forward(sliced, _gpu(w), **kw).cpu().numpy(), y)
    gw, gx = nd.dnn_conv2d_backward(sliced, _gpu(dy), nd.transpose(_gpu(np.ascontiguousarray(w.transpose(3, 2, 1, 0)))), **kw)
    assert _same(gw.cpu().numpy(), dw) and _same(gx.cpu().numpy(), dx)
    nd.set_lazy_binding(True)
    try:
        assert _same(nd.dnn_conv2d_forward((_gpu(x) * 2.0) * 0.5, (_gpu(w) * 4.0) * 0.25, **kw).cpu().numpy(), y)    # pending chains
        gw, gx = nd.dnn_conv2d_backward((_gpu(x) * 2.0) * 0.5, (_gpu(dy) * 2.0) * 0.5, _gpu(w), **kw)
        assert _same(gw.cpu().numpy(), dw) and _same(gx.cpu().numpy(), dx)
    finally:
        nd.set_lazy_binding(False)


def test_messages_and_nothing_leaks(hip):
    from numpower_amd.ndarray import Error
    nd = _nd()
    stride = "dnn_conv2d: the stride must be at least 1 along both axes"
    dilation = "dnn_conv2d: the dilation must be at least 1 along both axes"
    padding = "dnn_conv2d: the padding must be at least 0 and smaller than the effective window, dilation . (k - 1) + 1"
    effective = "dnn_conv2d: the effective window, dilation . (k - 1) + 1, must not be larger than the padded input (H + 2 ph, W + 2 pw)"
    gradient = ("dnn_conv2d_backward: the gradient must have the shape of the forward result "
                "(N, F, (H + 2 ph - keh) / sh + 1, (W + 2 pw - kew) / sw + 1)")
    same = "dnn_conv2d: padding 'same' needs stride 1 and an odd effective window, dilation . (k - 1) + 1, along both axes"
    device = "dnn_conv2d: the operands must be on the same device"
    ones = lambda *s: _gpu(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 8, 9), ones(4, 3, 3, 2), ones(2, 4, 4, 5)    # stride 2, padding 1: (8 + 2 - 3) / 2 + 1, (9 + 2 - 2) / 2 + 1
    cases = (({"stride": 0}, stride), ({"stride": (2, -1)}, stride), ({"dilation": (0, 1)}, dilation), ({"stride": 2, "padding": 3}, padding),
             ({"padding": (0, 2)}, padding), ({"padding": -1}, padding), ({"dilation": (4, 1)}, effective), ({"stride": 3, "dilation": (1, 9)}, effective),
             ({"padding": "same"}, same), ({"stride": 2, "padding": "same", "dilation": (1, 2)}, same))
    for kw, msg in cases:
        for call in (lambda: nd.dnn_conv2d_forward(x, w, **kw), lambda: nd.dnn_conv2d_backward(x, dy, w, **kw)):
            before = nd.live_device_allocations()
            with pytest.raises(Error) as e:
                call()
            assert str(e.value) == msg, kw
            del e
            assert nd.live_device_allocations() == before
    for g, msg in ((ones(2, 4, 4, 4), gradient), (ones(2, 4, 6, 8), gradient), (ones(2, 3, 4, 5), gradient),
                   (nd.array(np.ones((2, 4, 4, 5), np.float32)), device)):
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            nd.dnn_conv2d_backward(x, g, w, stride=2, padding=1)
        assert str(e.value) == msg
        del e
        assert nd.live_device_allocations() == before
    before = nd.live_device_allocations()
    y = nd.dnn_conv2d_forward(x, w, stride=2, padding=1)
    assert nd.live_device_allocations() == before + 1 and y.shape() == [2, 4, 4, 5]
    r = nd.dnn_conv2d_backward(x, dy, w, stride=2, padding=1)
    assert nd.live_device_allocations() == before + 3 and r[0].shape() == [4, 3, 3, 2] and r[1].shape() == [2, 3, 8, 9]
    del y, r
    gc.collect()
    assert nd.live_device_allocations() == before


def test_c_abi_refusals_leave_the_outputs_untouched_and_nothing_leaks(hip):
    _l, lib = _lib()
    d = hip.DeviceArray.from_host(np.full(512, 5.0, np.float32))
    live = lib.np_live_allocs()
    ok = (1, 2, 9, 9, 3, 3, 3, 1, 1, 2, 2, 2, 2)                       # N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw
    for call in (lib.np_conv2d_forward_ex, lib.np_conv2d_backward_data_ex, lib.np_conv2d_backward_filter_ex):
        for ptrs in ((None, d.ptr, d.ptr), (d.ptr, None, d.ptr), (d.ptr, d.ptr, None)):
            assert call(ptrs[0], ptrs[1], *ok, ptrs[2]) == -1 and b"null pointer" in lib.np_last_error()
        for k in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12):
            bad = list(ok)
            bad[k] = 0
            assert call(d.ptr, d.ptr, *bad, d.ptr) == -1 and b"at least 1" in lib.np_last_error()
        assert call(d.ptr, d.ptr, 1, 2, 9, 9, 3, 3, 3, 5, 0, 2, 2, 2, 2, d.ptr) == -1 and b"padding" in lib.np_last_error()
        assert call(d.ptr, d.ptr, 1, 2, 4, 9, 3, 3, 3, 0, 0, 1, 1, 2, 1, d.ptr) == -1 and b"larger than the padded image" in lib.np_last_error()
        assert call(d.ptr, d.ptr, 1, 1, 9, 9, 1, 2, 2, 0, 0, 1, 1, 1 << 31, 1, d.ptr) == -1 and b"2^31" in lib.np_last_error()
    assert np.all(d.to_host() == 5.0) and lib.np_live_allocs() == live
    g = G.geo(2, 1)
    x, w, dy = G.exact(np.random.default_rng(0), (3, 4, 40, 40), (5, 4, 3, 3), g)
    _all_abi(hip, x, w, dy, g)                                         # scratch (the flipped filters, the slices) went back to the pool
    assert lib.np_live_allocs() == live
    d.free()


@pytest.mark.parametrize("xs,ws,g", [((3, 4, 9, 11), (5, 4, 3, 4), G.geo(2, 1)), ((2, 3, 18, 17), (33, 3, 3, 3), G.geo((3, 2), (2, 0), (1, 2))),
                                     ((4, 2, 30, 40), (3, 2, 5, 2), G.geo(4, (4, 0)))])
def test_adjoint_identities_hold_as_exact_integers(hip, xs, ws, g):
    """<y, dy> = <x, dX> = <w, dW>, folded in int64 on the host"""
    x, w, dy = G.exact(np.random.default_rng(ws[0]), xs, ws, g)
    y, dw, dx = _all_abi(hip, x, w, dy, g)
    dot = lambda a, b: int(np.sum(G.as_int(a) * G.as_int(b)))
    assert dot(y, dy) == dot(x, dx) == dot(w, dw)


# ---- 7. one host path: the plain, _ex and _act entry points are one call ----------------------------------------------------------

def _probes():
    """(TM, S, form) and (act, has_bias, bias_slices) of the last launch"""
    _l, lib = _lib()
    v = [C.c_int(-1) for _ in range(3)]
    _l.check(lib.np_debug_dnn_last_epilogue(*(C.byref(c) for c in v)))
    return _last() + tuple(c.value for c in v)


def _spelled(hip, fn, a, b, shape, *args):
    """fn(a, b, *args with None standing for the result) on device copies -> (host result, probes).  A strided relu layer runs
    first: it leaves TM 32, form 1 and act 1 in the probes, which no unit-geometry call without an epilogue leaves."""
    _l, lib = _lib()
    da, db, do = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b), hip.DeviceArray(shape)
    d1 = hip.DeviceArray.from_host(np.ones((1, 1, 3, 3), np.float32))
    try:
        _l.check(lib.np_conv2d_forward_act(d1.ptr, d1.ptr, None, 1, 1, 3, 3, 1, 3, 3, 0, 0, 2, 2, 1, 1, 1, do.ptr))
        assert _probes()[:5] == (32, 0, 1, 1, 0)
        _l.check(fn(da.ptr, db.ptr, *(do.ptr if v is None else v for v in args)))
        return do.to_host(), _probes()
    finally:
        for d in (da, db, do, d1):
            d.free()


# x, w, (ph, pw) -> TM of y and dW, S of dW.  The three tile heights; dW in two slices: 648 (512 without the padding) columns are
# 21 (16) steps of 32, one tile, want = min(21 // 8, 512, 256) = 2 slices of 11 (8) steps
SPELLINGS = [((2, 3, 6, 7), (32, 3, 3, 2), (1, 0), 32, 1), ((2, 3, 6, 7), (33, 3, 3, 2), (1, 0), 64, 1), ((2, 3, 6, 7), (65, 3, 3, 2), (1, 0), 128, 1),
             ((2, 2, 18, 18), (3, 2, 3, 3), (1, 1), 32, 2), ((2, 2, 18, 18), (3, 2, 3, 3), (0, 0), 32, 2)]


@pytest.mark.parametrize("xs,ws,pad,tm,slices", SPELLINGS)
def test_one_call_three_spellings(hip, xs, ws, pad, tm, slices):
    """The plain call, the _ex call at (1, 1, 1, 1) and np_conv2d_forward_act with NULL / NP_ACT_NONE: the same bits, the same
    probes, the evaluator's integers; through NDArray the defaults and the keywords written out."""
    _l, lib = _lib()
    nd = _nd()
    g = G.Geo(*pad)
    (N, Cc, H, W), (F, _, kh, kw) = xs, ws
    x, w, dy = G.exact(np.random.default_rng(F + H), xs, ws, g)
    want = dict(zip(("y", "dw", "dx"), (r.astype(np.float32) for r in _all_ref(G.as_int(x), G.as_int(w), G.as_int(dy), g))))
    ext, unit = (N, Cc, H, W, F, kh, kw) + pad, (1, 1, 1, 1)
    assert _slices(F, Cc * kh * kw, N * dy.shape[2] * dy.shape[3]) == slices          # the rule at plan_wgrad; the probe is asserted below

    oh, ow, eh, ew = (C.c_size_t() for _ in range(4))
    _l.check(lib.np_conv2d_shape(H, W, kh, kw, *pad, C.byref(oh), C.byref(ow)))
    _l.check(lib.np_conv2d_shape_ex(H, W, kh, kw, *pad, *unit, C.byref(eh), C.byref(ew)))
    assert (oh.value, ow.value) == (eh.value, ew.value) == dy.shape[2:] == G.out_hw(H, W, kh, kw, g)

    spellings = {
        "y": (x, w, dy.shape, (tm, 0, 0, 0, 0), [(lib.np_conv2d_forward, ext + (None,)), (lib.np_conv2d_forward_ex, ext + unit + (None,)),
                                           (lambda a, b, *r: lib.np_conv2d_forward_act(a, b, None, *r), ext + unit + (0, None))]),
        "dx": (dy, w, xs, (_tm(Cc), 0, 0, 0, 0), [(lib.np_conv2d_backward_data, ext + (None,)), (lib.np_conv2d_backward_data_ex, ext + unit + (None,))]),
        # dW has no epilogue and leaves those two probes as the relu layer before it set them
        "dw": (x, dy, ws, (tm, slices, 0, 1, 0), [(lib.np_conv2d_backward_filter, ext + (None,)), (lib.np_conv2d_backward_filter_ex, ext + unit + (None,))]),
    }
    for op, (a, b, shape, path, calls) in spellings.items():
        results = [_spelled(hip, fn, a, b, shape, *args) for fn, args in calls]
        for got, probes in results:
            assert _same(got, results[0][0]) and probes == results[0][1], op
            assert probes[:5] == path, (op, probes)                                    # TM, S, the unit form, the activation, the bias
        assert np.array_equal(results[0][0], want[op]), op

    kw_pad = {} if pad == (0, 0) else {"padding": pad}
    for kw_f, kw_b in ((kw_pad, kw_pad), (dict(kw_pad, bias=None, activation=None), dict(kw_pad, out=None, activation=None, bias=False))):
        assert _same(nd.dnn_conv2d_forward(_gpu(x), _gpu(w), **kw_f).cpu().numpy(), want["y"])
        assert _probes()[:5] == (tm, 0, 0, 0, 0)
        grads = nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), **kw_b)
        assert len(grads) == 2 and _same(grads[0].cpu().numpy(), want["dw"]) and _same(grads[1].cpu().numpy(), want["dx"])
