"""GPU tests of the convolution layer's bias and activation (np_dnn.hip: np_conv2d_forward_act, np_conv2d_backward_act;
NDArray.dnn_conv2d_forward / _backward with bias, activation and out), through the C ABI and through NDArray.

1. exact: integer operands and an integer bias (tests/dnn_act_family.py over the exact family): y for relu and none, dW, dX and db
   of the three layers (bias alone, relu alone, both) with array_equal, around every tile height, N.P around the tile width, P = 1,
   49 and 64, a strided and a dilated layer;
2. the backward rules of tanh and sigmoid on dyadic outputs k / 8 and integer gradients: dz and db with array_equal;
3. bit identities on standard-normal data, every element: the fused y against the activation of float32(y_plain + bias), relu on the
   host and tanh by NDArray.tanh on the device; no bias and no activation against np_conv2d_forward_ex; three runs; an image alone
   against the same image in a batch of 5, for y and for dz;
4. the sigmoid forward against float64 on [-30, 30], and exactly 0, 1 and NaN at -Inf, +Inf and NaN;
5. derived bounds on Gaussian data: db for any summation order, sigmoid's and tanh's dz from their three roundings;
6. the probe: (act, has_bias) of every forward, S = 1 and S > 1 of the bias gradient at the smallest extents that reach them;
7. NaN footprints: a NaN bias, a NaN in x through relu, a NaN gradient over a relu output that is zero;
8. the surface: views and pending chains, every new message, the 2- and 3-tuples, no leak, the adjoint identity as integers;
   examples/conv_classifier.py trains on the device and its loss falls."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import dnn_act_family as A
from tests import dnn_general_family as G

pytestmark = pytest.mark.gpu
U = G.U
ACTS = (None, "relu", "tanh", "sigmoid")


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


def _probe():
    """(act, has_bias, S of the last bias gradient)"""
    _l, lib = _lib()
    v = [C.c_int(-1) for _ in range(3)]
    _l.check(lib.np_debug_dnn_last_epilogue(*(C.byref(c) for c in v)))
    return tuple(c.value for c in v)


def _run(hip, call, ins, out_shapes):
    """device copies of `ins` (None stays NULL), results of `out_shapes` (None stays NULL) -> host results"""
    _l, _ = _lib()
    dev = [None if a is None else hip.DeviceArray.from_host(np.ascontiguousarray(a, np.float32)) for a in ins]
    outs = [None if s is None else hip.DeviceArray(s) for s in out_shapes]
    ptr = lambda d: None if d is None else d.ptr
    try:
        _l.check(call([ptr(d) for d in dev], [ptr(d) for d in outs]))
        return [None if d is None else d.to_host() for d in outs]
    finally:
        for d in dev + outs:
            if d is not None:
                d.free()


def _fwd(hip, x, w, b, act, g=G.Geo(), plain=False):
    """np_conv2d_forward_act (plain: np_conv2d_forward_ex) on host arrays"""
    _, lib = _lib()
    (N, Cc, H, W), (F, _c, kh, kw) = x.shape, w.shape
    ys = (N, F) + G.out_hw(H, W, kh, kw, g)
    if plain:
        return _run(hip, lambda i, o: lib.np_conv2d_forward_ex(i[0], i[1], N, Cc, H, W, F, kh, kw, *g, o[0]), [x, w], [ys])[0]
    return _run(hip, lambda i, o: lib.np_conv2d_forward_act(i[0], i[1], i[2], N, Cc, H, W, F, kh, kw, *g, A.ACT[act], o[0]), [x, w, b], [ys])[0]


def _bwd_act(hip, y, dy, act, dz=True, db=True):
    """np_conv2d_backward_act -> (dz or None, db or None)"""
    _, lib = _lib()
    N, F = dy.shape[:2]
    P = int(np.prod(dy.shape[2:]))
    return _run(hip, lambda i, o: lib.np_conv2d_backward_act(i[0], i[1], N, F, P, A.ACT[act], o[0], o[1]), [y, dy],
                [dy.shape if dz else None, (F,) if db else None])


def _grads(hip, x, w, dz, g):
    _, lib = _lib()
    (N, Cc, H, W), (F, _c, kh, kw) = x.shape, w.shape
    dims = (N, Cc, H, W, F, kh, kw) + tuple(g)
    dw = _run(hip, lambda i, o: lib.np_conv2d_backward_filter_ex(i[0], i[1], *dims, o[0]), [x, dz], [w.shape])[0]
    dx = _run(hip, lambda i, o: lib.np_conv2d_backward_data_ex(i[0], i[1], *dims, o[0]), [dz, w], [x.shape])[0]
    return dw, dx


def _kw(g):
    return {"stride": (g.sh, g.sw), "padding": (g.ph, g.pw), "dilation": (g.dh, g.dw)}


# ---- 1. exact -------------------------------------------------------------------------------------------------------------------------

def _check_exact(hip, xs, ws, g=G.Geo(), seed=0, layers=((True, None), (False, "relu"), (True, "relu")), ndarray=True):
    """every layer (has a bias, activation): y, dz, dW, dX and db through the C ABI, then through NDArray"""
    nd = _nd()
    x, w, dy, b = A.exact(np.random.default_rng(seed + 131 * xs[3] + ws[0]), xs, ws, g)
    for has_bias, act in layers:
        bias = b if has_bias else None
        y = A.forward(G.as_int(x), G.as_int(w), bias, act, g)
        dz, dW, dX, db = A.backward(x, w, y, dy, act, g)
        got = _fwd(hip, x, w, bias, act, g)
        assert got.shape == y.shape and np.array_equal(got, y), ("y", xs, ws, g, has_bias, act)
        assert _probe()[:2] == (A.ACT[act], int(has_bias))
        if act == "relu":
            assert not np.signbit(got).any()                           # -0.0 becomes +0.0
        gz, gb = _bwd_act(hip, got, dy, act, dz=act is not None)
        assert gz is None or np.array_equal(gz, dz), ("dz", xs, ws, g, act)
        assert np.array_equal(gb, db.astype(np.float32)), ("db", xs, ws, g, act)
        assert _probe()[2] == A.slices(xs[0], ws[0], y.shape[2] * y.shape[3])[0]
        gw, gx = _grads(hip, x, w, dz, g)
        assert np.array_equal(gw, dW.astype(np.float32)) and np.array_equal(gx, dX.astype(np.float32)), ("dW dX", xs, ws, g, act)
        if ndarray:
            ny = nd.dnn_conv2d_forward(_gpu(x), _gpu(w), bias=None if bias is None else _gpu(bias), activation=act, **_kw(g))
            assert ny.shape() == list(y.shape) and np.array_equal(ny.cpu().numpy(), y)
            r = nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), out=ny, activation=act, bias=True, **_kw(g))
            assert len(r) == 3 and r[2].shape() == [ws[0]]
            for a, want in zip(r, (dW, dX, db)):
                assert np.array_equal(a.cpu().numpy(), want.astype(np.float32)), (xs, ws, g, act)


@pytest.mark.parametrize("F", [1, 31, 32, 33, 64, 65, 128, 129])
def test_exact_filters_around_every_tile_height(hip, F):
    """every TM and its ragged last tile: a bias read past F would be a read past the array"""
    _check_exact(hip, (2, 3, 5, 6), (F, 3, 3, 2), ndarray=F in (33, 129))


@pytest.mark.parametrize("npix", [127, 128, 129])
def test_exact_pixels_around_the_tile_width(hip, npix):
    xs, ws = (1, 2, 3, npix + 1), (5, 2, 3, 2)                       # oh = 1, ow = npix
    assert G.out_hw(3, npix + 1, 3, 2, G.Geo()) == (1, npix)
    _check_exact(hip, xs, ws, ndarray=False)


@pytest.mark.parametrize("side", [1, 7, 8])
def test_exact_planes_of_one_pixel_odd_and_aligned(hip, side):
    """P = 1, 49 (planes that start off a 16-byte boundary), 64; N = 3 so that the walk crosses planes"""
    xs, ws = (3, 2, side + 2, side + 2), (33, 2, 3, 3)
    assert G.out_hw(xs[2], xs[3], 3, 3, G.Geo()) == (side, side)
    _check_exact(hip, xs, ws, ndarray=side == 7)


@pytest.mark.parametrize("g", [G.geo(2, 1), G.geo(1, 0, 2)])
def test_exact_a_strided_and_a_dilated_layer(hip, g):
    _check_exact(hip, (2, 3, 11, 12), (33, 3, 3, 3), g)
    _l, lib = _lib()
    form = C.c_int(-1)
    _fwd(hip, *A.exact(np.random.default_rng(0), (2, 3, 11, 12), (33, 3, 3, 3), g)[:2], None, "relu", g)
    _l.check(lib.np_debug_dnn_last_form(C.byref(form)))
    assert form.value == 1


# ---- 2. the backward rules, exactly --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 7), (2, 3, 64, 64)])             # S = 1; M = 8192: S = 2
def test_backward_rules_are_exact_on_dyadic_outputs(hip, act, shape):
    """y = k / 8, dy a small integer: every operation of the rule is exact in fp32, contracted or not, and so is every partial
    sum of db (multiples of 1 / 64 below 4, fewer than 2^16 of them)"""
    rng = np.random.default_rng(shape[0])
    k = rng.integers(-7, 8, shape) if act == "tanh" else rng.integers(1, 8, shape)
    y, dy = (k / 8.0).astype(np.float32), rng.integers(-4, 5, shape).astype(np.float32)
    dz = A.act_grad(y, dy, act)
    assert np.array_equal(dz.astype(np.float64), dy * (1 - y.astype(np.float64) ** 2) if act == "tanh" else dy * ((1 - y.astype(np.float64)) * y))
    gz, gb = _bwd_act(hip, y, dy, act)
    assert np.array_equal(gz, dz) and np.array_equal(gb.astype(np.float64), A.grad_b(dz))
    assert _probe()[2] == A.slices(shape[0], shape[1], shape[2] * shape[3])[0] == (1 if shape[2] == 7 else 2)
    only_dz = _bwd_act(hip, y, dy, act, db=False)
    assert only_dz[1] is None and _same(only_dz[0], gz)


# ---- 3. bit identities on standard-normal data -----------------------------------------------------------------------------------------

XS, WS = (2, 5, 20, 37), (33, 5, 3, 3)


@pytest.mark.parametrize("g", [G.Geo(), G.geo(2, 1)])
def test_the_fused_result_is_the_activation_of_the_plain_result_plus_the_bias(hip, g):
    nd = _nd()
    x, w, _ = G.gaussian(XS, WS, g, seed=1)
    b = np.random.default_rng(2).standard_normal(WS[0]).astype(np.float32)
    plain = _fwd(hip, x, w, None, None, g, plain=True)
    v = (plain + b[None, :, None, None]).astype(np.float32)           # one IEEE add: the same everywhere
    assert _same(_fwd(hip, x, w, b, None, g), v)
    assert _same(_fwd(hip, x, w, b, "relu", g), np.where(v <= 0, np.float32(0), v))
    assert _same(_fwd(hip, x, w, None, "relu", g), np.where(plain <= 0, np.float32(0), plain))
    assert _same(_fwd(hip, x, w, b, "tanh", g), nd.tanh(_gpu(v)).cpu().numpy())
    assert _same(_fwd(hip, x, w, None, "tanh", g), nd.tanh(_gpu(plain)).cpu().numpy())
    assert _same(_fwd(hip, x, w, None, None, g), plain) and _probe()[:2] == (0, 0)      # the plain kernels, the plain bits


def test_three_runs_are_bit_identical(hip):
    g = G.geo((2, 3), 1, (1, 2))
    x, w, dy = G.gaussian(XS, WS, g, seed=3)
    b = np.random.default_rng(4).standard_normal(WS[0]).astype(np.float32)
    for act in ACTS:
        y = _fwd(hip, x, w, b, act, g)
        first = _bwd_act(hip, y, dy, act, dz=act is not None)
        for _ in range(2):
            assert _same(_fwd(hip, x, w, b, act, g), y)
            again = _bwd_act(hip, y, dy, act, dz=act is not None)
            assert _same(again[1], first[1]) and (act is None or _same(again[0], first[0]))


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid"])
def test_an_image_gives_the_same_bits_alone_and_in_a_batch(hip, act):
    xs, ws, g = (5, 6, 17, 19), (7, 6, 3, 3), G.geo(2, 1)
    x, w, dy = G.gaussian(xs, ws, g, seed=7)
    b = np.random.default_rng(8).standard_normal(ws[0]).astype(np.float32)
    y = _fwd(hip, x, w, b, act, g)
    dz, db = _bwd_act(hip, y, dy, act)
    for n in range(5):
        assert _same(_fwd(hip, x[n:n + 1], w, b, act, g), y[n:n + 1])
        one = _bwd_act(hip, y[n:n + 1], dy[n:n + 1], act)
        assert _same(one[0], dz[n:n + 1])                              # db of a batch is NOT expected to be a sum of these


# ---- 4. the sigmoid forward ----------------------------------------------------------------------------------------------------------------

def test_sigmoid_forward_against_float64_and_at_the_special_values(hip):
    """a 1 x 1 layer with unit filters: the pre-activation is x + bias[f], one fp32 add"""
    v = np.linspace(-30, 30, 2 * 3 * 41 * 25).astype(np.float32).reshape(2, 1, 41, 75)
    w = np.ones((3, 1, 1, 1), np.float32)
    b = np.array([0.0, 0.375, -2.5], np.float32)
    pre = (v + b[None, :, None, None]).astype(np.float32)
    assert _same(_fwd(hip, v, w, b, None), pre)
    got = _fwd(hip, v, w, b, "sigmoid").astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(-pre.astype(np.float64)))
    worst = float(np.max(np.abs(got - ref) / ref))
    print("\nsigmoid forward on [-32.5, 30.4]: worst relative error against float64 %.3g (bound 1e-5)" % worst, flush=True)
    assert worst <= 1e-5
    special = _fwd(hip, v, w, np.array([-np.inf, np.inf, np.nan], np.float32), "sigmoid")
    assert np.all(special[:, 0] == 0) and not np.signbit(special[:, 0]).any() and np.all(special[:, 1] == 1) and np.isnan(special[:, 2]).all()


# ---- 5. derived bounds --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(4, 33, 14, 14), (8, 5, 56, 56)])           # M = 784: S = 1; M = 25088: S = 6
def test_gaussian_gradients_stay_inside_the_derived_bounds(hip, shape):
    rng = np.random.default_rng(shape[1])
    dy = rng.standard_normal(shape).astype(np.float32)
    pre = (2 * rng.standard_normal(shape)).astype(np.float32)
    M, lines = shape[0] * shape[2] * shape[3], []
    for act in ACTS:
        y = A.activate(pre, act)                                       # any fp32 y in the activation's range will do
        y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
        gz, gb = _bwd_act(hip, y, dy, act, dz=act is not None)
        dz = dy if act is None else gz
        if act == "relu":
            assert _same(gz, np.where(y <= 0, np.float32(0), dy))
        if act == "sigmoid":                                            # three roundings: gamma_3 |dz_ref|
            ref = dy64 * ((1 - y64) * y64)
            bound = 3 * U / (1 - 3 * U) * np.abs(ref)
        if act == "tanh":                                               # y^2 rounded, 1 - . rounded, the product rounded
            ref = dy64 * (1 - y64 * y64)
            bound = np.abs(dy64) * (U * y64 * y64 + 2 * U * np.abs(1 - y64 * y64)) * (1 + U)
        ratio_z = 0.0
        if act in ("tanh", "sigmoid"):
            err = np.abs(gz.astype(np.float64) - ref)
            ratio_z = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
            assert np.all(err <= bound), act
        z64 = dz.astype(np.float64)                                      # db sums the dz the device wrote
        ref_b, abs_b = z64.sum(axis=(0, 2, 3)), np.abs(z64).sum(axis=(0, 2, 3))
        bound_b = (M - 1) * U * abs_b / (1 - (M - 1) * U)
        err_b = np.abs(gb.astype(np.float64) - ref_b)
        lines.append("%-7s dz %.3f  db %.2e" % (act, ratio_z, float(np.max(err_b / bound_b))))
        assert np.all(err_b <= bound_b), act
    print("\n(N, F, oh, ow) = %s, M = %d, S = %d: worst |err| / bound   %s" % (shape, M, A.slices(shape[0], shape[1], shape[2] * shape[3])[0],
                                                                             "   ".join(lines)), flush=True)


# ---- 6. paths -----------------------------------------------------------------------------------------------------------------------------

def test_the_probe_reports_every_epilogue(hip):
    x, w, _, b = A.exact(np.random.default_rng(0), (2, 3, 6, 6), (4, 3, 3, 3))
    for act in ACTS:
        for bias in (None, b):
            _fwd(hip, x, w, bias, act)
            assert _probe()[:2] == (A.ACT[act], int(bias is not None))
    _fwd(hip, x, w, b, "tanh")
    _fwd(hip, x, w, None, None, plain=True)
    assert _probe()[:2] == (0, 0)


@pytest.mark.parametrize("shape,S", [((1, 3, 1, 8191), 1), ((1, 3, 1, 8192), 2), ((2, 1, 64, 64), 2), ((3, 2047, 1, 1), 1), ((5, 2, 49, 49), 2)])
def test_the_bias_gradient_with_one_slice_and_with_more(hip, shape, S):
    """the smallest extents that reach S > 1 (M = 2 kActMinSlice) and the largest that do not; integers: exact whatever the order"""
    assert A.slices(shape[0], shape[1], shape[2] * shape[3])[0] == S
    rng = np.random.default_rng(S)
    y, dy = rng.integers(-4, 5, shape).astype(np.float32), rng.integers(-4, 5, shape).astype(np.float32)
    for act in (None, "relu"):
        dz = A.act_grad(y, dy, act)
        gz, gb = _bwd_act(hip, y, dy, act, dz=act is not None)
        assert _probe()[2] == S and np.array_equal(gb, A.grad_b(dz).astype(np.float32)) and (act is None or np.array_equal(gz, dz))
    g = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    first = _bwd_act(hip, y, g, "relu")
    for _ in range(2):
        again = _bwd_act(hip, y, g, "relu")
        assert _same(again[0], first[0]) and _same(again[1], first[1])


# ---- 7. footprints -----------------------------------------------------------------------------------------------------------------------

NXS, NWS, NG = (3, 4, 13, 14), (5, 4, 3, 3), G.geo(2, 1)


def _only(got, mask, clean):
    return np.array_equal(np.isnan(got), mask) and np.array_equal(got[~mask], clean[~mask])


def test_a_nan_bias_reaches_exactly_its_filter(hip):
    x, w, _, b = A.exact(np.random.default_rng(3), NXS, NWS, NG)
    for act in (None, "relu", "tanh"):
        clean = _fwd(hip, x, w, b, act, NG)
        bad = b.copy()
        bad[3] = np.nan
        mask = np.zeros(clean.shape, bool)
        mask[:, 3] = True
        assert not np.isnan(clean).any() and _only(_fwd(hip, x, w, bad, act, NG), mask, clean)


def test_a_nan_in_x_keeps_its_footprint_through_relu(hip):
    x, w, _, b = A.exact(np.random.default_rng(3), NXS, NWS, NG)
    clean = _fwd(hip, x, w, b, "relu", NG)
    x[1, 2, 4, 5] = np.nan
    mask = np.isnan(G.forward(x, w, NG))
    assert mask.any() and not mask.all() and not mask[[0, 2]].any()
    assert _only(_fwd(hip, x, w, b, "relu", NG), mask, clean)


def test_a_nan_gradient_over_a_zero_of_relu_reaches_nothing(hip):
    nd = _nd()
    x, w, dy, b = A.exact(np.random.default_rng(3), NXS, NWS, NG)
    y = nd.dnn_conv2d_forward(_gpu(x), _gpu(w), bias=_gpu(b), activation="relu", **_kw(NG))
    yh = y.cpu().numpy()
    clean = [a.cpu().numpy() for a in nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), out=y, activation="relu", bias=True, **_kw(NG))]
    cells = np.argwhere(yh <= 0)
    assert len(cells) > 10
    for cell, value in zip(cells[::len(cells) // 3][:3], (np.nan, np.inf, -np.inf)):
        bad = dy.copy()
        bad[tuple(cell)] = value
        got = [a.cpu().numpy() for a in nd.dnn_conv2d_backward(_gpu(x), _gpu(bad), _gpu(w), out=y, activation="relu", bias=True, **_kw(NG))]
        assert all(_same(a, c) for a, c in zip(got, clean)), cell
        gz, gb = _bwd_act(hip, yh, bad, "relu")
        assert np.isfinite(gz).all() and np.isfinite(gb).all() and gz[tuple(cell)] == 0 and not np.signbit(gz[tuple(cell)])
    over = dy.copy()
    hot = tuple(np.argwhere(yh > 0)[0])
    over[hot] = np.nan                                                  # and over a positive output it does arrive: exactly filter hot[1]'s db
    gz, gb = _bwd_act(hip, yh, over, "relu")
    assert np.isnan(gz[hot]) and np.isnan(gz).sum() == 1 and np.array_equal(np.isnan(gb), np.arange(NWS[0]) == hot[1])


# ---- 8. the surface ---------------------------------------------------------------------------------------------------------------------

def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    xs, ws, g = (2, 3, 10, 12), (5, 3, 3, 2), G.geo((2, 3), 1, (2, 1))
    kw = _kw(g)
    x, w, dy = G.gaussian(xs, ws, g, seed=2)
    b = np.random.default_rng(5).standard_normal(ws[0]).astype(np.float32)
    y = _fwd(hip, x, w, b, "tanh", g)
    dz, db = _bwd_act(hip, y, dy, "tanh")
    dw, dx = _grads(hip, x, w, dz, g)
    xt = nd.transpose(_gpu(np.ascontiguousarray(x.transpose(3, 2, 1, 0))))               # a strided view: all axes reversed
    long_bias = np.full(2 * ws[0] + 1, 9.0, np.float32)
    long_bias[1:1 + ws[0]] = b
    bias_view = _gpu(long_bias).slice([1, 1 + ws[0]])                                      # a slice of a longer vector
    assert bias_view.shape() == [ws[0]]
    assert _same(nd.dnn_conv2d_forward(xt, _gpu(w), bias=bias_view, activation="tanh", **kw).cpu().numpy(), y)
    yt = nd.transpose(_gpu(np.ascontiguousarray(y.transpose(3, 2, 1, 0))))
    r = nd.dnn_conv2d_backward(xt, _gpu(dy), _gpu(w), out=yt, activation="tanh", bias=True, **kw)
    assert all(_same(a.cpu().numpy(), want) for a, want in zip(r, (dw, dx, db)))
    nd.set_lazy_binding(True)
    try:
        got = nd.dnn_conv2d_forward((_gpu(x) * 2.0) * 0.5, _gpu(w), bias=(_gpu(b) * 4.0) * 0.25, activation="tanh", **kw)     # pending chains
        assert _same(got.cpu().numpy(), y)
        r = nd.dnn_conv2d_backward(_gpu(x), (_gpu(dy) * 2.0) * 0.5, _gpu(w), out=(_gpu(y) * 2.0) * 0.5, activation="tanh", bias=True, **kw)
        assert all(_same(a.cpu().numpy(), want) for a, want in zip(r, (dw, dx, db)))
    finally:
        nd.set_lazy_binding(False)


def test_messages_returns_and_nothing_leaks(hip):
    from numpower_amd import ndarray
    from numpower_amd.ndarray import Error
    nd = _nd()
    bias_msg = "dnn_conv2d: the bias must be 1-dimensional with one element per filter (F,)"
    out_msg = "dnn_conv2d_backward: out, the forward result, must have the shape of the gradient"
    bias_device = "dnn_conv2d: the bias must be on the device of the input and the filters"
    activation = "dnn_conv2d: unknown activation: 'r' (relu), 't' (tanh), 's' (sigmoid), 'n' or 0 (none)"
    needs_out = "dnn_conv2d_backward: an activation needs out, the forward result (gradients are expressed through the output)"
    device = "dnn_conv2d: the operands must be on the same device"
    ones = lambda *s: _gpu(np.ones(s, np.float32))
    cpu = lambda *s: nd.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 8, 9), ones(4, 3, 3, 2), ones(2, 4, 4, 5)    # stride 2, padding 1
    g = {"stride": 2, "padding": 1}
    h = ndarray._load_host()

    def raw_forward():
        if not h.NDArrayDNN_Conv2D_LayerForward(x._p, w._p, None, None, None, None, b"x"):
            ndarray._raise_pending(h)

    def raw_backward():
        if not h.NDArrayDNN_Conv2D_LayerBackward(x._p, dy._p, dy._p, w._p, None, None, None, b"R", 1):
            ndarray._raise_pending(h)

    cases = ((lambda: nd.dnn_conv2d_forward(x, w, bias=ones(3), **g), bias_msg), (lambda: nd.dnn_conv2d_forward(x, w, bias=ones(4, 1), activation="relu"), bias_msg),
             (lambda: nd.dnn_conv2d_forward(x, w, bias=cpu(4), **g), bias_device), (lambda: nd.dnn_conv2d_forward(x, w, bias=cpu(4), activation="tanh"), bias_device),
             (lambda: nd.dnn_conv2d_backward(x, dy, w, out=ones(2, 4, 4, 4), activation="relu", **g), out_msg),
             (lambda: nd.dnn_conv2d_backward(x, dy, w, out=ones(2, 4, 20), activation="sigmoid", bias=True, **g), out_msg),
             (lambda: nd.dnn_conv2d_backward(x, dy, w, out=cpu(2, 4, 4, 5), activation="relu", **g), device),
             (lambda: nd.dnn_conv2d_backward(x, dy, w, activation="relu", **g), needs_out),
             (lambda: nd.dnn_conv2d_backward(x, ones(2, 4, 4, 4), w, out=ones(2, 4, 4, 4), activation="relu", bias=True, **g),
              "dnn_conv2d_backward: the gradient must have the shape of the forward result (N, F, (H + 2 ph - keh) / sh + 1, (W + 2 pw - kew) / sw + 1)"),
             (lambda: nd.dnn_conv2d_forward(x, w, bias=ones(4), stride=0), "dnn_conv2d: the stride must be at least 1 along both axes"),
             (raw_forward, activation), (raw_backward, activation))
    for call, msg in cases:
        gc.collect()
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == msg
        del e
        gc.collect()
        assert nd.live_device_allocations() == before, msg
    _l, lib = _lib()
    gc.collect()
    before, pool = nd.live_device_allocations(), lib.np_live_allocs()
    y = nd.dnn_conv2d_forward(x, w, bias=ones(4), activation="relu", **g)
    gc.collect()
    assert nd.live_device_allocations() == before + 1 and y.shape() == [2, 4, 4, 5]
    two = nd.dnn_conv2d_backward(x, dy, w, out=y, activation="relu", **g)
    three = nd.dnn_conv2d_backward(x, dy, w, out=y, activation="relu", bias=True, **g)
    plain3 = nd.dnn_conv2d_backward(x, dy, w, bias=True, **g)
    plain2 = nd.dnn_conv2d_backward(x, dy, w, **g)
    assert (len(two), len(three), len(plain3), len(plain2)) == (2, 3, 3, 2) and isinstance(three, tuple)
    assert [a.shape() for a in three] == [[4, 3, 3, 2], [2, 3, 8, 9], [4]]
    assert np.array_equal(plain3[2].cpu().numpy(), np.full(4, 40.0, np.float32))           # N.P ones per filter
    assert nd.live_device_allocations() == before + 1 + 2 + 3 + 3 + 2
    del y, two, three, plain3, plain2
    gc.collect()
    assert nd.live_device_allocations() == before and lib.np_live_allocs() == pool           # dz went back to the pool


@pytest.mark.parametrize("xs,ws,g", [((3, 4, 9, 11), (5, 4, 3, 4), G.geo(2, 1)), ((2, 3, 18, 17), (33, 3, 3, 3), G.geo((3, 2), (2, 0), (1, 2)))])
def test_the_adjoint_identity_holds_as_exact_integers_for_relu(hip, xs, ws, g):
    """sum dz . conv(x', w) == sum dX . x' for any x': dX is the adjoint of the convolution applied to the masked gradient"""
    nd = _nd()
    rng = np.random.default_rng(ws[0])
    x, w, dy, b = A.exact(rng, xs, ws, g)
    other = rng.integers(-4, 5, xs).astype(np.float32)
    y = nd.dnn_conv2d_forward(_gpu(x), _gpu(w), bias=_gpu(b), activation="relu", **_kw(g))
    dW, dX, db = (a.cpu().numpy() for a in nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w), out=y, activation="relu", bias=True, **_kw(g)))
    dz = _bwd_act(hip, y.cpu().numpy(), dy, "relu", db=False)[0]
    conv_other = nd.dnn_conv2d_forward(_gpu(other), _gpu(w), **_kw(g)).cpu().numpy()
    dot = lambda a, c: int(np.sum(G.as_int(a) * G.as_int(c)))
    assert dot(dz, conv_other) == dot(dX, other) and dot(dz, np.ones_like(dz)) == int(G.as_int(db).sum())
    assert dot(dz, nd.dnn_conv2d_forward(_gpu(x), _gpu(w), **_kw(g)).cpu().numpy()) == dot(dW, w)


def test_the_example_trains_a_two_layer_classifier_on_the_device(hip):
    """examples/conv_classifier.py: both layers forward and backward through the new keywords; the loss falls"""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("conv_classifier", Path(__file__).resolve().parent.parent / "examples" / "conv_classifier.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, Y, labels = ex.make_problem(128)
    params, losses, p = ex.train_gpu(X, Y, 25, 0.1)
    assert np.isfinite(losses).all() and losses[-1] < 0.2 * losses[0] and all(b < a for a, b in zip(losses, losses[1:]))
    assert [a.shape() for a in params] == [[8, 1, 3, 3], [8], [4, 8, 12, 12], [4]]
    assert np.mean(np.argmax(p, axis=1) == labels) > 0.9
