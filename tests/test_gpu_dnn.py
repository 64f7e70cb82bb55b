"""The device convolution layer (np_dnn.hip: np_conv2d_forward / _backward_data / _backward_filter; NDArray.dnn_conv2d_forward /
dnn_conv2d_backward).

The reference is tests/dnn_family (float64 / int64 numpy, held against torch on the CPU by tests/test_dnn_reference_cpu.py).

Exact tests.  Integer-valued operands (|x|, |w|, |dy| <= 4, every reduction shorter than 2^20): every partial sum in any order
is an exact integer, so results compare with array_equal — through the C ABI, dnn_bodies and NDArray.  The shapes sit around
the kernel's constants: a workgroup owns TM x TN outputs with TM one of 32 / 64 / 128 (the smallest that covers the rows) and
TN = 128, reduced in steps of TK = 32.  Rows are F for the forward pass and dW and C for dX; columns are the N.oh.ow pixels for
the forward pass and dX and the C.kh.kw taps for dW, whose reduction over the pixels is cut into S slices.

Bound tests.  Standard-normal data: |got - ref64| <= gamma (|a| (*) |b|) elementwise, gamma = (K + 1) u / (1 - (K + 1) u),
u = 2^-24, K the reduction length of the operation: the bound of a K-term inner product in any order, with or without FMA —
derived, not measured.  Each case prints its worst ratio in units of u sum |a||b| before it asserts."""
import ctypes as C
import gc
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import dnn_family as D

pytestmark = pytest.mark.gpu
TN, TK, TMS = 128, 32, (32, 64, 128)                       # np_dnn.hip: kTN, kTK, kTMSmall / kTMMid / kTMLarge
MIN_STEPS, TARGET_GROUPS, MAX_SLICES = 8, 512, 256         # np_dnn.hip: kWgradMinSteps, kWgradTargetGroups, kWgradMaxSlices


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


def _last_path():
    _l, lib = _lib()
    tm, s = C.c_int(-1), C.c_int(-1)
    _l.check(lib.np_debug_dnn_last_path(C.byref(tm), C.byref(s)))
    return tm.value, s.value


def _abi(hip, op, a, b, xs, ws, ph=0, pw=0):
    """op 'y': a = x, b = w; 'dx': a = dy, b = w; 'dw': a = x, b = dy.  Host arrays in, host result out."""
    _l, lib = _lib()
    (N, Cc, H, W), (F, _, kh, kw) = xs, ws
    oh, ow = C.c_size_t(), C.c_size_t()
    _l.check(lib.np_conv2d_shape(H, W, kh, kw, ph, pw, C.byref(oh), C.byref(ow)))
    assert (oh.value, ow.value) == D.out_hw(H, W, kh, kw, D.Geo(ph, pw))
    call, shape = {"y": (lib.np_conv2d_forward, (N, F, oh.value, ow.value)), "dx": (lib.np_conv2d_backward_data, tuple(xs)),
                   "dw": (lib.np_conv2d_backward_filter, tuple(ws))}[op]
    da, db, do = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b), hip.DeviceArray(shape)
    try:
        _l.check(call(da.ptr, db.ptr, N, Cc, H, W, F, kh, kw, ph, pw, do.ptr))
        return do.to_host()
    finally:
        for d in (da, db, do):
            d.free()


def _all_abi(hip, x, w, dy, ph=0, pw=0):
    xs, ws = x.shape, w.shape
    return (_abi(hip, "y", x, w, xs, ws, ph, pw), _abi(hip, "dw", x, dy, xs, ws, ph, pw), _abi(hip, "dx", dy, w, xs, ws, ph, pw))


def _all_ref(x, w, dy, ph=0, pw=0, blas=False):
    g = D.Geo(ph, pw)
    return (D.forward(x, w, g, blas), D.grad_w(x, dy, w.shape[2], w.shape[3], g, blas), D.grad_x(dy, w, x.shape[2], x.shape[3], g, blas))


def _check_exact(hip, xs, ws, ph=0, pw=0, seed=0):
    x, w, dy = D.exact(np.random.default_rng(seed + 131 * xs[3] + ws[0]), xs, ws, D.Geo(ph, pw))
    want = _all_ref(D.as_int(x), D.as_int(w), D.as_int(dy), ph, pw)
    for name, got, ref in zip(("y", "dW", "dX"), _all_abi(hip, x, w, dy, ph, pw), want):
        assert got.shape == ref.shape, (name, xs, ws, ph, pw)
        assert np.array_equal(got, ref.astype(np.float32)), (name, xs, ws, ph, pw)


# ---- 1. exact, around every constant --------------------------------------------------------------------------------------

ROWS = sorted({1} | {t + d for t in TMS for d in (-1, 0, 1)})                     # F (and, for dX, C) around every TM
F_CASES = [((2, 3, 6, 7), (f, 3, 3, 2)) for f in ROWS]                            # K = 18, N.P = 48
C_CASES = [((2, c, 3, 5), (4, c, 1, 1)) for c in sorted({1, TK - 1, TK, TK + 1, 3 * TK + 1, TN - 1, TN, TN + 1, 2 * TN + 3} | set(ROWS))]
#            ^ 1 x 1 taps, a plain GEMM: K = C around TK (forward) and TN (dW's columns); C = 1; C is dX's row count
NP_CASES = [((1, 2, 3, npix + 1), (5, 2, 3, 2)) for npix in (1, TN - 1, TN, TN + 1, 2 * TN + 3)]    # oh = 1, ow = N.P; N = 1
OW_CASES = [((3, 2, 9, 3), (2, 2, 2, 3)), ((3, 2, 9, 4), (2, 2, 2, 3)), ((1, 2, 4, TN), (3, 2, 2, 2)),   # ow = 1, 2, TN - 1: rows wrap in a tile
            ((5, 3, 9, 9), (6, 3, 3, 3)),                                                             # P = 49, N = 5: images straddle tiles
            ((2, 2, 6, 9), (3, 2, 1, 5)), ((2, 2, 9, 6), (3, 2, 5, 1)), ((2, 2, 6, 9), (3, 2, 2, 3)),   # kh != kw
            ((4, 3, 5, 6), (7, 3, 5, 6)), ((1, 1, 1, 1), (1, 1, 1, 1)),                               # the window as large as the image
            ((1, 1, 8, 8), (2, 1, 3, 3))]                                                             # C = 1, N = 1


@pytest.mark.parametrize("xs,ws", F_CASES + C_CASES + NP_CASES + OW_CASES)
def test_exact_c_abi(hip, xs, ws):
    _check_exact(hip, xs, ws)
    assert _last_path()[0] == _tm(xs[1])          # dX ran last: its rows are the C channels


@pytest.mark.parametrize("xs,ws", [F_CASES[3], F_CASES[-1], C_CASES[4], NP_CASES[-1], OW_CASES[3], OW_CASES[4], OW_CASES[7]])
def test_exact_ndarray(hip, xs, ws):
    nd = _nd()
    x, w, dy = D.exact(np.random.default_rng(xs[1] + ws[0]), xs, ws)
    y, dw, dx = _all_ref(D.as_int(x), D.as_int(w), D.as_int(dy))
    got = nd.dnn_conv2d_forward(_gpu(x), _gpu(w))
    assert got.shape() == list(y.shape) and np.array_equal(got.cpu().numpy(), y.astype(np.float32))
    gw, gx = nd.dnn_conv2d_backward(_gpu(x), _gpu(dy), _gpu(w))              # the reference's order: dW first
    assert gw.shape() == list(ws) and np.array_equal(gw.cpu().numpy(), dw.astype(np.float32))
    assert gx.shape() == list(xs) and np.array_equal(gx.cpu().numpy(), dx.astype(np.float32))


def test_dnn_bodies_gpu_operands_never_reach_the_reference_code(hip):
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "dnn_bodies"
    proc = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "dnn_bodies gpu: 0 calls reached the reference's own code, 0 failures" in proc.stdout


# ---- 2. padding ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xs,ws", [((2, 3, 7, 9), (4, 3, 3, 3)), ((3, 2, 5, 6), (33, 2, 2, 5)), ((1, 4, 6, 5), (2, 4, 4, 1)),
                                   ((2, 2, 3, 3), (3, 2, 5, 5))])
def test_padding_exact_c_abi(hip, xs, ws):
    kh, kw = ws[2:]
    for ph, pw in sorted({(0, 0), (kh - 1, kw - 1), ((kh - 1) // 2, (kw - 1) // 2), (kh - 1, 0)}):
        if kh > xs[2] + 2 * ph or kw > xs[3] + 2 * pw:
            continue                              # the 5 x 5 window on 3 x 3 needs its padding
        _check_exact(hip, xs, ws, ph, pw, seed=ph * 7 + pw)


def test_padding_as_large_as_the_window_is_refused(hip):
    _l, lib = _lib()
    d = hip.DeviceArray.from_host(np.full(512, 5.0, np.float32))
    live = lib.np_live_allocs()
    oh, ow = C.c_size_t(77), C.c_size_t(77)
    for ph, pw in ((3, 0), (0, 3), (3, 3), (4, 1)):
        assert lib.np_conv2d_shape(6, 6, 3, 3, ph, pw, C.byref(oh), C.byref(ow)) == -1 and (oh.value, ow.value) == (77, 77)
        for call in (lib.np_conv2d_forward, lib.np_conv2d_backward_data, lib.np_conv2d_backward_filter):
            assert call(d.ptr, d.ptr, 1, 1, 6, 6, 1, 3, 3, ph, pw, d.ptr) == -1 and b"padding" in lib.np_last_error()
    assert np.all(d.to_host() == 5.0) and lib.np_live_allocs() == live
    d.free()


# ---- 3. footprints -------------------------------------------------------------------------------------------------------------

XS, WS = (3, 4, 9, 11), (5, 4, 3, 4)       # oh, ow = 7, 8


def _clean():
    x, w, dy = D.exact(np.random.default_rng(3), XS, WS)
    return x, w, dy, [r.astype(np.float32) for r in _all_ref(D.as_int(x), D.as_int(w), D.as_int(dy))]


def _only(got, mask, clean):
    """got is NaN exactly on mask and equals clean elsewhere"""
    return np.array_equal(np.isnan(got), mask) and np.array_equal(got[~mask], clean[~mask])


@pytest.mark.parametrize("n,c,u,v", [(1, 2, 4, 5), (0, 0, 0, 0), (2, 3, 8, 10), (1, 1, 0, 10), (2, 0, 8, 3)])
def test_one_nan_in_x_reaches_exactly_its_receptive_footprint(hip, n, c, u, v):
    x, w, dy, (y0, dw0, _) = _clean()
    x[n, c, u, v] = np.nan
    (kh, kw), (oh, ow) = WS[2:], y0.shape[2:]
    mask = np.zeros(y0.shape, bool)
    mask[n, :, max(0, u - kh + 1):min(oh, u + 1), max(0, v - kw + 1):min(ow, v + 1)] = True
    assert _only(_abi(hip, "y", x, w, XS, WS), mask, y0)
    assert np.array_equal(mask, np.isnan(D.forward(x, w)))                   # and that is the evaluator's mask
    wmask = np.zeros(dw0.shape, bool)                                        # dW: the taps (p, q) under which (u, v) is read
    for p in range(kh):
        for q in range(kw):
            wmask[:, c, p, q] = 0 <= u - p < oh and 0 <= v - q < ow
    assert _only(_abi(hip, "dw", x, dy, XS, WS), wmask, dw0)


def test_one_nan_in_w_reaches_exactly_its_channel(hip):
    x, w, dy, (y0, _, dx0) = _clean()
    w[3, 2, 1, 2] = np.nan
    mask = np.zeros(y0.shape, bool)
    mask[:, 3] = True
    assert _only(_abi(hip, "y", x, w, XS, WS), mask, y0)
    xmask = np.zeros(dx0.shape, bool)      # dX is the forward pass over dy with STORED zeros around it: every element of input channel 2
    xmask[:, 2] = True                     # meets the NaN tap, over the gradient or over a stored zero
    assert _only(_abi(hip, "dx", dy, w, XS, WS), xmask, dx0)


@pytest.mark.parametrize("n,f,i,j", [(1, 2, 3, 4), (0, 0, 0, 0), (2, 4, 6, 7)])
def test_one_nan_in_dy_reaches_exactly_its_window_and_its_filter(hip, n, f, i, j):
    x, w, dy, (_, dw0, dx0) = _clean()
    dy[n, f, i, j] = np.nan
    xmask = np.zeros(dx0.shape, bool)
    xmask[n, :, i:i + WS[2], j:j + WS[3]] = True
    assert _only(_abi(hip, "dx", dy, w, XS, WS), xmask, dx0)
    wmask = np.zeros(dw0.shape, bool)
    wmask[f] = True
    assert _only(_abi(hip, "dw", x, dy, XS, WS), wmask, dw0)


def test_an_inf_tap_over_the_padding_gives_nan(hip):
    x, w, dy, _ = _clean()
    x[x == 0] = 1.0                                # inside the image the Inf tap meets no zero: NaN comes from the padding alone
    w[1, 2, 0, 0] = np.inf
    for ph, pw in ((1, 1), (2, 3), (0, 2)):
        want = D.forward(x, w, D.Geo(ph, pw))
        got = _abi(hip, "y", x, w, XS, WS, ph, pw)
        nan = np.isnan(want)
        assert nan[:, 1].any() and not nan[:, [0, 2, 3, 4]].any()
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan], want[~nan].astype(np.float32))


# ---- 4. the bound ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xs,ws", [((2, 5, 34, 67), (33, 5, 3, 3)), ((1, 64, 14, 14), (64, 64, 3, 3)), ((2, 128, 20, 20), (32, 128, 5, 5)),
                                   ((4, 64, 56, 56), (64, 64, 3, 3))])
def test_gaussian_operands_stay_inside_the_bound(hip, xs, ws):
    x, w, dy = D.gaussian(xs, ws, seed=xs[2])
    ref = _all_ref(x, w, dy, blas=True)
    absref = _all_ref(np.abs(x), np.abs(w), np.abs(dy), blas=True)
    got = _all_abi(hip, x, w, dy)
    ratios = [D.worst_ratio(g, r, a) for g, r, a in zip(got, ref, absref)]
    Ks = D.reductions(xs, ws)
    print("\n%s * %s: worst |err| / (u sum|a||b|)  y %.2f (K %d)  dW %.2f (K %d)  dX %.2f (K %d)"
          % (xs, ws, ratios[0], Ks[0], ratios[1], Ks[1], ratios[2], Ks[2]), flush=True)
    for name, g, r, a, K in zip(("y", "dW", "dX"), got, ref, absref, Ks):
        assert np.all(np.abs(g.astype(np.float64) - r) <= D.gamma(K) * a), name


# ---- 5. determinism and batch independence ------------------------------------------------------------------------------------------

def test_three_runs_are_bit_identical(hip):
    xs, ws = (2, 5, 34, 67), (33, 5, 3, 3)
    x, w, dy = D.gaussian(xs, ws, seed=5)
    first = _all_abi(hip, x, w, dy)
    assert _last_path()[0] == 32 and _slices(ws[0], 45, 2 * 32 * 65) > 1     # dW went through the fold
    for _ in range(2):
        assert all(_same(a, b) for a, b in zip(first, _all_abi(hip, x, w, dy)))


@pytest.mark.parametrize("hw,k", [((9, 9), (3, 3)), ((5, 45), (3, 3))])        # P = 49; P = 3 x 43 = TN + 1
def test_an_image_gives_the_same_bits_alone_and_in_a_batch(hip, hw, k):
    xs, ws = (5, 6, *hw), (7, 6, *k)
    x, w, dy = D.gaussian(xs, ws, seed=hw[1])
    y = _abi(hip, "y", x, w, xs, ws)
    dx = _abi(hip, "dx", dy, w, xs, ws)
    assert y.shape[2] * y.shape[3] in (49, TN + 1)
    for n in range(5):
        one = (1,) + xs[1:]
        assert _same(_abi(hip, "y", x[n:n + 1], w, one, ws), y[n:n + 1])
        assert _same(_abi(hip, "dx", dy[n:n + 1], w, one, ws), dx[n:n + 1])


def test_every_tile_and_both_slice_counts_are_taken(hip):
    seen = set()
    for f in (4, 40, 130):                         # TM 32, 64, 128 on a short reduction: S = 1
        xs, ws = (1, 3, 6, 6), (f, 3, 3, 3)
        x, w, dy = D.exact(np.random.default_rng(f), xs, ws)
        got = _abi(hip, "dw", x, dy, xs, ws)
        seen.add(_last_path())
        assert _last_path() == (_tm(f), 1) and _slices(f, 27, 16) == 1
        assert np.array_equal(got, D.grad_w(D.as_int(x), D.as_int(dy), 3, 3).astype(np.float32))
        _abi(hip, "y", x, w, xs, ws)
        assert _last_path() == (_tm(f), 0)
    xs, ws = (4, 3, 122, 122), (4, 3, 3, 3)        # N.P = 57 600 against 3 x 3 x 3 -> 4 filters
    x, w, dy = D.exact(np.random.default_rng(1), xs, ws)
    got = _abi(hip, "dw", x, dy, xs, ws)
    tm, s = _last_path()
    assert (tm, s) == (32, _slices(4, 27, 57600)) and s > 1
    assert np.array_equal(got, D.grad_w(D.as_int(x), D.as_int(dy), 3, 3).astype(np.float32))
    assert {t for t, _ in seen} == set(TMS)


# ---- 6. the surface --------------------------------------------------------------------------------------------------------------

def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    xs, ws = (2, 3, 10, 12), (5, 3, 3, 2)
    x, w, dy = D.gaussian(xs, ws, seed=2)
    y, dw, dx = _all_abi(hip, x, w, dy)
    xt = nd.transpose(_gpu(np.ascontiguousarray(x.transpose(3, 2, 1, 0))))               # a strided view: all axes reversed
    assert _same(nd.dnn_conv2d_forward(xt, _gpu(w)).cpu().numpy(), y)
    big = np.full((2, 3, 13, 17), 9.0, np.float32)
    big[:, :, 1:11, 2:14] = x
    sliced = _gpu(big).slice([0, 2], [0, 3], [1, 11], [2, 14])                           # a strided slice
    assert _same(nd.dnn_conv2d_forward(sliced, _gpu(w)).cpu().numpy(), y)
    gw, gx = nd.dnn_conv2d_backward(sliced, _gpu(dy), nd.transpose(_gpu(np.ascontiguousarray(w.transpose(3, 2, 1, 0)))))
    assert _same(gw.cpu().numpy(), dw) and _same(gx.cpu().numpy(), dx)
    nd.set_lazy_binding(True)
    try:
        assert _same(nd.dnn_conv2d_forward((_gpu(x) * 2.0) * 0.5, (_gpu(w) * 4.0) * 0.25).cpu().numpy(), y)    # pending chains
        gw, gx = nd.dnn_conv2d_backward((_gpu(x) * 2.0) * 0.5, (_gpu(dy) * 2.0) * 0.5, _gpu(w))
        assert _same(gw.cpu().numpy(), dw) and _same(gx.cpu().numpy(), dx)
    finally:
        nd.set_lazy_binding(False)


def test_messages_and_nothing_leaks(hip):
    from numpower_amd.ndarray import Error
    nd = _nd()
    ndim = "dnn_conv2d: the operands must be 4-dimensional: the input (N, C, H, W), the filters (F, C, kh, kw)"
    channels = "dnn_conv2d: the filters' second extent must equal the input's number of channels"
    window = "dnn_conv2d: the filter window must not be larger than the input (kh <= H and kw <= W)"
    gradient = "dnn_conv2d_backward: the gradient must have the shape of the forward result (N, F, H - kh + 1, W - kw + 1)"
    device = "dnn_conv2d: the operands must be on the same device"
    cpu = ("dnn_conv2d: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first, the CPU path is the "
           "reference's own)")
    ones = lambda *s: _gpu(np.ones(s, np.float32))
    host = lambda *s: nd.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 6, 7), ones(4, 3, 3, 2), ones(2, 4, 4, 6)
    forward = ((ones(3, 6, 7), w, ndim), (x, ones(3, 3, 2), ndim), (x, ones(4, 2, 3, 2), channels), (x, ones(4, 3, 7, 2), window),
               (x, ones(4, 3, 3, 8), window), (x, host(4, 3, 3, 2), device), (host(2, 3, 6, 7), w, device),
               (host(2, 3, 6, 7), host(4, 3, 3, 2), cpu))
    for a, b, msg in forward:
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            nd.dnn_conv2d_forward(a, b)
        assert str(e.value) == msg
        del e
        assert nd.live_device_allocations() == before
    backward = ((x, ones(2, 4, 4), w, ndim), (x, dy, ones(4, 2, 3, 2), channels), (x, dy, ones(4, 3, 7, 2), window),
                (x, ones(2, 4, 4, 5), w, gradient), (x, ones(2, 3, 4, 6), w, gradient), (x, ones(1, 4, 4, 6), w, gradient),
                (x, host(2, 4, 4, 6), w, device), (x, dy, host(4, 3, 3, 2), device), (host(2, 3, 6, 7), host(2, 4, 4, 6), host(4, 3, 3, 2), cpu))
    for a, g, b, msg in backward:
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            nd.dnn_conv2d_backward(a, g, b)
        assert str(e.value) == msg
        del e
        assert nd.live_device_allocations() == before
    before = nd.live_device_allocations()
    y = nd.dnn_conv2d_forward(x, w)
    assert nd.live_device_allocations() == before + 1 and y.shape() == [2, 4, 4, 6]
    r = nd.dnn_conv2d_backward(x, dy, w)
    assert nd.live_device_allocations() == before + 3 and r[0].shape() == [4, 3, 3, 2] and r[1].shape() == [2, 3, 6, 7]
    del y, r
    gc.collect()
    assert nd.live_device_allocations() == before


def test_c_abi_refusals_leave_the_outputs_untouched_and_nothing_leaks(hip):
    _l, lib = _lib()
    d = hip.DeviceArray.from_host(np.full(512, 5.0, np.float32))
    live = lib.np_live_allocs()
    calls = (lib.np_conv2d_forward, lib.np_conv2d_backward_data, lib.np_conv2d_backward_filter)
    ok = (1, 2, 5, 5, 3, 3, 3, 0, 0)                                          # N, C, H, W, F, kh, kw, ph, pw
    for call in calls:
        for ptrs in ((None, d.ptr, d.ptr), (d.ptr, None, d.ptr), (d.ptr, d.ptr, None)):
            assert call(ptrs[0], ptrs[1], *ok, ptrs[2]) == -1 and b"null pointer" in lib.np_last_error()
        for k in range(7):                                                    # a zero extent
            bad = list(ok)
            bad[k] = 0
            assert call(d.ptr, d.ptr, *bad, d.ptr) == -1 and b"at least 1" in lib.np_last_error()
        assert call(d.ptr, d.ptr, 1, 2, 5, 5, 3, 6, 3, 0, 0, d.ptr) == -1 and b"larger than the padded image" in lib.np_last_error()
        assert call(d.ptr, d.ptr, 1, 2, 5, 5, 3, 3, 10, 0, 2, d.ptr) == -1 and b"larger than the padded image" in lib.np_last_error()
        # 2^31 elements or more are refused, not truncated: numel(x), numel(w), numel(y) / N.P, K, and a single extent
        for big in ((1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0, 0), (1, 1 << 16, 1, 1, 1 << 15, 1, 1, 0, 0), (1 << 16, 1, 1, 1, 1 << 15, 1, 1, 0, 0),
                    (1, 1 << 11, 1 << 10, 1 << 10, 1, 1 << 10, 1 << 10, 0, 0), (1, 1, 1 << 31, 1, 1, 1, 1, 0, 0), (1 << 32, 1, 1, 1, 1, 1, 1, 0, 0)):
            assert call(d.ptr, d.ptr, *big, d.ptr) == -1 and b"2^31" in lib.np_last_error()
    assert np.all(d.to_host() == 5.0) and lib.np_live_allocs() == live
    x, w, dy = D.exact(np.random.default_rng(0), (3, 4, 20, 20), (5, 4, 3, 3))
    _all_abi(hip, x, w, dy)                                                   # scratch (the flipped filters, the slices) went back to the pool
    assert lib.np_live_allocs() == live
    d.free()


@pytest.mark.parametrize("xs,ws,ph,pw", [((3, 4, 9, 11), (5, 4, 3, 4), 0, 0), ((2, 3, 8, 8), (33, 3, 3, 3), 1, 1), ((4, 2, 30, 40), (3, 2, 5, 2), 4, 0)])
def test_adjoint_identities_hold_as_exact_integers(hip, xs, ws, ph, pw):
    """<y, dy> = <x, dX> = <w, dW>, folded in int64 on the host"""
    x, w, dy = D.exact(np.random.default_rng(ws[0]), xs, ws, D.Geo(ph, pw))
    y, dw, dx = _all_abi(hip, x, w, dy, ph, pw)
    dot = lambda a, b: int(np.sum(D.as_int(a) * D.as_int(b)))
    assert dot(y, dy) == dot(x, dx) == dot(w, dw)
