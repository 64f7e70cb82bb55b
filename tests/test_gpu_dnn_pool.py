"""GPU tests of the pooling layers (np_pool.hip: np_pool2d_forward, np_pool2d_backward; NDArray.dnn_pool2d_forward / _backward),
bit for bit against the evaluator of tests/dnn_pool_family.py (which tests/test_dnn_pool_reference_cpu.py holds against torch),
through the C ABI and through NDArray.

1. nine windows (WINDOWS) x extents from {1, 2, 7, 8, 63, 64, 65, 130} x planes 1, 3, 65 x the three modes, on the exact
   family (integers with planted ties) and on Gaussian data: y, idx and dx by bits; idx == NULL gives the same y; the probe;
2. outputs and cells on either side of the block constant, 256 lanes per workgroup; both forward forms, asserted by the probe: planes
   of H.W on either side of 8192 cells, plane counts on either side of a staged workgroup's share, and the two forms bit for bit on
   shapes both accept;
3. ties, a window of all -Inf, -0.0 against +0.0;
4. NaN footprints of x in y and idx and of dy in dx; a NaN in a cell no window reads reaches nothing; uncovered cells are +0.0;
5. three runs are bit-identical; a plane alone equals the same plane in a batch of 5;
6. the adjoint identity of the average modes on integers with power-of-two divisors;
7. the surface: views and pending chains, the device message, no leaked allocation (the max backward's scratch included);
   examples/conv_pool_classifier.py trains on the device and its loss falls."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import dnn_pool_family as P

pytestmark = pytest.mark.gpu
MODES = ("max", "avg", "avg_valid")
BLOCK = 256                       # kPoolBlock of np_pool.hip: lanes per workgroup
STAGE = 8192                      # kStageCells: planes of at most this many cells take the staged forward form, floor(STAGE / (H.W)) to a workgroup
# (window, stride, padding); None: window = image
WINDOWS = {"2x2/2": ((2, 2), (2, 2), (0, 0)), "3x3/2p1": ((3, 3), (2, 2), (1, 1)), "3x3/1p1": ((3, 3), (1, 1), (1, 1)),
           "1x1/1": ((1, 1), (1, 1), (0, 0)), "2x3/(2,1)": ((2, 3), (2, 1), (0, 0)), "5x1/1p(2,0)": ((5, 1), (1, 1), (2, 0)),
           "7x7/3p3": ((7, 7), (3, 3), (3, 3)), "image": None, "3x3/4": ((3, 3), (4, 4), (0, 0))}
# (planes, H, W): every extent of the list along both axes, every planes count with a small and a large plane
EXTENTS = [(1, 1, 1), (3, 2, 3), (1, 3, 3), (3, 2, 7), (65, 7, 8), (3, 8, 2), (1, 63, 64), (3, 64, 65), (65, 65, 63), (1, 130, 7), (3, 7, 130), (65, 1, 2), (1, 8, 130), (3, 130, 64), (1, 65, 130)]


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
    _l, lib = _lib()
    f, b = C.c_int(-1), C.c_int(-1)
    _l.check(lib.np_debug_pool_last_path(C.byref(f), C.byref(b)))
    return f.value, b.value


def _geometry(name, H, W):
    """-> (k, s, p) or None where the window does not fit the padded plane"""
    if WINDOWS[name] is None:
        return (H, W), (H, W), (0, 0)
    k, s, p = WINDOWS[name]
    return (k, s, p) if k[0] <= H + 2 * p[0] and k[1] <= W + 2 * p[1] else None


def _fwd(hip, x, k, s, p, mode, with_idx=True):
    """np_pool2d_forward on a host array -> y, idx (None without with_idx)"""
    _l, lib = _lib()
    planes, H, W = x.shape
    ys = (planes,) + P.out_hw(H, W, k, s, p)
    dx, dy, di = hip.DeviceArray.from_host(x), hip.DeviceArray(ys), hip.DeviceArray(ys) if with_idx else None
    try:
        _l.check(lib.np_pool2d_forward(dx.ptr, planes, H, W, *k, *p, *s, P.MODE[mode], dy.ptr, di.ptr if di else None))
        return dy.to_host(), di.to_host().view(np.int32) if di else None
    finally:
        for d in (dx, dy, di):
            if d is not None:
                d.free()


def _bwd(hip, dy, idx, xshape, k, s, p, mode):
    """np_pool2d_backward on host arrays -> dx"""
    _l, lib = _lib()
    planes, H, W = xshape
    g, out = hip.DeviceArray.from_host(dy), hip.DeviceArray(xshape)
    di = hip.DeviceArray.from_host(np.ascontiguousarray(idx, np.int32).view(np.float32)) if idx is not None else None
    try:
        _l.check(lib.np_pool2d_backward(g.ptr, di.ptr if di else None, planes, H, W, *k, *p, *s, P.MODE[mode], out.ptr))
        return out.to_host()
    finally:
        for d in (g, out, di):
            if d is not None:
                d.free()


def _check(hip, x, dy, k, s, p, mode, tag):
    y, idx = P.forward(x, k, s, p, mode)
    dx = P.backward(dy, idx, x.shape, k, s, p, mode)
    gy, gi = _fwd(hip, x, k, s, p, mode)
    assert _same(gy, y), ("y", tag)
    assert mode != "max" or np.array_equal(gi, idx), ("idx", tag)
    gx = _bwd(hip, dy, idx, x.shape, k, s, p, mode)
    assert _same(gx, dx), ("dx", tag)
    return y, idx, dx


# ---- 1. every window, extent and mode -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(WINDOWS))
def test_every_window_extent_and_mode_by_bits(hip, name):
    rng = np.random.default_rng(len(name) + 17 * list(WINDOWS).index(name))
    ran, remainders, single = 0, set(), False
    for planes, H, W in EXTENTS:
        geo = _geometry(name, H, W)
        if geo is None:
            continue
        k, s, p = geo
        remainders.add(((H + 2 * p[0] - k[0]) % s[0], s[0]))
        single = single or P.out_hw(H, W, k, s, p) == (1, 1)
        for family in (P.exact, P.gaussian):
            x, dy = family(rng, planes, H, W, k, s, p)
            for mode in MODES:
                _check(hip, x, dy, k, s, p, mode, (name, planes, H, W, family.__name__, mode))
                assert _probe() == (2 if H * W <= STAGE else 1, 1)
                ran += 1
        x, _ = P.gaussian(rng, planes, H, W, k, s, p)
        assert _same(_fwd(hip, x, k, s, p, "max", with_idx=False)[0], P.forward(x, k, s, p, "max")[0])      # idx == NULL: the same y
    assert ran >= 6 * 6 and single                                                    # oh = ow = 1 is among them
    if name in ("2x2/2", "3x3/2p1", "7x7/3p3", "3x3/4"):                              # floor remainders 0 and s - 1
        s0 = WINDOWS[name][1][0]
        assert {(0, s0), (s0 - 1, s0)} <= remainders, remainders


@pytest.mark.parametrize("name", ["2x2/2", "3x3/2p1", "5x1/1p(2,0)", "image", "3x3/4"])
def test_through_ndarray_max_backward_finds_its_maxima_again(hip, name):
    nd = _nd()
    rng = np.random.default_rng(5)
    for (N, Cc), H, W in (((1, 1), 7, 8), ((1, 3), 8, 7), ((5, 13), 9, 10), ((2, 2), 64, 65)):
        geo = _geometry(name, H, W)
        if geo is None:
            continue
        k, s, p = geo
        for family in (P.exact, P.gaussian):
            x, dy = family(rng, N * Cc, H, W, k, s, p)
            for mode in MODES:
                y, idx = P.forward(x, k, s, p, mode)
                dx = P.backward(dy, idx, x.shape, k, s, p, mode)
                kw = {} if WINDOWS[name] is not None and s == k and p == (0, 0) else {"stride": s, "padding": p}      # the defaults: stride = the window
                gy = nd.dnn_pool2d_forward(_gpu(x.reshape(N, Cc, H, W)), k, mode=mode, **kw)
                assert gy.shape() == [N, Cc, y.shape[1], y.shape[2]] and _same(gy.cpu().numpy().reshape(y.shape), y), (name, mode)
                gx = nd.dnn_pool2d_backward(_gpu(x.reshape(N, Cc, H, W)), _gpu(dy.reshape((N, Cc) + dy.shape[1:])), k, mode=mode, **kw)
                assert gx.shape() == [N, Cc, H, W] and _same(gx.cpu().numpy().reshape(dx.shape), dx), (name, mode)
    x = np.arange(2 * 3 * 6 * 6, dtype=np.float32).reshape(2, 3, 6, 6)               # ints for a square window, stride and padding
    want = P.forward(x.reshape(6, 6, 6), 3, 2, 1, "avg_valid")[0].reshape(2, 3, 3, 3)
    assert _same(nd.dnn_pool2d_forward(_gpu(x), 3, stride=2, padding=1, mode="avg_valid").cpu().numpy(), want)


# ---- 2. the block constant --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_either_side_of_the_workgroup(hip, n):
    """n outputs (2x2/2 over (2, 2n)) and n cells (1x1/1 over (1, n)); then n cells and n / 2 outputs in one plane row"""
    rng = np.random.default_rng(n)
    for planes, H, W, k, s, p in ((1, 2, 2 * n, (2, 2), (2, 2), (0, 0)), (1, 1, n, (1, 1), (1, 1), (0, 0)), (1, 1, n, (1, 2), (1, 2), (0, 0)),
                                  (n, 1, 1, (1, 1), (1, 1), (0, 0)), (n, 2, 2, (3, 3), (1, 1), (1, 1))):
        x, dy = P.exact(rng, planes, H, W, k, s, p, ties=1 if planes > 8 else 6)
        for mode in MODES:
            _check(hip, x, dy, k, s, p, mode, (n, planes, H, W, mode))
    # nothing is written past the end: guard words behind y, idx and dx
    _l, lib = _lib()
    k, s, p = (2, 2), (2, 2), (0, 0)
    x, dy = P.gaussian(rng, 1, 2, 2 * n, k, s, p)
    y, idx = P.forward(x, k, s, p, "max")
    dev_x, out = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(np.full(6 * n + 32, 777.0, np.float32))
    try:
        _l.check(lib.np_pool2d_forward(dev_x.ptr, 1, 2, 2 * n, *k, *p, *s, 0, out.view(8, (n,)).ptr, out.view(n + 16, (n,)).ptr))
        _l.check(lib.np_pool2d_backward(out.view(8, (n,)).ptr, out.view(n + 16, (n,)).ptr, 1, 2, 2 * n, *k, *p, *s, 0, out.view(2 * n + 24, (4 * n,)).ptr))
        got = out.to_host()
    finally:
        dev_x.free()
        out.free()
    assert _same(got[8:8 + n], y.ravel()) and np.array_equal(got[n + 16:2 * n + 16].view(np.int32), idx.ravel())
    assert _same(got[2 * n + 24:6 * n + 24], P.backward(y, idx, x.shape, k, s, p, "max").ravel())
    assert (got[:8] == 777.0).all() and (got[n + 8:n + 16] == 777.0).all() and (got[2 * n + 16:2 * n + 24] == 777.0).all() and (got[6 * n + 24:] == 777.0).all() and got.size == 6 * n + 32


def _forced_direct(hip, x, k, s, p, mode):
    _l, lib = _lib()
    _l.check(lib.np_debug_pool_forward_form(1))
    try:
        got = _fwd(hip, x, k, s, p, mode)
        assert _probe()[0] == 1
        return got
    finally:
        _l.check(lib.np_debug_pool_forward_form(0))


@pytest.mark.parametrize("planes,H,W", [(2, 64, 128), (2, 1, STAGE), (2, 1, STAGE + 1), (1, 3, 2731), (3, 128, 64), (2, 129, 64), (1, 91, 90), (1, 91, 91),
                                        (166, 7, 7), (167, 7, 7), (168, 7, 7), (335, 7, 7), (2, 2048, 2), (4, 2048, 2), (5, 2, 2048)])
def test_both_forward_forms_by_the_probe_and_bit_for_bit(hip, planes, H, W):
    """H.W = 8192 is staged, 8193 and more direct; 7 x 7 planes go 167 to a workgroup: 166, 167, 168 and 335 planes"""
    rng = np.random.default_rng(planes + H)
    for name in ("2x2/2", "3x3/2p1", "5x1/1p(2,0)", "image", "1x1/1"):
        geo = _geometry(name, H, W)
        if geo is None:
            continue
        k, s, p = geo
        x, _ = P.gaussian(rng, planes, H, W, k, s, p)
        x[rng.random(x.shape) < 0.01] = np.nan
        for mode in MODES:
            y, idx = P.forward(x, k, s, p, mode)
            gy, gi = _fwd(hip, x, k, s, p, mode)
            assert _probe()[0] == (2 if H * W <= STAGE else 1), (H, W)
            assert _same(gy, y) and (mode != "max" or np.array_equal(gi, idx)), (name, mode)
            dy, di = _forced_direct(hip, x, k, s, p, mode)
            assert _same(dy, gy) and (mode != "max" or np.array_equal(di, gi)), (name, mode)


# ---- 3. ties, -Inf, signed zeros -----------------------------------------------------------------------------------------------------------

def test_the_first_maximum_wins_all_minus_inf_and_signed_zeros(hip):
    k, s, p = (3, 3), (2, 2), (1, 1)
    x = np.full((3, 7, 8), 5.0, np.float32)                      # every cell ties: the first REAL cell of every window
    y, idx = _fwd(hip, x, k, s, p, "max")
    oh, ow = P.out_hw(7, 8, k, s, p)
    first = (np.maximum(np.arange(oh) * 2 - 1, 0)[:, None] * 8 + np.maximum(np.arange(ow) * 2 - 1, 0)[None, :]).astype(np.int32)
    assert (y == 5.0).all() and np.array_equal(idx, np.broadcast_to(first, idx.shape))
    dy = np.arange(1, 3 * oh * ow + 1, dtype=np.float32).reshape(3, oh, ow)
    dx = _bwd(hip, dy, idx, x.shape, k, s, p, "max")
    want = np.zeros_like(x)
    for pl in range(3):
        np.add.at(want[pl].reshape(-1), first.ravel(), dy[pl].ravel())      # first cells are distinct: one term each, exact
    assert _same(dx, want) and _same(dx, P.backward(dy, idx, x.shape, k, s, p, "max"))

    x = np.full((2, 7, 8), -np.inf, np.float32)                 # nothing beats -Inf: idx stays the first real cell
    x[1, 3, 3] = 1.0
    y, idx = _fwd(hip, x, k, s, p, "max")
    assert np.array_equal(idx[0], first) and np.isneginf(y[0]).all()
    holds = np.zeros((oh, ow), bool)
    holds[1:3, 1:3] = True                                      # rows 2i - 1 ... 2i + 1 hold row 3 for i = 1, 2
    assert np.array_equal(y[1] == 1.0, holds) and np.isneginf(y[1][~holds]).all() and (idx[1][holds] == 3 * 8 + 3).all()
    assert np.array_equal(idx[1][~holds], first[~holds])
    for mode in ("avg", "avg_valid"):
        assert np.isneginf(_fwd(hip, x[:1], k, s, p, mode)[0]).all()

    for a, b in ((-0.0, 0.0), (0.0, -0.0)):                     # equal: the first one stays, with its sign
        x = np.array([[[a, b, a, b]]], np.float32)
        y, idx = _fwd(hip, x, (1, 2), (1, 2), (0, 0), "max")
        assert np.array_equal(idx.ravel(), [0, 2]) and _same(y.ravel(), np.array([a, a], np.float32))
        assert _same(y, P.forward(x, (1, 2), (1, 2), (0, 0), "max")[0])
    x = np.array([[[-0.0, -0.0]]], np.float32)                   # the average's chain starts from +0.0f
    for mode in ("avg", "avg_valid"):
        assert _bits(_fwd(hip, x, (1, 2), (1, 2), (0, 0), mode)[0]).ravel()[0] == 0


# ---- 4. NaN footprints and uncovered cells -------------------------------------------------------------------------------------------------

def _holds(cell, k, s, p, H, W):
    """the windows (oh, ow) bool that hold cell (u, v), from the definition"""
    oh, ow = P.out_hw(H, W, k, s, p)
    i, j = np.arange(oh)[:, None] * s[0] - p[0], np.arange(ow)[None, :] * s[1] - p[1]
    return (i <= cell[0]) & (cell[0] < i + k[0]) & (j <= cell[1]) & (cell[1] < j + k[1])


@pytest.mark.parametrize("name", ["3x3/2p1", "3x3/1p1", "2x3/(2,1)", "7x7/3p3", "3x3/4"])
def test_nan_footprints(hip, name):
    k, s, p = WINDOWS[name]
    planes, H, W = 3, 15, 14
    rng = np.random.default_rng(3)
    x, dy = P.gaussian(rng, planes, H, W, k, s, p)
    clean = {m: _fwd(hip, x, k, s, p, m) for m in MODES}
    for cell in ((0, 0), (7, 6), (H - 1, W - 1), (3, 3)):
        bad = x.copy()
        bad[1, cell[0], cell[1]] = np.nan
        holds = _holds(cell, k, s, p, H, W)
        for mode in MODES:
            y, idx = _fwd(hip, bad, k, s, p, mode)
            assert np.array_equal(np.isnan(y[1]), holds), (name, cell, mode)
            assert _same(y[[0, 2]], clean[mode][0][[0, 2]]) and _same(y[1][~holds], clean[mode][0][1][~holds])
            if mode == "max":
                assert (idx[1][holds] == cell[0] * W + cell[1]).all() and np.array_equal(idx[1][~holds], clean[mode][1][1][~holds])
            assert _same(y, P.forward(bad, k, s, p, mode)[0])
    two = x.copy()                                               # two NaNs in one window: the index is the LAST one's
    two[0, 4, 4] = two[0, 4, 5] = np.nan
    y, idx = _fwd(hip, two, k, s, p, "max")
    both = _holds((4, 4), k, s, p, H, W) & _holds((4, 5), k, s, p, H, W)
    assert both.any() and (idx[0][both] == 4 * W + 5).all() and np.array_equal(idx, P.forward(two, k, s, p, "max")[1])

    oh, ow = P.out_hw(H, W, k, s, p)
    _, idx = P.forward(x, k, s, p, "max")
    for i, j in ((0, 0), (oh // 2, ow // 2), (oh - 1, ow - 1)):
        bad = dy.copy()
        bad[2, i, j] = np.nan
        for mode in MODES:
            dx = _bwd(hip, bad, idx, x.shape, k, s, p, mode)
            reach = np.zeros((H, W), bool)
            if mode == "max":
                reach.reshape(-1)[idx[2, i, j]] = True          # the one cell that term is added to
            else:
                reach[max(i * s[0] - p[0], 0):i * s[0] - p[0] + k[0], max(j * s[1] - p[1], 0):j * s[1] - p[1] + k[1]] = True
            assert np.array_equal(np.isnan(dx[2]), reach) and not np.isnan(dx[:2]).any(), (name, i, j, mode)
            assert _same(dx, P.backward(bad, idx, x.shape, k, s, p, mode))


def test_cells_no_window_reads(hip):
    """3x3 stride 4 over 15 x 14: rows 3, 7, 11 and columns 3, 7, 11, 12, 13 are read by no window"""
    k, s, p = WINDOWS["3x3/4"]
    planes, H, W = 3, 15, 14
    x, dy = P.gaussian(np.random.default_rng(4), planes, H, W, k, s, p)
    dy = -np.abs(dy)                                            # negative terms only: a product or a -0.0 start would show
    covered = np.zeros((H, W), bool)
    for cell in np.ndindex(H, W):
        covered[cell] = _holds(cell, k, s, p, H, W).any()
    assert not covered[3].any() and not covered[:, 12:].any() and covered[14, 10] and covered.sum() == 4 * 3 * 9
    bad = x.copy()
    bad[:, ~covered] = np.nan
    for mode in MODES:
        y, idx = _fwd(hip, x, k, s, p, mode)
        yb, ib = _fwd(hip, bad, k, s, p, mode)
        assert _same(y, yb) and (mode != "max" or np.array_equal(idx, ib))            # a NaN there reaches nothing
        dx = _bwd(hip, dy, idx, x.shape, k, s, p, mode)
        assert (_bits(dx)[:, ~covered] == 0).all(), mode                              # +0.0 by bits
        assert (dx[:, covered] != 0).any() and _same(dx, P.backward(dy, idx, x.shape, k, s, p, mode))


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------------

def test_three_runs_are_identical_and_a_plane_does_not_see_its_batch(hip):
    rng = np.random.default_rng(6)
    for name, (H, W) in (("3x3/2p1", (63, 65)), ("7x7/3p3", (64, 63)), ("2x2/2", (130, 8))):
        k, s, p = WINDOWS[name]
        x, dy = P.gaussian(rng, 5, H, W, k, s, p)
        for mode in MODES:
            runs = [_fwd(hip, x, k, s, p, mode) for _ in range(3)]
            assert all(_same(r[0], runs[0][0]) for r in runs[1:]) and (mode != "max" or all(np.array_equal(r[1], runs[0][1]) for r in runs[1:]))
            idx = runs[0][1]
            back = [_bwd(hip, dy, idx, x.shape, k, s, p, mode) for _ in range(3)]
            assert all(_same(b, back[0]) for b in back[1:])
            for pl in (0, 3, 4):
                y1, i1 = _fwd(hip, x[pl:pl + 1], k, s, p, mode)
                assert _same(y1[0], runs[0][0][pl]) and (mode != "max" or np.array_equal(i1[0], idx[pl]))
                d1 = _bwd(hip, dy[pl:pl + 1], None if idx is None else idx[pl:pl + 1], (1, H, W), k, s, p, mode)
                assert _same(d1[0], back[0][pl])


# ---- 6. the adjoint identity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,k,s,p", [("avg", (2, 2), (2, 2), (0, 0)), ("avg", (4, 4), (2, 2), (2, 2)), ("avg", (2, 8), (1, 3), (1, 4)),
                                        ("avg_valid", (2, 2), (2, 2), (0, 0)), ("avg_valid", (2, 2), (1, 1), (1, 1)), ("avg_valid", (4, 2), (4, 1), (0, 1))])
def test_the_adjoint_identity_on_integers_with_power_of_two_divisors(hip, mode, k, s, p):
    """sum y.dy == sum x.dx: every quotient is a dyadic rational, every sum exact in fp32 and fp64, so the identity is an equality"""
    planes, H, W = 3, 16, 17
    x, dy = P.exact(np.random.default_rng(11), planes, H, W, k, s, p)
    d = P.divisors(x.shape, k, s, p, mode)
    assert (np.log2(d) % 1 == 0).all()
    y, _ = _fwd(hip, x, k, s, p, mode)
    dx = _bwd(hip, dy, None, x.shape, k, s, p, mode)
    assert _same(y, P.forward(x, k, s, p, mode)[0]) and _same(dx, P.backward(dy, None, x.shape, k, s, p, mode))
    lhs, rhs = (y.astype(np.float64) * dy).sum(), (x.astype(np.float64) * dx).sum()
    assert lhs == rhs and lhs != 0.0


# ---- 7. the surface ----------------------------------------------------------------------------------------------------------------------

def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    k, s, p = (3, 2), (2, 1), (1, 1)
    N, Cc, H, W = 2, 3, 10, 12
    x, dy = P.gaussian(np.random.default_rng(12), N * Cc, H, W, k, s, p)
    x4, dy4 = x.reshape(N, Cc, H, W), dy.reshape((N, Cc) + dy.shape[1:])
    for mode in MODES:
        y, idx = P.forward(x, k, s, p, mode)
        dx = P.backward(dy, idx, x.shape, k, s, p, mode)
        kw = {"stride": s, "padding": p, "mode": mode}
        xt = nd.transpose(_gpu(np.ascontiguousarray(x4.transpose(3, 2, 1, 0))))               # a strided view: all axes reversed
        dyt = nd.transpose(_gpu(np.ascontiguousarray(dy4.transpose(3, 2, 1, 0))))
        assert _same(nd.dnn_pool2d_forward(xt, k, **kw).cpu().numpy().reshape(y.shape), y)
        assert _same(nd.dnn_pool2d_backward(xt, dyt, k, **kw).cpu().numpy().reshape(dx.shape), dx)
        nd.set_lazy_binding(True)
        try:
            got = nd.dnn_pool2d_forward((_gpu(x4) * 2.0) * 0.5, k, **kw)                         # pending chains
            assert _same(got.cpu().numpy().reshape(y.shape), y)
            got = nd.dnn_pool2d_backward((_gpu(x4) * 2.0) * 0.5, (_gpu(dy4) * 4.0) * 0.25, k, **kw)
            assert _same(got.cpu().numpy().reshape(dx.shape), dx)
        finally:
            nd.set_lazy_binding(False)


def test_messages_and_nothing_leaks(hip):
    from tests.test_dnn_pool_glue_cpu import MESSAGES
    from numpower_amd.ndarray import Error
    nd = _nd()
    ones = lambda *sh: _gpu(np.ones(sh, np.float32))
    cpu = lambda *sh: nd.array(np.ones(sh, np.float32))
    x, dy = ones(2, 3, 8, 9), ones(2, 3, 4, 4)
    cases = [(lambda: nd.dnn_pool2d_forward(ones(3, 8, 9), 2), "NDIM"), (lambda: nd.dnn_pool2d_backward(x, ones(2, 3, 16), 2), "NDIM"),
             (lambda: nd.dnn_pool2d_forward(x, (2, 0)), "WINDOW"), (lambda: nd.dnn_pool2d_forward(x, 2, stride=(0, 1)), "STRIDE"),
             (lambda: nd.dnn_pool2d_forward(x, 3, padding=2), "PADDING"), (lambda: nd.dnn_pool2d_backward(x, dy, 2, padding=-1), "PADDING"),
             (lambda: nd.dnn_pool2d_forward(x, (9, 3)), "LARGER"), (lambda: nd.dnn_pool2d_backward(x, dy, (3, 12), padding=1), "LARGER"),
             (lambda: nd.dnn_pool2d_backward(x, ones(2, 3, 4, 5), 2), "GRADIENT"), (lambda: nd.dnn_pool2d_backward(x, dy, 2, mode="avg", stride=1), "GRADIENT"),
             (lambda: nd.dnn_pool2d_backward(x, cpu(2, 3, 4, 4), 2), "DEVICE"), (lambda: nd.dnn_pool2d_backward(cpu(2, 3, 8, 9), dy, 2, mode="avg"), "DEVICE"),
             (lambda: nd.dnn_pool2d_forward(cpu(2, 3, 8, 9), 2), "CPU"), (lambda: nd.dnn_pool2d_backward(cpu(2, 3, 8, 9), cpu(2, 3, 4, 4), 2), "CPU")]
    for call, name in cases:
        gc.collect()
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == MESSAGES["NPH_POOL_MSG_" + name]
        del e
        gc.collect()
        assert nd.live_device_allocations() == before, name
    _l, lib = _lib()
    gc.collect()
    before, pool = nd.live_device_allocations(), lib.np_live_allocs()
    results = [nd.dnn_pool2d_forward(x, 2, mode=m) for m in MODES] + [nd.dnn_pool2d_backward(x, dy, 2, mode=m) for m in MODES]
    gc.collect()
    assert nd.live_device_allocations() == before + 6
    assert [r.shape() for r in results] == [[2, 3, 4, 4]] * 3 + [[2, 3, 8, 9]] * 3
    assert np.array_equal(results[3].cpu().numpy()[0, 0], np.kron(np.ones((4, 4)), [[1, 0], [0, 0]]).astype(np.float32) @ np.eye(8, 9, dtype=np.float32))
    assert np.array_equal(results[4].cpu().numpy()[..., :8], np.full((2, 3, 8, 8), 0.25, np.float32)) and (results[4].cpu().numpy()[..., 8] == 0).all()
    del results
    gc.collect()
    assert nd.live_device_allocations() == before and lib.np_live_allocs() == pool           # the max backward's y and idx went back to the pool


def test_the_example_trains_a_pooling_classifier_on_the_device(hip):
    """examples/conv_pool_classifier.py: conv + relu, a 2x2/2 max pool, a conv, a global average pool; the loss falls"""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("conv_pool_classifier", Path(__file__).resolve().parent.parent / "examples" / "conv_pool_classifier.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, Y, labels = ex.make_problem(128)
    params, losses, logit = ex.train_gpu(X, Y, 25, 0.03)
    assert np.isfinite(losses).all() and losses[-1] < 0.2 * losses[0]
    assert [a.shape() for a in params] == [[8, 1, 3, 3], [8], [4, 8, 3, 3], [4]]
    assert logit.shape == (128, 4) and np.mean(np.argmax(logit, axis=1) == labels) > 0.9
