"""The pooling evaluator (tests/dnn_pool_family.py) against torch on the CPU, bit for bit: y, idx and dx of all three modes
(count_include_pad True for 'avg', False for 'avg_valid') on the exact family and on Gaussian data, over windows 1x1, 2x2, 3x3, 2x3,
5x1 and 7x7, strides 1, 2, 3, (2, 1) and one larger than the window, paddings 0 and k // 2; y and idx with NaNs planted; and
np_pool2d_shape against the formula and torch's result shape."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dnn_pool_family as P

WINDOWS = [(1, 1), (2, 2), (3, 3), (2, 3), (5, 1), (7, 7)]
STRIDES = [1, 2, 3, (2, 1), "larger"]
H, W, PLANES = 17, 15, 3


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _grid():
    for k in WINDOWS:
        for s in STRIDES:
            s = (k[0] + 1, k[1] + 1) if s == "larger" else P.pair(s)
            for p in ((0, 0), (k[0] // 2, k[1] // 2)):
                yield k, s, p


def _torch(x, dy, k, s, p, mode):
    """-> y, idx or None, dx, computed by torch on the CPU"""
    t = torch.from_numpy(x[None].copy()).requires_grad_(True)
    idx = None
    if mode == "max":
        y, ti = F.max_pool2d(t, k, s, p, return_indices=True)
        idx = ti[0].numpy().astype(np.int32)
    else:
        y = F.avg_pool2d(t, k, s, p, ceil_mode=False, count_include_pad=mode == "avg")
    dx = None
    if dy is not None:
        y.backward(torch.from_numpy(dy[None].copy()))
        dx = t.grad[0].numpy()
    return y.detach()[0].numpy(), idx, dx


@pytest.mark.parametrize("mode", ["max", "avg", "avg_valid"])
@pytest.mark.parametrize("family", ["exact", "gaussian"])
def test_the_evaluator_is_torch_bit_for_bit(mode, family):
    rng = np.random.default_rng(7)
    for k, s, p in _grid():
        x, dy = (P.exact if family == "exact" else P.gaussian)(rng, PLANES, H, W, k, s, p)
        y, idx = P.forward(x, k, s, p, mode)
        dx = P.backward(dy, idx, x.shape, k, s, p, mode)
        ty, tidx, tdx = _torch(x, dy, k, s, p, mode)
        assert _same(y, ty), ("y", k, s, p)
        assert mode != "max" or (idx.dtype == np.int32 and np.array_equal(idx, tidx)), ("idx", k, s, p)
        assert _same(dx, tdx), ("dx", k, s, p)
        if family == "exact" and mode == "max" and k != (1, 1):      # the planted ties are there: a maximum 9 held by several cells
            win = np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (p[0],) * 2, (p[1],) * 2), constant_values=-np.inf), k, (1, 2))
            win = win[:, ::s[0], ::s[1]]
            assert ((win == y[..., None, None]).sum((3, 4)) > 1).any(), (k, s, p)


def test_exact_sums_are_integers_and_the_division_is_the_correctly_rounded_one():
    rng = np.random.default_rng(8)
    x, dy = P.exact(rng, 2, 9, 9, (3, 3), (1, 1), (1, 1))
    y, _ = P.forward(x, 3, 1, 1, "avg")
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, ((0, 0), (1, 1), (1, 1))).astype(np.float64), (3, 3), (1, 2)).sum((3, 4))
    assert np.array_equal(y, (win / 9.0).astype(np.float32))         # float64 quotient of small integers, rounded once
    assert not np.array_equal(y, (win.astype(np.float32) * np.float32(1.0 / 9.0)))      # a reciprocal would be caught


def test_nan_values_and_indices_are_torchs():
    rng = np.random.default_rng(9)
    for k, s, p in _grid():
        x, _ = P.gaussian(rng, PLANES, H, W, k, s, p)
        x[rng.random(x.shape) < 0.08] = np.nan
        x[0, 0, 0] = x[1, H - 1, W - 1] = np.nan
        y, idx = P.forward(x, k, s, p, "max")
        ty, tidx, _ = _torch(x, None, k, s, p, "max")
        assert _same(np.isnan(y), np.isnan(ty)) and np.array_equal(np.nan_to_num(y), np.nan_to_num(ty)), (k, s, p)
        assert np.array_equal(idx, tidx), (k, s, p)
        if k[0] * k[1] > 1:      # the LAST NaN of a window keeps the index
            both = np.isnan(y)
            assert both.any() and np.isnan(x.reshape(PLANES, -1)[np.nonzero(both)[0], idx[both]]).all()
        for mode in ("avg", "avg_valid"):
            y, _ = P.forward(x, k, s, p, mode)
            assert np.array_equal(np.isnan(y), np.isnan(_torch(x, None, k, s, p, mode)[0])), (mode, k, s, p)


def test_the_shape_call_is_the_formula_and_torchs():
    from numpower_amd import _lib
    lib = _lib.load()
    for Hh, Ww in ((1, 1), (2, 7), (7, 8), (17, 15), (64, 65)):
        for k, s, p in _grid():
            oh, ow = C.c_size_t(0), C.c_size_t(0)
            rc = lib.np_pool2d_shape(Hh, Ww, *k, *p, *s, C.byref(oh), C.byref(ow))
            if k[0] > Hh + 2 * p[0] or k[1] > Ww + 2 * p[1]:
                assert rc == -1 and b"larger than the padded image" in lib.np_last_error()
                continue
            assert rc == _lib.NP_OK
            assert (oh.value, ow.value) == P.out_hw(Hh, Ww, k, s, p) == ((Hh + 2 * p[0] - k[0]) // s[0] + 1, (Ww + 2 * p[1] - k[1]) // s[1] + 1)
            assert tuple(F.max_pool2d(torch.zeros(1, 1, Hh, Ww), k, s, p).shape[2:]) == (oh.value, ow.value)
