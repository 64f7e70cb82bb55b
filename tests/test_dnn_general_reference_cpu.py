"""The strided / dilated convolution-layer tests' reference (tests/dnn_general_family.py) against torch on the CPU: on the exact
family forward, grad_w and grad_x equal torch.nn.functional.conv2d and its autograd gradients bit for bit for every stride,
dilation and padding below; the data gradient equals the unit-stride forward pass over the zero-stuffed dy with the flipped
filters, the layer's tap dilation and the complementary padding (the identity the device kernel uses), in int64, with floor
remainders 0 and s - 1; np_conv2d_shape_ex agrees with the formula and with torch's output shape on a grid."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import dnn_general_family as G

torch = pytest.importorskip("torch")
NP_ERR_INVALID = -1            # np_hip.h: np_status

# x shape, w shape, Geo(ph, pw, sh, sw, dh, dw).  (H + 2 ph - keh) mod sh and the same along W are the remainders in the comments
SHAPES = [((1, 1, 1, 1), (1, 1, 1, 1), G.Geo()),
          ((2, 3, 7, 9), (4, 3, 3, 3), G.geo(2)),                            # remainders 0, 0
          ((2, 3, 8, 10), (4, 3, 3, 3), G.geo(2)),                           # 1, 1 = s - 1
          ((2, 3, 8, 9), (4, 3, 3, 3), G.geo((2, 3), 1)),                    # 1, 2 = s - 1 with padding
          ((1, 2, 9, 5), (3, 2, 3, 3), G.geo((3, 1))),                       # 0; mixed per axis
          ((2, 2, 13, 14), (3, 2, 3, 3), G.geo(4)),                          # the stride larger than the window: 2, 3 = s - 1
          ((2, 2, 11, 11), (3, 2, 3, 3), G.geo(4, 2)),                       # ph = keh - 1, remainder 0
          ((2, 3, 9, 9), (2, 3, 3, 3), G.geo(1, 0, 2)),                      # dilation alone
          ((2, 3, 9, 10), (2, 3, 3, 2), G.geo(1, (4, 1), (3, 2))),           # dilation (3, 2), ph = keh - 1 - 2
          ((1, 2, 6, 12), (2, 2, 2, 3), G.geo((2, 3), (0, 2), (1, 3))),      # stride and dilation, kh != kw
          ((2, 2, 6, 9), (3, 2, 1, 5), G.geo(2, (0, 4))),                    # 1 x 5 window, pw = kew - 1
          ((3, 4, 7, 7), (5, 4, 1, 1), G.geo(2)),                            # 1 x 1 / 2
          ((2, 2, 3, 3), (2, 2, 3, 3), G.geo(2)),                            # oh = ow = 1
          ((2, 2, 8, 3), (2, 2, 3, 3), G.geo((2, 3), (1, 0))),               # ow = 1
          ((1, 3, 23, 23), (8, 3, 7, 7), G.geo(2, 3)),                       # a 7 x 7 / 2 stem, small
          ((1, 16, 14, 14), (16, 16, 3, 3), G.geo(2, 2, 2))]


def _torch_all(x, w, dy, g):
    tx, tw = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    y = torch.nn.functional.conv2d(tx, tw, stride=(g.sh, g.sw), padding=(g.ph, g.pw), dilation=(g.dh, g.dw))
    y.backward(torch.tensor(dy))
    return y.detach().numpy(), tw.grad.numpy(), tx.grad.numpy()


@pytest.mark.parametrize("xs,ws,g", SHAPES)
def test_the_evaluator_equals_torch_bit_for_bit_on_the_exact_family(xs, ws, g):
    x, w, dy = G.exact(np.random.default_rng(xs[3] + ws[0]), xs, ws, g)
    ix, iw, idy = G.as_int(x), G.as_int(w), G.as_int(dy)
    want = (G.forward(ix, iw, g), G.grad_w(ix, idy, ws[2], ws[3], g), G.grad_x(idy, iw, xs[2], xs[3], g))
    assert want[0].dtype == np.int64 and want[0].shape == (xs[0], ws[0]) + G.out_hw(xs[2], xs[3], ws[2], ws[3], g)
    for got, ref in zip(_torch_all(x, w, dy, g), want):
        assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32))
    for got, ref in zip((G.forward(x, w, g), G.grad_w(x, dy, ws[2], ws[3], g), G.grad_x(dy, w, xs[2], xs[3], g)), want):
        assert got.dtype == np.float64 and np.array_equal(got, ref)             # the float64 path is the same evaluator


def test_unit_geometry_is_the_unit_family():
    from tests import dnn_family as D
    x, w, dy = D.exact(np.random.default_rng(5), (2, 3, 6, 7), (4, 3, 3, 2), D.Geo(1, 1))
    g = G.geo(1, 1)
    assert np.array_equal(G.forward(x, w, g), D.forward(x, w, D.Geo(1, 1)))
    assert np.array_equal(G.grad_w(x, dy, 3, 2, g), D.grad_w(x, dy, 3, 2, D.Geo(1, 1)))
    assert np.array_equal(G.grad_x(dy, w, 6, 7, g), D.grad_x(dy, w, 6, 7, D.Geo(1, 1)))


@pytest.mark.parametrize("xs,ws,g", SHAPES)
def test_the_data_gradient_is_the_forward_pass_over_the_dilated_dy(xs, ws, g):
    _, w, dy = G.exact(np.random.default_rng(xs[2] + ws[1]), xs, ws, g)
    iw, idy = G.as_int(w), G.as_int(dy)
    want = G.grad_x(idy, iw, xs[2], xs[3], g)
    got = G.grad_x_as_forward(idy, iw, xs[2], xs[3], g)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    dead = G.never_read(xs[2], xs[3], ws[2], ws[3], g)
    assert not np.any(want[:, :, dead])                                         # the cells no window reads: the chain over stored zeros


def test_the_shapes_cover_remainders_zero_and_s_minus_one_and_cells_never_read():
    rem = lambda xs, ws, g: ((xs[2] + 2 * g.ph - G.effective(ws[2], ws[3], g)[0]) % g.sh, (xs[3] + 2 * g.pw - G.effective(ws[2], ws[3], g)[1]) % g.sw)
    strided = [(xs, ws, g) for xs, ws, g in SHAPES if g.sh > 1 or g.sw > 1]
    assert len(strided) >= 10
    assert any(rem(*s) == (0, 0) for s in strided) and any(rem(*s) == (s[2].sh - 1, s[2].sw - 1) and s[2].sh > 1 and s[2].sw > 1 for s in strided)
    assert any(G.never_read(xs[2], xs[3], ws[2], ws[3], g).any() for xs, ws, g in strided)
    assert any(g.ph == G.effective(ws[2], ws[3], g)[0] - 1 for _, ws, g in SHAPES if g.sh > 1)


def test_a_strided_forward_is_the_subsample_and_a_dilated_one_the_stuffed_filter():
    x, w, _ = G.exact(np.random.default_rng(3), (2, 3, 11, 12), (4, 3, 3, 2), G.Geo())
    unit = G.forward(x, w, G.geo(1, 1))
    assert np.array_equal(G.forward(x, w, G.geo((2, 3), 1)), unit[:, :, ::2, ::3])
    assert np.array_equal(G.forward(x, w, G.geo(1, 0, (2, 3))), G.forward(x, G.stuffed(w, 2, 3)))
    assert G.stuffed(w, 2, 3).shape == (4, 3, 5, 4) and np.array_equal(G.stuffed(w, 2, 3)[:, :, ::2, ::3], w)


def test_a_nan_in_a_cell_no_window_reads_reaches_nothing():
    g = G.geo(4)
    x, w, dy = G.gaussian((1, 2, 12, 12), (3, 2, 3, 3), g)
    dead = G.never_read(12, 12, 3, 3, g)
    assert dead[3, 3] and dead[11, 0] and not dead[4, 4]
    x[0, 1, 3, 3] = np.nan
    assert not np.isnan(G.forward(x, w, g)).any() and not np.isnan(G.grad_w(x, dy, 3, 3, g)).any()
    x[0, 1, 4, 4] = np.nan
    assert np.isnan(G.forward(x, w, g)).sum() == 3                              # one pixel of every filter


def test_shape_ex_equals_the_formula_and_torch_on_a_grid():
    from numpower_amd import _lib
    lib = _lib.load()
    oh, ow = C.c_size_t(), C.c_size_t()
    seen = 0
    for H, W, kh, kw, s, d in itertools.product((1, 5, 8, 13), (3, 9), (1, 2, 3), (1, 3), ((1, 1), (2, 3), (4, 1)), ((1, 1), (2, 1), (1, 3))):
        g0 = G.Geo(0, 0, *s, *d)
        keh, kew = G.effective(kh, kw, g0)
        for ph, pw in ((0, 0), (keh // 2, kew // 2), (keh - 1, kew - 1)):
            g = G.Geo(ph, pw, *s, *d)
            rc = lib.np_conv2d_shape_ex(H, W, kh, kw, ph, pw, g.sh, g.sw, g.dh, g.dw, C.byref(oh), C.byref(ow))
            if keh > H + 2 * ph or kew > W + 2 * pw:
                assert rc == NP_ERR_INVALID and b"larger than the padded image" in lib.np_last_error()
                continue
            assert rc == _lib.NP_OK and (oh.value, ow.value) == G.out_hw(H, W, kh, kw, g)
            t = torch.nn.functional.conv2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, kh, kw), stride=s, padding=(ph, pw), dilation=d)
            assert tuple(t.shape[2:]) == (oh.value, ow.value)
            seen += 1
    assert seen > 300
