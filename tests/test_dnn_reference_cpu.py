"""The convolution-layer tests' reference (tests/dnn_family.py) against torch on the CPU: on the exact family forward, grad_w and
grad_x equal torch.nn.functional.conv2d and its autograd gradients bit for bit, with and without padding; the data gradient
equals the forward pass over dy with the flipped filters and the complementary padding (the identity the device kernel uses);
and on standard-normal data torch's fp32 result lies inside the bound the GPU tests hold the device to, far inside it (torch
measured 0.9 - 4.8 u sum|a||b| for K from 45 to 3200), so that bound is not vacuous."""
import numpy as np
import pytest

from tests import dnn_family as D

torch = pytest.importorskip("torch")

# from 1 x 1 x 1 x 1 to (1, 64, 14, 14) * (64, 64, 3, 3): x shape, w shape, (ph, pw)
SHAPES = [((1, 1, 1, 1), (1, 1, 1, 1), (0, 0)), ((2, 3, 6, 7), (4, 3, 3, 2), (0, 0)), ((3, 2, 9, 4), (2, 2, 2, 3), (1, 2)),
          ((5, 3, 9, 9), (6, 3, 3, 3), (1, 1)), ((2, 2, 6, 9), (3, 2, 1, 5), (0, 4)), ((2, 2, 9, 6), (3, 2, 5, 1), (4, 0)),
          ((4, 3, 5, 6), (7, 3, 5, 6), (0, 0)), ((2, 2, 3, 3), (3, 2, 5, 5), (4, 4)), ((2, 5, 34, 67), (33, 5, 3, 3), (2, 0)),
          ((1, 64, 14, 14), (64, 64, 3, 3), (0, 0))]


def _torch_all(x, w, dy, ph, pw):
    tx, tw = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    y = torch.nn.functional.conv2d(tx, tw, padding=(ph, pw))
    y.backward(torch.tensor(dy))
    return y.detach().numpy(), tw.grad.numpy(), tx.grad.numpy()


@pytest.mark.parametrize("xs,ws,pad", SHAPES)
def test_the_evaluator_equals_torch_bit_for_bit_on_the_exact_family(xs, ws, pad):
    ph, pw = pad
    g = D.Geo(ph, pw)
    x, w, dy = D.exact(np.random.default_rng(xs[3] + ws[0]), xs, ws, g)
    ix, iw, idy = D.as_int(x), D.as_int(w), D.as_int(dy)
    want = (D.forward(ix, iw, g), D.grad_w(ix, idy, ws[2], ws[3], g), D.grad_x(idy, iw, xs[2], xs[3], g))
    assert want[0].dtype == np.int64 and want[0].shape == (xs[0], ws[0]) + D.out_hw(xs[2], xs[3], ws[2], ws[3], g)
    for got, ref in zip(_torch_all(x, w, dy, ph, pw), want):
        assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32))
    for got, ref in zip((D.forward(x, w, g), D.grad_w(x, dy, ws[2], ws[3], g), D.grad_x(dy, w, xs[2], xs[3], g)), want):
        assert got.dtype == np.float64 and np.array_equal(got, ref)             # the float64 path is the same evaluator


@pytest.mark.parametrize("xs,ws,pad", SHAPES)
def test_the_data_gradient_is_the_forward_pass_over_dy_with_the_flipped_filters(xs, ws, pad):
    ph, pw = pad
    g = D.Geo(ph, pw)
    _, w, dy = D.exact(np.random.default_rng(xs[2] + ws[1]), xs, ws, g)
    iw, idy = D.as_int(w), D.as_int(dy)
    flipped = D.flipped(iw)
    assert flipped.shape == (ws[1], ws[0], ws[2], ws[3]) and flipped[0, -1, 0, -1] == iw[-1, 0, -1, 0]
    assert np.array_equal(D.forward(idy, flipped, D.Geo(ws[2] - 1 - ph, ws[3] - 1 - pw)), D.grad_x(idy, iw, xs[2], xs[3], g))


def test_stored_zeros_meet_an_inf_tap_as_nan():
    x = np.ones((1, 1, 3, 3), np.float32)
    w = np.ones((1, 1, 2, 2), np.float32)
    w[0, 0, 0, 0] = np.inf
    y = D.forward(x, w, D.Geo(1, 1))
    assert np.array_equal(np.isnan(y[0, 0]), np.array([[1, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]], bool))
    assert np.all(np.isposinf(y[0, 0][1:, 1:]))
    t = torch.nn.functional.conv2d(torch.nn.functional.pad(torch.tensor(x), (1, 1, 1, 1)), torch.tensor(w)).numpy()
    assert np.array_equal(np.isnan(t), np.isnan(y))


@pytest.mark.parametrize("xs,ws", [((2, 5, 34, 67), (33, 5, 3, 3)), ((1, 64, 14, 14), (64, 64, 3, 3)), ((2, 128, 20, 20), (32, 128, 5, 5))])
def test_torch_fp32_lies_inside_the_bound_on_gaussian_data(xs, ws):
    x, w, dy = D.gaussian(xs, ws, seed=xs[2])
    ref = (D.forward(x, w, blas=True), D.grad_w(x, dy, ws[2], ws[3], blas=True), D.grad_x(dy, w, xs[2], xs[3], blas=True))
    ax, aw, ady = np.abs(x), np.abs(w), np.abs(dy)
    absref = (D.forward(ax, aw, blas=True), D.grad_w(ax, ady, ws[2], ws[3], blas=True), D.grad_x(ady, aw, xs[2], xs[3], blas=True))
    for name, got, r, a, K in zip(("y", "dW", "dX"), _torch_all(x, w, dy, 0, 0), ref, absref, D.reductions(xs, ws)):
        ratio = D.worst_ratio(got, r, a)
        print("\n%s * %s %s: torch fp32 at %.2f u sum|a||b|, bound %.0f (K %d)" % (xs, ws, name, ratio, D.gamma(K) / D.U, K), flush=True)
        assert np.all(np.abs(got.astype(np.float64) - r) <= D.gamma(K) * a), name
        assert 0 < ratio < 0.25 * D.gamma(K) / D.U                              # far inside: the bound has room, and torch does round
