"""The reference of the convolution layer's bias and activation (tests/dnn_act_family.py) against torch on the CPU: on the exact
family conv2d(..., bias) then relu, and autograd's dW, dX and db, equal the evaluator bit for bit; relu's NaN and -0.0 rules and
its select in the backward pass are as the header states them; tanh and sigmoid are within 1e-5 relative of float64 (the bound
tests/test_gpu_libm_domain.py uses for this class of function); the slice rule of the bias gradient."""
import numpy as np
import pytest

from tests import dnn_act_family as A
from tests import dnn_general_family as G

torch = pytest.importorskip("torch")

SHAPES = [((1, 1, 1, 1), (1, 1, 1, 1), G.Geo()),
          ((2, 3, 7, 9), (4, 3, 3, 3), G.Geo()),
          ((3, 2, 8, 9), (33, 2, 3, 3), G.geo(2, 1)),
          ((2, 3, 9, 9), (5, 3, 3, 3), G.geo(1, 0, 2)),
          ((2, 2, 6, 12), (3, 2, 2, 3), G.geo((2, 3), (0, 2), (1, 3)))]


@pytest.mark.parametrize("xs,ws,g", SHAPES)
@pytest.mark.parametrize("act", [None, "relu"])
def test_the_evaluator_equals_torch_bit_for_bit_on_the_exact_family(xs, ws, g, act):
    x, w, dy, b = A.exact(np.random.default_rng(xs[3] + ws[0]), xs, ws, g)
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    ty = torch.nn.functional.conv2d(tx, tw, tb, stride=(g.sh, g.sw), padding=(g.ph, g.pw), dilation=(g.dh, g.dw))
    if act == "relu":
        ty = torch.relu(ty)
    ty.backward(torch.tensor(dy))
    y = A.forward(G.as_int(x), G.as_int(w), b, act, g)
    assert y.dtype == np.float32 and np.array_equal(ty.detach().numpy(), y)
    dz, dW, dX, db = A.backward(x, w, y, dy, act, g)
    assert dW.dtype == np.int64 and db.dtype == np.int64 and db.shape == (ws[0],)
    assert np.array_equal(tw.grad.numpy(), dW.astype(np.float32))
    assert np.array_equal(tx.grad.numpy(), dX.astype(np.float32))
    assert np.array_equal(tb.grad.numpy(), db.astype(np.float32))
    if act == "relu" and y.size > 1:
        assert (y == 0).any() and (y > 0).any() and not np.array_equal(dz, dy)


def test_relu_rules_for_nan_and_negative_zero():
    v = np.array([np.nan, -0.0, 0.0, -1.5, 2.5, -np.inf, np.inf], np.float32)
    y = A.activate(v, "relu")
    assert np.isnan(y[0]) and not np.signbit(y[1:4]).any() and np.array_equal(y[1:], np.array([0, 0, 0, 2.5, 0, np.inf], np.float32))
    assert np.array_equal(y[1:], torch.relu(torch.tensor(v)).numpy()[1:]) and np.isnan(torch.relu(torch.tensor(v)).numpy()[0])
    dy = np.array([3.0, np.nan, np.inf, np.nan, 7.0, -np.inf, 1.0], np.float32)
    dz = A.act_grad(y, dy, "relu")                    # y = NaN passes dy; y <= 0 stops everything, NaN and Inf included
    assert np.array_equal(dz, np.array([3.0, 0, 0, 0, 7.0, 0, 1.0], np.float32)) and not np.signbit(dz).any()
    ty = torch.tensor(y, requires_grad=True)          # torch's threshold_backward: the same select
    t = torch.tensor(v, requires_grad=True)
    torch.relu(t).backward(torch.tensor(dy))
    assert np.array_equal(t.grad.numpy(), dz)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_tanh_and_sigmoid_are_within_1e5_of_float64(act):
    v = np.concatenate([np.linspace(-30, 30, 4001), np.random.default_rng(0).standard_normal(4000) * 3]).astype(np.float32)
    got = A.activate(v, act).astype(np.float64)
    ref = np.tanh(v.astype(np.float64)) if act == "tanh" else 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), np.finfo(np.float32).tiny)) <= 1e-5
    fn = torch.tanh if act == "tanh" else torch.sigmoid
    tor = fn(torch.tensor(v)).numpy().astype(np.float64)
    assert np.max(np.abs(tor - ref) / np.maximum(np.abs(ref), np.finfo(np.float32).tiny)) <= 1e-5
    special = A.activate(np.array([-np.inf, np.inf, np.nan], np.float32), act)
    assert np.array_equal(special[:2], np.array([-1, 1] if act == "tanh" else [0, 1], np.float32)) and np.isnan(special[2])


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_the_backward_rules_are_exact_on_dyadic_outputs(act):
    """y = k / 8 and small integer dy: every operation of the rule is exact in fp32, so the rule equals autograd's in float64"""
    rng = np.random.default_rng(3)
    k = rng.integers(-7, 8, (2, 3, 4, 5)) if act == "tanh" else rng.integers(1, 8, (2, 3, 4, 5))
    y, dy = (k / 8.0).astype(np.float32), rng.integers(-4, 5, k.shape).astype(np.float32)
    dz = A.act_grad(y, dy, act)
    y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
    assert np.array_equal(dz.astype(np.float64), dy64 * (1 - y64 * y64) if act == "tanh" else dy64 * ((1 - y64) * y64))
    assert A.grad_b(dz).dtype == np.float64 and np.array_equal(A.grad_b(dz), dz.astype(np.float64).sum(axis=(0, 2, 3)))


def test_the_slice_rule():
    assert A.slices(1, 1, 1) == (1, 256) and A.slices(2, 3, 4095) == (1, 8192) and A.slices(2, 3, 4096) == (2, 4096)
    assert A.slices(8, 1, 1024) == (2, 4096) and A.slices(1, 4096, 8192) == (1, 8192)       # F alone fills the device
    assert A.slices(32, 64, 3136) == (24, 4352) and A.slices(256, 128, 3136) == (16, 50176)
    for N, F, P in ((3, 5, 4097), (1, 1, 1 << 21), (7, 2047, 1000), (5, 1, 49 * 2000)):
        S, L = A.slices(N, F, P)
        assert L % 256 == 0 and (S - 1) * L < N * P <= S * L and 1 <= S <= 256
