"""What the tests of the convolution layer's bias and activation compare with (no test here): the numpy evaluator.

On top of tests/dnn_general_family.py (x (N, C, H, W), w (F, C, kh, kw), y and dy (N, F, oh, ow), g a Geo):

    forward(x, w, b, act, g)   act(float32(y_plain + b[None, :, None, None])): the bias is ONE fp32 add to the plain result
    act_grad(y, dy, act)       dz = dy . act'(y) through the OUTPUT y, in float32, in the stated operation order:
                               relu     where(y <= 0, +0.0, dy)       a select: a NaN y passes dy
                               tanh     dy * (1 - y*y)
                               sigmoid  dy * ((1 - y) * y)
    grad_b(dz)                 db[f] = sum_{n,i,j} dz, in int64 for integers and float64 otherwise
    backward(x, w, y, dy, act, g)  -> dz, dW, dX, db: the three gradients of the plain layer on dz

act is None, 'relu', 'tanh' or 'sigmoid'; ACT maps it to np_conv_act.  tests/test_dnn_act_reference_cpu.py holds the evaluator
against torch on the CPU, bit for bit on the exact family.
slices(N, F, P) mirrors np_dnn.hip's rule for the number of slices of the bias gradient.
"""
import numpy as np

from tests import dnn_general_family as G

ACT = {None: 0, "relu": 1, "tanh": 2, "sigmoid": 3}            # np_hip.h: np_conv_act
U = G.U
ACT_BLOCK, ACT_MIN_SLICE, ACT_TARGET_GROUPS, ACT_MAX_SLICES = 256, 4096, 2048, 256     # np_dnn.hip: kAct*


def slices(N, F, P):
    """np_conv2d_backward_act's (S, L), from the extents alone"""
    M = N * P
    want = max(1, min(M // ACT_MIN_SLICE, -(-ACT_TARGET_GROUPS // F), ACT_MAX_SLICES))
    L = -(-(-(-M // want)) // ACT_BLOCK) * ACT_BLOCK
    return -(-M // L), L


def activate(v, act):
    """float32 in, float32 out; tanh and sigmoid through float64 (a reference, not the device's bits)"""
    v = np.asarray(v, np.float32)
    if act is None:
        return v
    if act == "relu":
        return np.where(v <= 0, np.float32(0.0), v)                    # NaN <= 0 is False: a NaN stays; -0.0 becomes +0.0
    with np.errstate(over="ignore"):
        if act == "tanh":
            return np.tanh(v.astype(np.float64)).astype(np.float32)
        return (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(np.float32)


def pre_activation(x, w, b, g=G.Geo(), blas=False):
    """float32(y_plain + b): y_plain rounded to fp32 first (exact for the integer family), then one fp32 add"""
    y = np.asarray(G.forward(x, w, g, blas)).astype(np.float32)
    return y if b is None else (y + np.asarray(b, np.float32)[None, :, None, None]).astype(np.float32)


def forward(x, w, b=None, act=None, g=G.Geo(), blas=False):
    return activate(pre_activation(x, w, b, g, blas), act)


def act_grad(y, dy, act):
    y, dy, one = np.asarray(y, np.float32), np.asarray(dy, np.float32), np.float32(1.0)
    if act is None:
        return dy
    if act == "relu":
        return np.where(y <= 0, np.float32(0.0), dy)
    with np.errstate(invalid="ignore", over="ignore"):
        if act == "tanh":
            return (dy * (one - (y * y).astype(np.float32)).astype(np.float32)).astype(np.float32)
        return (dy * ((one - y).astype(np.float32) * y).astype(np.float32)).astype(np.float32)


def grad_b(dz):
    dz = np.asarray(dz)
    wide = np.int64 if np.all(np.isfinite(dz)) and np.array_equal(dz, np.rint(dz)) else np.float64
    return dz.astype(wide).sum(axis=(0, 2, 3))


def backward(x, w, y, dy, act=None, g=G.Geo(), blas=False):
    """-> dz (float32), dW, dX, db of the layer whose forward result is y"""
    dz = act_grad(y, dy, act)
    integer = all(np.all(np.isfinite(a)) and np.array_equal(a, np.rint(a)) for a in (x, w, dz))
    wide =(lambda a: G.as_int(a)) if integer else (lambda a: a)
    dW = G.grad_w(wide(x), wide(dz), w.shape[2], w.shape[3], g, blas)
    dX = G.grad_x(wide(dz), wide(w), x.shape[2], x.shape[3], g, blas)
    return dz, dW, dX, grad_b(dz)


def exact(rng, xs, ws, g=G.Geo()):
    """-> x, w, dy, b: tests/dnn_family.py's exact family and an integer bias in [-4, 4]"""
    x, w, dy = G.exact(rng, xs, ws, g)
    return x, w, dy, rng.integers(-4, 5, ws[0]).astype(np.float32)
