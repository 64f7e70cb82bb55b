"""What the convolution-layer tests compare with (no test here): the reference evaluator and the exact family.

x (N, C, H, W), w (F, C, kh, kw), y and dy (N, F, oh, ow); cross-correlation with a window stride (sh, sw), a tap dilation
(dh, dw) and zero padding (ph, pw); keh = dh (kh - 1) + 1, oh = floor((H + 2 ph - keh) / sh) + 1, likewise kew and ow.  g is a
Geo in the C ABI's order, Geo() the unit geometry (stride 1, no padding, dilation 1), geo(stride, padding, dilation) the same
from ints or pairs:

    forward(x, w, g)           y[n,f,i,j]  = sum_{c,p,q} w[f,c,p,q] x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
    grad_w(x, dy, kh, kw, g)   dW[f,c,p,q] = sum_{n,i,j} dy[n,f,i,j] x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
    grad_x(dy, w, H, W, g)     dX[n,c,u,v] = sum_{f,p,q} dy[n,f,i,j] w[f,c,p,q] over u = i.sh+p.dh-ph, v = j.sw+q.dw-pw

each as kh.kw einsums over strided windows of the MATERIALISED padded array (a stored zero under an Inf tap gives NaN; a cell no
window reads is never touched), in float64 for floating operands and int64 for integer ones (blas=True lets einsum use a GEMM,
for float64 alone).  tests/test_dnn_reference_cpu.py (unit stride and dilation) and tests/test_dnn_general_reference_cpu.py hold
them against torch.nn.functional.conv2d and its autograd on the CPU, bit for bit on the exact family.

exact(rng, xs, ws, g)  integer-valued operands with |x|, |w|, |dy| <= 4.  With every reduction length (C.kh.kw, N.oh.ow, F.kh.kw)
    below 2^20 every partial sum in any order is an integer below 2^24, hence exact in fp32: results compare with array_equal.
gamma(K)  the bound of a K-term fp32 inner product in any order, with or without FMA: (K + 1) u / (1 - (K + 1) u), u = 2^-24.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
EXACT_MAX = 4             # |entries| of the exact family
EXACT_REDUCTION = 1 << 20

Geo = namedtuple("Geo", "ph pw sh sw dh dw", defaults=(0, 0, 1, 1, 1, 1))


def geo(stride=1, padding=0, dilation=1):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return Geo(*pair(padding), *pair(stride), *pair(dilation))


def effective(kh, kw, g):
    return g.dh * (kh - 1) + 1, g.dw * (kw - 1) + 1


def out_hw(H, W, kh, kw, g=Geo()):
    keh, kew = effective(kh, kw, g)
    return (H + 2 * g.ph - keh) // g.sh + 1, (W + 2 * g.pw - kew) // g.sw + 1


def _wide(a):
    a = np.asarray(a)
    return a.astype(np.int64) if np.issubdtype(a.dtype, np.integer) else a.astype(np.float64)


def _padded(x, ph, pw):
    return np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))      # stored zeros


def _window(xp, p, q, oh, ow, g):
    """the padded array's cells under tap (p, q) of every output pixel"""
    return xp[:, :, p * g.dh:p * g.dh + (oh - 1) * g.sh + 1:g.sh, q * g.dw:q * g.dw + (ow - 1) * g.sw + 1:g.sw]


def forward(x, w, g=Geo(), blas=False):
    xp, w = _padded(_wide(x), g.ph, g.pw), _wide(w)
    kh, kw = w.shape[2:]
    oh, ow = out_hw(np.shape(x)[2], np.shape(x)[3], kh, kw, g)
    y = np.zeros((xp.shape[0], w.shape[0], oh, ow), xp.dtype)
    for p in range(kh):
        for q in range(kw):
            y += np.einsum("fc,ncij->nfij", w[:, :, p, q], _window(xp, p, q, oh, ow, g), optimize=blas)
    return y


def grad_w(x, dy, kh, kw, g=Geo(), blas=False):
    xp, dy = _padded(_wide(x), g.ph, g.pw), _wide(dy)
    oh, ow = dy.shape[2:]
    dw = np.zeros((dy.shape[1], xp.shape[1], kh, kw), xp.dtype)
    for p in range(kh):
        for q in range(kw):
            dw[:, :, p, q] = np.einsum("nfij,ncij->fc", dy, _window(xp, p, q, oh, ow, g), optimize=blas)
    return dw


def grad_x(dy, w, H, W, g=Geo(), blas=False):
    dy, w = _wide(dy), _wide(w)
    kh, kw = w.shape[2:]
    oh, ow = dy.shape[2:]
    dxp = np.zeros((dy.shape[0], w.shape[1], H + 2 * g.ph, W + 2 * g.pw), dy.dtype)
    for p in range(kh):
        for q in range(kw):
            _window(dxp, p, q, oh, ow, g)[...] += np.einsum("nfij,fc->ncij", dy, w[:, :, p, q], optimize=blas)
    return dxp[:, :, g.ph:g.ph + H, g.pw:g.pw + W]


def flipped(w):
    """w'[c, f, p, q] = w[f, c, kh - 1 - p, kw - 1 - q]: at unit stride dX = forward(dy, w', Geo(keh - 1 - ph, kew - 1 - pw, dh=dh, dw=dw))"""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def reductions(xs, ws, g=Geo()):
    """the three reduction lengths: (forward C.kh.kw, dW N.oh.ow, dX F.kh.kw)"""
    oh, ow = out_hw(xs[2], xs[3], ws[2], ws[3], g)
    return xs[1] * ws[2] * ws[3], xs[0] * oh * ow, ws[0] * ws[2] * ws[3]


def _draw(draw, xs, ws, g):
    oh, ow = out_hw(xs[2], xs[3], ws[2], ws[3], g)
    assert oh >= 1 and ow >= 1
    return draw(xs), draw(ws), draw((xs[0], ws[0], oh, ow))


def exact(rng, xs, ws, g=Geo()):
    """-> x, w, dy as fp32 arrays holding integers in [-EXACT_MAX, EXACT_MAX]: every partial sum is an exact fp32 integer"""
    assert max(reductions(xs, ws, g)) < EXACT_REDUCTION
    return _draw(lambda s: rng.integers(-EXACT_MAX, EXACT_MAX + 1, s).astype(np.float32), xs, ws, g)


def as_int(a):
    return np.asarray(a).astype(np.int64)


def gaussian(xs, ws, g=Geo(), seed=0):
    rng = np.random.default_rng(seed)
    return _draw(lambda s: rng.standard_normal(s).astype(np.float32), xs, ws, g)


def gamma(K):
    return (K + 1) * U / (1 - (K + 1) * U)


def worst_ratio(got, ref64, absref64):
    """max |got - ref| / (u . sum |a||b|): at most gamma(K) / u, about K + 1, for any summation order"""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    return float(np.max(err / (U * np.maximum(absref64, np.finfo(np.float64).tiny))))
