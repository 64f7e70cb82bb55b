"""What the strided / dilated convolution-layer tests compare with (no test here): the reference evaluator of the general layer.

x (N, C, H, W), w (F, C, kh, kw), y and dy (N, F, oh, ow); cross-correlation with a window stride (sh, sw), a tap dilation
(dh, dw) and zero padding (ph, pw); keh = dh (kh - 1) + 1, oh = floor((H + 2 ph - keh) / sh) + 1, likewise kew and ow:

    forward(x, w, g)           y[n,f,i,j]  = sum_{c,p,q} w[f,c,p,q] x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
    grad_w(x, dy, kh, kw, g)   dW[f,c,p,q] = sum_{n,i,j} dy[n,f,i,j] x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
    grad_x(dy, w, H, W, g)     dX[n,c,u,v] = sum_{f,p,q} dy[n,f,i,j] w[f,c,p,q] over u = i.sh+p.dh-ph, v = j.sw+q.dw-pw

each as kh.kw einsums over strided windows of the MATERIALISED padded array (a stored zero under an Inf tap gives NaN; a cell no
window reads is never touched), in float64 for floating operands and int64 for integer ones (blas=True lets einsum use a GEMM,
for float64 alone).  g is a Geo in the C ABI's order.
tests/test_dnn_general_reference_cpu.py holds them against torch.nn.functional.conv2d and its autograd on the CPU, bit for bit
on the exact family of tests/dnn_family.py (integers with |.| <= 4, every reduction below 2^20).

The data gradient as a forward pass (what the device computes): grad_x_as_forward = the unit-stride forward, taps dilated by
(dh, dw), over stuffed(dy, sh, sw) padded by (keh - 1 - ph, kew - 1 - pw) in front and up to H + keh - 1 behind, with the
filters flipped and transposed.  stuffed(a, lh, lw) puts lh - 1 rows and lw - 1 columns of zeros BETWEEN the entries of the last
two axes: a dilated filter is stuffed(w, dh, dw), a strided layer's gradient on the unit grid stuffed(dy, sh, sw).
"""
from collections import namedtuple

import numpy as np

from tests import dnn_family as D

Geo = namedtuple("Geo", "ph pw sh sw dh dw", defaults=(0, 0, 1, 1, 1, 1))
U, gamma, as_int, flipped, worst_ratio = D.U, D.gamma, D.as_int, D.flipped, D.worst_ratio


def geo(stride=1, padding=0, dilation=1):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return Geo(*pair(padding), *pair(stride), *pair(dilation))


def effective(kh, kw, g):
    return g.dh * (kh - 1) + 1, g.dw * (kw - 1) + 1


def out_hw(H, W, kh, kw, g):
    keh, kew = effective(kh, kw, g)
    return (H + 2 * g.ph - keh) // g.sh + 1, (W + 2 * g.pw - kew) // g.sw + 1


def _window(xp, p, q, oh, ow, g):
    """the padded array's cells under tap (p, q) of every output pixel"""
    return xp[:, :, p * g.dh:p * g.dh + (oh - 1) * g.sh + 1:g.sh, q * g.dw:q * g.dw + (ow - 1) * g.sw + 1:g.sw]


def forward(x, w, g=Geo(), blas=False):
    xp, w = D._padded(D._wide(x), g.ph, g.pw), D._wide(w)
    kh, kw = w.shape[2:]
    oh, ow = out_hw(x.shape[2], x.shape[3], kh, kw, g)
    y = np.zeros((xp.shape[0], w.shape[0], oh, ow), xp.dtype)
    for p in range(kh):
        for q in range(kw):
            y += np.einsum("fc,ncij->nfij", w[:, :, p, q], _window(xp, p, q, oh, ow, g), optimize=blas)
    return y


def grad_w(x, dy, kh, kw, g=Geo(), blas=False):
    xp, dy = D._padded(D._wide(x), g.ph, g.pw), D._wide(dy)
    oh, ow = dy.shape[2:]
    dw = np.zeros((dy.shape[1], xp.shape[1], kh, kw), xp.dtype)
    for p in range(kh):
        for q in range(kw):
            dw[:, :, p, q] = np.einsum("nfij,ncij->fc", dy, _window(xp, p, q, oh, ow, g), optimize=blas)
    return dw


def grad_x(dy, w, H, W, g=Geo(), blas=False):
    dy, w = D._wide(dy), D._wide(w)
    kh, kw = w.shape[2:]
    oh, ow = dy.shape[2:]
    dxp = np.zeros((dy.shape[0], w.shape[1], H + 2 * g.ph, W + 2 * g.pw), dy.dtype)
    for p in range(kh):
        for q in range(kw):
            _window(dxp, p, q, oh, ow, g)[...] += np.einsum("nfij,fc->ncij", dy, w[:, :, p, q], optimize=blas)
    return dxp[:, :, g.ph:g.ph + H, g.pw:g.pw + W]


def stuffed(a, lh, lw):
    a = np.asarray(a)
    out = np.zeros(a.shape[:-2] + ((a.shape[-2] - 1) * lh + 1, (a.shape[-1] - 1) * lw + 1), a.dtype)
    out[..., ::lh, ::lw] = a
    return out


def grad_x_as_forward(dy, w, H, W, g=Geo()):
    """the input-dilation identity, on materialised arrays"""
    dy, w = D._wide(dy), D._wide(w)
    keh, kew = effective(w.shape[2], w.shape[3], g)
    d = stuffed(dy, g.sh, g.sw)
    lo_h, lo_w = keh - 1 - g.ph, kew - 1 - g.pw
    hi_h, hi_w = H + keh - 1 - lo_h - d.shape[2], W + kew - 1 - lo_w - d.shape[3]
    assert min(lo_h, lo_w, hi_h, hi_w) >= 0
    d = np.pad(d, ((0, 0), (0, 0), (lo_h, hi_h), (lo_w, hi_w)))
    out = forward(d, flipped(w), Geo(dh=g.dh, dw=g.dw))
    assert out.shape[2:] == (H, W)
    return out


def never_read(H, W, kh, kw, g):
    """boolean (H, W): the cells of an image that no window reads"""
    oh, ow = out_hw(H, W, kh, kw, g)
    seen = np.zeros((1, 1, H + 2 * g.ph, W + 2 * g.pw), bool)
    for p in range(kh):
        for q in range(kw):
            _window(seen, p, q, oh, ow, g)[...] = True
    return ~seen[0, 0, g.ph:g.ph + H, g.pw:g.pw + W]


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
    assert max(reductions(xs, ws, g)) < D.EXACT_REDUCTION
    return _draw(lambda s: rng.integers(-D.EXACT_MAX, D.EXACT_MAX + 1, s).astype(np.float32), xs, ws, g)


def gaussian(xs, ws, g=Geo(), seed=0):
    rng = np.random.default_rng(seed)
    return _draw(lambda s: rng.standard_normal(s).astype(np.float32), xs, ws, g)
