"""What the strided / dilated convolution-layer tests add to the reference evaluator of tests/dnn_family.py (no test here), which
this module re-exports: forward, grad_w, grad_x, reductions, exact and gaussian take a Geo there.

The data gradient as a forward pass (what the device computes): grad_x_as_forward = the unit-stride forward, taps dilated by
(dh, dw), over stuffed(dy, sh, sw) padded by (keh - 1 - ph, kew - 1 - pw) in front and up to H + keh - 1 behind, with the
filters flipped and transposed.  stuffed(a, lh, lw) puts lh - 1 rows and lw - 1 columns of zeros BETWEEN the entries of the last
two axes: a dilated filter is stuffed(w, dh, dw), a strided layer's gradient on the unit grid stuffed(dy, sh, sw).
never_read(H, W, kh, kw, g): the cells of an image that no window reads.
tests/test_dnn_general_reference_cpu.py holds all of it against torch on the CPU.
"""
import numpy as np

from tests import dnn_family as D
from tests.dnn_family import (U, Geo, as_int, effective, exact, flipped, forward, gamma, gaussian, geo, grad_w, grad_x, out_hw,  # noqa: F401
                              reductions, worst_ratio, _window)


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
