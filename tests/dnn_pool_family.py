"""The pooling layers' definition as a numpy evaluator, and the exact family of operands (no test in here).

forward(x, k, s, p, mode) -> y, idx and backward(dy, idx, xshape, k, s, p, mode) -> dx follow include/np_hip.h to the letter, with
float32 at every step: the real cells of a window are scanned in row-major order (max: a cell is taken when v > best || v != v;
average: one chain of adds from +0.0f, then one division by float32(divisor)); dx adds the terms of the covering windows with i
ascending, then j ascending, from +0.0f, each average term rounded on its own.  The loops run over the window's taps and are
vectorised over the outputs, which keeps every output's own order: tap (p, q) ascending is the row-major scan, and for a cell
(u, v) the window index i = (u + ph - p) / sh ascends as p descends.

x is (planes, H, W); k, s, p are (rows, columns) pairs; mode is 'max', 'avg' (divisor kh.kw) or 'avg_valid' (the real cells)."""
import numpy as np

MODE = {"max": 0, "avg": 1, "avg_valid": 2}          # np_pool_mode
CODE = {"max": b"m", "avg": b"a", "avg_valid": b"v"}  # the glue's characters


def pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def out_hw(H, W, k, s, p):
    return (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1


def _tap(n_out, s, pad, t, extent):
    """the outputs i in [i0, i1) whose tap t is a real cell, and that cell for i0: r = i.s - pad + t in [0, extent)"""
    i0 = max(0, -((t - pad) // s))                    # ceil((pad - t) / s)
    i1 = min(n_out, (extent - 1 + pad - t) // s + 1)
    return i0, max(i0, i1), i0 * s - pad + t


def _real(n_out, s, pad, k, extent):
    """per output: the first real row and the number of real rows of its window"""
    t = np.arange(n_out) * s - pad
    lo, hi = np.maximum(t, 0), np.minimum(t + k, extent)
    return lo, hi - lo


def divisors(xshape, k, s, p, mode):
    """(oh, ow) float32"""
    _, H, W = xshape
    oh, ow = out_hw(H, W, k, s, p)
    if mode == "avg":
        return np.full((oh, ow), k[0] * k[1], np.float32)
    return (_real(oh, s[0], p[0], k[0], H)[1][:, None] * _real(ow, s[1], p[1], k[1], W)[1][None, :]).astype(np.float32)


def forward(x, k, s, p, mode):
    x = np.asarray(x, np.float32)
    k, s, p = pair(k), pair(s), pair(p)
    planes, H, W = x.shape
    oh, ow = out_hw(H, W, k, s, p)
    if mode == "max":
        acc = np.full((planes, oh, ow), -np.inf, np.float32)
        first = _real(oh, s[0], p[0], k[0], H)[0][:, None] * W + _real(ow, s[1], p[1], k[1], W)[0][None, :]
        idx = np.broadcast_to(first.astype(np.int32), acc.shape).copy()
    else:
        acc = np.zeros((planes, oh, ow), np.float32)
        idx = None
    with np.errstate(invalid="ignore"):
        for a in range(k[0]):
            i0, i1, r0 = _tap(oh, s[0], p[0], a, H)
            for b in range(k[1]):
                j0, j1, c0 = _tap(ow, s[1], p[1], b, W)
                if i1 == i0 or j1 == j0:
                    continue
                v = x[:, r0:r0 + (i1 - i0 - 1) * s[0] + 1:s[0], c0:c0 + (j1 - j0 - 1) * s[1] + 1:s[1]]
                part = acc[:, i0:i1, j0:j1]
                if mode == "max":
                    take = (v > part) | (v != v)
                    at = ((r0 + np.arange(i1 - i0) * s[0])[:, None] * W + (c0 + np.arange(j1 - j0) * s[1])[None, :]).astype(np.int32)
                    idx[:, i0:i1, j0:j1] = np.where(take, at[None], idx[:, i0:i1, j0:j1])
                    acc[:, i0:i1, j0:j1] = np.where(take, v, part)
                else:
                    acc[:, i0:i1, j0:j1] = part + v
        if mode != "max":
            acc = (acc / divisors(x.shape, k, s, p, mode)[None]).astype(np.float32)
    return acc, idx


def backward(dy, idx, xshape, k, s, p, mode):
    dy = np.asarray(dy, np.float32)
    k, s, p = pair(k), pair(s), pair(p)
    planes, H, W = xshape
    oh, ow = out_hw(H, W, k, s, p)
    assert dy.shape == (planes, oh, ow)
    dx = np.zeros((planes, H, W), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        term = dy if mode == "max" else (dy / divisors(xshape, k, s, p, mode)[None]).astype(np.float32)
        for a in range(k[0] - 1, -1, -1):
            i0, i1, r0 = _tap(oh, s[0], p[0], a, H)
            for b in range(k[1] - 1, -1, -1):
                j0, j1, c0 = _tap(ow, s[1], p[1], b, W)
                if i1 == i0 or j1 == j0:
                    continue
                rows, cols = slice(r0, r0 + (i1 - i0 - 1) * s[0] + 1, s[0]), slice(c0, c0 + (j1 - j0 - 1) * s[1] + 1, s[1])
                t = term[:, i0:i1, j0:j1]
                if mode == "max":
                    at = ((r0 + np.arange(i1 - i0) * s[0])[:, None] * W + (c0 + np.arange(j1 - j0) * s[1])[None, :]).astype(np.int32)
                    hit = idx[:, i0:i1, j0:j1] == at[None]
                    dx[:, rows, cols] = np.where(hit, dx[:, rows, cols] + t, dx[:, rows, cols])
                else:
                    dx[:, rows, cols] = dx[:, rows, cols] + t
    return dx


def exact(rng, planes, H, W, k, s, p, ties=6):
    """integer x in [-8, 8] with planted ties (equal maxima, 9, at the first, a middle and the last real cell of `ties` windows per
    plane; neighbouring windows that overlap them see the same value at other positions) and an integer dy in [-8, 8]"""
    k, s, p = pair(k), pair(s), pair(p)
    oh, ow = out_hw(H, W, k, s, p)
    x = rng.integers(-8, 9, (planes, H, W)).astype(np.float32)
    (rlo, rn), (clo, cn) = _real(oh, s[0], p[0], k[0], H), _real(ow, s[1], p[1], k[1], W)
    for pl in range(planes):
        for _ in range(ties):
            i, j = int(rng.integers(oh)), int(rng.integers(ow))
            cells = [(rlo[i], clo[j]), (rlo[i] + rn[i] // 2, clo[j] + cn[j] // 2), (rlo[i] + rn[i] - 1, clo[j] + cn[j] - 1)]
            for u, v in cells:
                x[pl, u, v] = 9.0
    dy = rng.integers(-8, 9, (planes, oh, ow)).astype(np.float32)
    return x, dy


def gaussian(rng, planes, H, W, k, s, p):
    k, s, p = pair(k), pair(s), pair(p)
    oh, ow = out_hw(H, W, k, s, p)
    return rng.standard_normal((planes, H, W)).astype(np.float32), rng.standard_normal((planes, oh, ow)).astype(np.float32)
