"""What the 2-D correlation tests compare with (no test here): a float64 numpy reference, and two families of inputs
whose results are exact in fp32 in ANY summation order.

ref2d(a, b, mode, boundary, fill, flip) is scipy.signal.correlate2d (flip = 0) / convolve2d (flip = 1) restated with
np.pad (constant / wrap / symmetric) and one shifted-slice product per tap, the 'valid' swap and the reversal of a swapped
correlation included; tests/test_signal_reference_cpu.py holds it against SciPy itself.

exact(rng, shape_a, shape_b)  integer-valued fp32 operands, |a| <= 8, |b| <= 4 (and an integer |fill| <= 8): with
    taps * 32 < 2^24 every partial sum in any order is an integer below 2^24, hence exact, and results compare with
    array_equal.
separable(rng, ah, aw)  a[r][c] = u[r] + v[c] with small integers, for sizes where a dense reference is too slow:
    separable_expected() is two 1-D correlations against the window's row and column sums — a closed form, exact.
"""
import numpy as np

MODES = ("valid", "same", "full")
BOUNDARIES = ("fill", "wrap", "symm")
MODE_FLAG = {"valid": 0, "same": 1, "full": 2}            # signal.h: VALID, SAME, FULL
BOUNDARY_FLAG = {"fill": 0, "symm": 4, "wrap": 8}         # signal.h: PAD, REFLECT, CIRCULAR
_PAD = {"fill": "constant", "wrap": "wrap", "symm": "symmetric"}
U = 2.0 ** -24                                            # unit roundoff of fp32


def covers(sa, sb):
    return sa[0] >= sb[0] and sa[1] >= sb[1]


def out_shape(sa, sb, mode):
    """SciPy's result shape; ValueError when 'valid' has no operand that covers the other."""
    if mode == "full":
        return sa[0] + sb[0] - 1, sa[1] + sb[1] - 1
    if mode == "same":
        return tuple(sa)
    if covers(sa, sb):
        return sa[0] - sb[0] + 1, sa[1] - sb[1] + 1
    if covers(sb, sa):
        return sb[0] - sa[0] + 1, sb[1] - sa[1] + 1
    raise ValueError("For 'valid' mode, one input must be at least as large as the other in every dimension")


def _origin(n, mode, flip):
    """image index under the first footprint cell of output 0 (signal.c:155-157 in footprint coordinates)"""
    if mode == "full":
        return -(n - 1)
    if mode == "same":
        return -(n // 2) if flip else -((n - 1) // 2)
    return 0


def _pad(a, before, after, boundary, fill):
    """np.pad by any width: numpy's 'wrap' / 'symmetric' handle widths beyond the array by repeating the period"""
    widths = ((before[0], after[0]), (before[1], after[1]))
    if boundary == "fill":
        return np.pad(a, widths, mode="constant", constant_values=fill)
    return np.pad(a, widths, mode=_PAD[boundary])


def ref2d(a, b, mode, boundary="fill", fill=0.0, flip=0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    oh, ow = out_shape(a.shape, b.shape, mode)
    swapped = mode == "valid" and not covers(a.shape, b.shape)
    if swapped:
        a, b = b, a
    w = b[::-1, ::-1] if flip else b
    wh, ww = w.shape
    r0, c0 = _origin(wh, mode, flip), _origin(ww, mode, flip)
    before = (-r0, -c0)
    after = (max(0, oh - 1 + r0 + wh - a.shape[0]), max(0, ow - 1 + c0 + ww - a.shape[1]))
    p = _pad(a, before, after, boundary, float(fill))
    out = np.zeros((oh, ow), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(wh):
            for k in range(ww):
                out += w[j, k] * p[j:j + oh, k:k + ow]
    return out[::-1, ::-1] if swapped and not flip else out


def abs_ref2d(a, b, mode, boundary="fill", fill=0.0, flip=0):
    """|a| (*) |b| with |fill|: the elementwise scale of the inner-product error bound"""
    return ref2d(np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64)), mode, boundary, abs(float(fill)), flip)


def gamma(taps):
    """(K + 1) u / (1 - (K + 1) u): the bound for a K-term inner product accumulated from zero in any order, with or without
    FMA (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_K for the products' sum, one more u for
    rounding a and b's product separately)"""
    k = (taps + 1) * U
    return k / (1.0 - k)


def exact(rng, shape_a, shape_b):
    taps = min(shape_a[0] * shape_a[1], shape_b[0] * shape_b[1])
    assert taps * 32 < 2 ** 24, "the exact family needs taps * 32 < 2^24"
    a = rng.integers(-8, 9, size=shape_a).astype(np.float32)
    b = rng.integers(-4, 5, size=shape_b).astype(np.float32)
    return a, b


def separable(rng, ah, aw):
    """(a, u, v) with a[r][c] = u[r] + v[c], |u|, |v| <= 4"""
    u = rng.integers(-4, 5, size=ah).astype(np.float32)
    v = rng.integers(-4, 5, size=aw).astype(np.float32)
    return u[:, None] + v[None, :], u, v


def _extend1(x, before, after, boundary):
    return np.pad(x, (before, after), mode=_PAD[boundary])


def separable_expected(u, v, b, mode, boundary, flip=0):
    """ref2d(u[:, None] + v[None, :], b, mode, boundary, flip=flip) in closed form, for 'wrap' / 'symm' (the extension of a
    separable image is separable) and for 'valid' (no boundary); fp32, exact while |result| < 2^24.
    out[m][n] = sum_j rowsum[j] U[m + r0 + j] + sum_k colsum[k] V[n + c0 + k]"""
    assert boundary in ("wrap", "symm") or mode == "valid"
    b = np.asarray(b, np.float64)
    w = b[::-1, ::-1] if flip else b
    wh, ww = w.shape
    assert covers((len(u), len(v)), w.shape)
    oh, ow = out_shape((len(u), len(v)), w.shape, mode)
    r0, c0 = _origin(wh, mode, flip), _origin(ww, mode, flip)
    pad = "wrap" if boundary == "fill" else boundary            # 'valid': never read
    ue = _extend1(np.asarray(u, np.float64), -r0, max(0, oh - 1 + r0 + wh - len(u)), pad)
    ve = _extend1(np.asarray(v, np.float64), -c0, max(0, ow - 1 + c0 + ww - len(v)), pad)
    rows, cols = w.sum(axis=1), w.sum(axis=0)
    # sum_{j,k} w[j][k] (U[..j] + V[..k]) = sum_j rowsum[j] U[..j] + sum_k colsum[k] V[..k]
    r = sum(rows[j] * ue[j:j + oh] for j in range(wh))
    c = sum(cols[k] * ve[k:k + ow] for k in range(ww))
    return (r[:, None] + c[None, :]).astype(np.float32)
