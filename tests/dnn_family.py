"""What the convolution-layer tests compare with (no test here): the reference evaluator and the exact family.

x (N, C, H, W), w (F, C, kh, kw), y and dy (N, F, oh, ow); cross-correlation, stride 1, zero padding (ph, pw):

    forward(x, w, ph, pw)        y[n,f,i,j]  = sum_{c,p,q} w[f,c,p,q] x~[n,c,i+p-ph,j+q-pw]
    grad_w(x, dy, kh, kw, ph, pw)  dW[f,c,p,q] = sum_{n,i,j} dy[n,f,i,j] x~[n,c,i+p-ph,j+q-pw]
    grad_x(dy, w, H, W, ph, pw)  dX[n,c,u,v] = sum_{f,p,q} dy[n,f,u-p+ph,v-q+pw] w[f,c,p,q]

each as kh.kw einsums over shifted windows of the MATERIALISED padded array (a stored zero under an Inf tap gives NaN), in
float64 for floating operands and int64 for integer ones.  tests/test_dnn_reference_cpu.py holds them against
torch.nn.functional.conv2d and its autograd on the CPU, bit for bit on the exact family.

exact(rng, xs, ws)  integer-valued operands with |x|, |w|, |dy| <= 4.  With every reduction length (C.kh.kw, N.oh.ow, F.kh.kw)
    below 2^20 every partial sum in any order is an integer below 2^24, hence exact in fp32: results compare with array_equal.
gamma(K)  the bound of a K-term fp32 inner product in any order, with or without FMA: (K + 1) u / (1 - (K + 1) u), u = 2^-24.
"""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
EXACT_MAX = 4             # |entries| of the exact family
EXACT_REDUCTION = 1 << 20


def out_hw(H, W, kh, kw, ph=0, pw=0):
    return H + 2 * ph - kh + 1, W + 2 * pw - kw + 1


def _wide(a):
    a = np.asarray(a)
    return a.astype(np.int64) if np.issubdtype(a.dtype, np.integer) else a.astype(np.float64)


def _padded(x, ph, pw):
    return np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))      # stored zeros


def forward(x, w, ph=0, pw=0, blas=False):
    x, w = _padded(_wide(x), ph, pw), _wide(w)
    kh, kw = w.shape[2:]
    oh, ow = x.shape[2] - kh + 1, x.shape[3] - kw + 1
    y = np.zeros((x.shape[0], w.shape[0], oh, ow), x.dtype)
    for p in range(kh):
        for q in range(kw):
            y += np.einsum("fc,ncij->nfij", w[:, :, p, q], x[:, :, p:p + oh, q:q + ow], optimize=blas)
    return y


def grad_w(x, dy, kh, kw, ph=0, pw=0, blas=False):
    x, dy = _padded(_wide(x), ph, pw), _wide(dy)
    oh, ow = dy.shape[2:]
    dw = np.zeros((dy.shape[1], x.shape[1], kh, kw), x.dtype)
    for p in range(kh):
        for q in range(kw):
            dw[:, :, p, q] = np.einsum("nfij,ncij->fc", dy, x[:, :, p:p + oh, q:q + ow], optimize=blas)
    return dw


def grad_x(dy, w, H, W, ph=0, pw=0, blas=False):
    dy, w = _wide(dy), _wide(w)
    kh, kw = w.shape[2:]
    oh, ow = dy.shape[2:]
    dx = np.zeros((dy.shape[0], w.shape[1], H + 2 * ph, W + 2 * pw), dy.dtype)
    for p in range(kh):
        for q in range(kw):
            dx[:, :, p:p + oh, q:q + ow] += np.einsum("nfij,fc->ncij", dy, w[:, :, p, q], optimize=blas)
    return dx[:, :, ph:ph + H, pw:pw + W]


def flipped(w):
    """w'[c, f, p, q] = w[f, c, kh - 1 - p, kw - 1 - q]: dX = forward(dy, w', kh - 1 - ph, kw - 1 - pw)"""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def reductions(xs, ws, ph=0, pw=0):
    """the three reduction lengths: (forward C.kh.kw, dW N.oh.ow, dX F.kh.kw)"""
    oh, ow = out_hw(xs[2], xs[3], ws[2], ws[3], ph, pw)
    return xs[1] * ws[2] * ws[3], xs[0] * oh * ow, ws[0] * ws[2] * ws[3]


def exact(rng, xs, ws, ph=0, pw=0):
    """-> x, w, dy as fp32 arrays holding integers in [-EXACT_MAX, EXACT_MAX]"""
    assert max(reductions(xs, ws, ph, pw)) < EXACT_REDUCTION
    oh, ow = out_hw(xs[2], xs[3], ws[2], ws[3], ph, pw)
    draw = lambda s: rng.integers(-EXACT_MAX, EXACT_MAX + 1, s).astype(np.float32)
    return draw(xs), draw(ws), draw((xs[0], ws[0], oh, ow))


def as_int(a):
    return np.asarray(a).astype(np.int64)


def gaussian(xs, ws, ph=0, pw=0, seed=0):
    rng = np.random.default_rng(seed)
    oh, ow = out_hw(xs[2], xs[3], ws[2], ws[3], ph, pw)
    draw = lambda s: rng.standard_normal(s).astype(np.float32)
    return draw(xs), draw(ws), draw((xs[0], ws[0], oh, ow))


def gamma(K):
    return (K + 1) * U / (1 - (K + 1) * U)


def worst_ratio(got, ref64, absref64):
    """max |got - ref| / (u . sum |a||b|): at most gamma(K) / u, about K + 1, for any summation order"""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    return float(np.max(err / (U * np.maximum(absref64, np.finfo(np.float64).tiny))))
