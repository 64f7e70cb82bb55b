"""The softmax family (numpy only): inputs whose results are exact, the fp64 evaluator of every formula of np_hip.h's softmax
block, the per-element error bounds an fp32 implementation of those formulas must meet, and the special-value class map.
tests/test_softmax_reference_cpu.py holds all of it to torch's CPU softmax; tests/test_gpu_softmax.py holds the kernels to it.

THE BOUNDS.  Three facts: fast_exp is within 1.2 ulp of exp, relatively 1.2 . 2^-23 = 2.4 u with u = 2^-24; an add, subtract,
multiply or divide has relative error at most u, and logf (1 ulp) absolute error at most 2 u |log|; a sum of n terms in ANY order
has |error| <= (n - 1) u sum|terms| to first order.  m is exact (a maximum rounds nothing).  All inputs are fp32 and exact.

  d^_i = d_i (1 + a), |a| <= u, so e^_i = exp(d_i) exp(a d_i) (1 + 2.4 u'): relative error u |d_i| + 2.4 u.
  s^ has relative error  sum_j y_j (u |d_j| + 2.4 u) + S u  =  u (W + 2.4 + S),  W = sum_j y_j |d_j|, S = the sum's depth.
  The forms that sum all cols terms have S = cols - 1.  The running forms (streaming, strided) add a lane's elements in chunks
  of 8 (at most 8 adds), then the chunks (L = chunks per lane adds), then join the lanes (J adds); a chunk that raises the
  maximum multiplies the sum so far by one fast_exp of the step (2.4 u, plus u |step| for its argument, plus u for the product).
  The steps an element lives through telescope: |x_j - ref_j| + (m - ref_j) = |d_j|, so W is unchanged; it lives through at most
  L + 1 of them.  So S = 8 + L + J + 3.4 (L + 1) there; depth() below returns max(cols - 1, that).
  softmax      y^_i = e^_i / s^ (1 + u):  |y^_i - y_i| <= u y_i (|d_i| + W + S + 5.8) + 2^-149
               = u y_i (|d_i| + W + cols + c) + 2^-149 with c = 4.8 for the forms that sum cols terms (c = S + 5.8 - cols in
               general).  2^-149: e^_i rounded into the subnormals (2^-150, s >= 1) and the quotient rounded there (2^-150).
  log-softmax  log s^ - log s <= u (W + 2.4 + S), logf adds 2 u |log s|, the last subtract u |y_i|:
               |y^_i - y_i| <= u (|d_i| + W + S + 2.4 + 2 |log s| + |y_i|).
  loss, index  the same quantity with the sign turned: the log-softmax bound at the label.
  loss, prob   sum_j t_j l_j, l_j = -logsoftmax_j with its bound B_j; a product u, the sum (cols - 1) u:
               <= sum_j |t_j| B_j + cols u sum_j |t_j l_j|.
  gradient     (p^_i - t_i) scale: |scale| (P_i + 2 u |p_i - t_i|) + 2^-149, P_i the softmax bound.
  softmax backward      T = sum_j |dy_j y_j|; t^ - t <= cols u T (products u, sum cols - 1); dx = y_i (dy_i - t):
               <= u |y_i| (cols T + 2 |dy_i - t|) + cols 2^-149 (products that underflow).
  log-softmax backward  t = sum dy, t^ - t <= (cols - 1) u sum|dy_j|; fast_exp(y_i) 2.4 u, the product u, the subtract u:
               <= exp(y_i) ((cols - 1) u sum|dy_j| + 3.4 u |t|) + u |dx_i| + 2^-149.
Second-order terms: every bound is a product of factors (1 + a u) with a <= 2^12 here (|d| <= 2^10, cols <= 2^20 in the tests that
use them), so the first-order bound is short by at most a factor 1 + 2^12 u < SECOND_ORDER."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
FAST_EXP_U = 2.4            # fast_exp's 1.2 ulp in units of u
SECOND_ORDER = 1.0 + 2.0 ** -10
CHUNK = 8                   # np_softmax.hip kChunk
STREAM_LANES = 1024         # np_softmax.hip kStreamLanes
FORM_SHORT, FORM_WAVE, FORM_BLOCK, FORM_STREAM, FORM_STRIDED = 1, 2, 3, 4, 5
SOFTMAX, LOG_SOFTMAX = 0, 1
XENT_INDEX, XENT_PROB = 0, 1


def depth(cols, form=FORM_SHORT):
    """S: how many roundings an element of the row sum can pass through, in units of u"""
    if form in (FORM_STREAM, FORM_STRIDED):
        lanes = STREAM_LANES if form == FORM_STREAM else 1
        chunks = -(-cols // (CHUNK * lanes))
        join = 6 + 15 if form == FORM_STREAM else 0           # six butterfly steps, then sixteen waves in order
        return max(cols - 1, CHUNK + chunks + join + (FAST_EXP_U + 1.0) * (chunks + 1))
    return cols - 1


# ---- the fp64 evaluator: every formula of the header, along the middle axis of (outer, cols, inner) ----
def stats(x):
    """-> m, d, e, s, y, ls of an (outer, cols, inner) fp32 array, in float64 (m ... with keepdims)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        m = x.max(axis=1, keepdims=True)
        d = x - m
        e = np.exp(d)
        s = e.sum(axis=1, keepdims=True)
        return m, d, e, s, e / s, np.log(s)


def forward(x, mode):
    m, d, e, s, y, ls = stats(x)
    with np.errstate(all="ignore"):
        return y if mode == SOFTMAX else d - ls


def backward(y, dy, mode):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    with np.errstate(all="ignore"):
        if mode == SOFTMAX:
            return y * (dy - (dy * y).sum(axis=1, keepdims=True))
        return dy - np.exp(y) * dy.sum(axis=1, keepdims=True)


def valid_labels(labels, cols):
    labels = np.asarray(labels, np.float64)
    with np.errstate(all="ignore"):
        return (labels >= 0) & (labels < cols) & (np.floor(labels) == labels)


def onehot(labels, cols):
    """(rows, cols) float64; the rows of invalid labels are NaN"""
    ok = valid_labels(labels, cols)
    t = np.zeros((len(labels), cols))
    t[np.flatnonzero(ok), np.asarray(labels)[ok].astype(np.int64)] = 1.0
    t[~ok] = np.nan
    return t


def cross_entropy(logits, target, kind, scale=1.0):
    """-> loss_rows (rows), dlogits (rows, cols) in float64"""
    logits = np.asarray(logits, np.float32)
    rows, cols = logits.shape
    m, d, e, s, y, ls = (a[:, :, 0] for a in stats(logits[:, :, None]))
    t = onehot(target, cols) if kind == XENT_INDEX else np.asarray(target, np.float64)
    with np.errstate(all="ignore"):
        terms = np.where(t != 0, t * (ls - d), 0.0)          # t == 0 is skipped; a NaN target is != 0
        terms[np.isnan(t)] = np.nan
        return terms.sum(axis=1), (y - t) * np.float64(np.float32(scale))


# ---- the bounds ----
def bound_forward(x, mode, form=FORM_SHORT):
    m, d, e, s, y, ls = stats(x)
    cols, S = np.shape(x)[1], depth(np.shape(x)[1], form)
    with np.errstate(all="ignore"):
        W = np.where(y > 0, y * np.abs(d), 0.0).sum(axis=1, keepdims=True)
        if mode == SOFTMAX:
            return np.where(y > 0, SECOND_ORDER * U * y * (np.abs(d) + W + S + 2 * FAST_EXP_U + 1.0), 0.0) + TINY
        return SECOND_ORDER * U * (np.abs(d) + W + S + FAST_EXP_U + 2 * np.abs(ls) + np.abs(d - ls))


def softmax_c(cols, form=FORM_SHORT):
    """the constant of  u y_i (|d_i| + W + cols + c):  4.8 when the form sums cols terms"""
    return depth(cols, form) + 2 * FAST_EXP_U + 1.0 - cols


def bound_backward(y, dy, mode):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    cols = y.shape[1]
    with np.errstate(all="ignore"):
        if mode == SOFTMAX:
            t = (dy * y).sum(axis=1, keepdims=True)
            T = np.abs(dy * y).sum(axis=1, keepdims=True)
            return SECOND_ORDER * U * np.abs(y) * (cols * T + 2 * np.abs(dy - t)) + cols * TINY
        t = dy.sum(axis=1, keepdims=True)
        A = np.abs(dy).sum(axis=1, keepdims=True)
        return SECOND_ORDER * (np.exp(y) * ((cols - 1) * U * A + (FAST_EXP_U + 1.0) * U * np.abs(t)) + U * np.abs(backward(y, dy, mode))) + TINY


def bound_cross_entropy(logits, target, kind, scale=1.0, form=FORM_SHORT):
    """-> the bounds of loss_rows and of dlogits"""
    logits = np.asarray(logits, np.float32)
    rows, cols = logits.shape
    B = bound_forward(logits[:, :, None], LOG_SOFTMAX, form)[:, :, 0]
    P = bound_forward(logits[:, :, None], SOFTMAX, form)[:, :, 0]
    m, d, e, s, y, ls = (a[:, :, 0] for a in stats(logits[:, :, None]))
    t = onehot(target, cols) if kind == XENT_INDEX else np.asarray(target, np.float64)
    with np.errstate(all="ignore"):
        nz = (t != 0) & ~np.isnan(t)
        l = np.where(nz, ls - d, 0.0)
        loss = np.where(nz, np.abs(t) * B, 0.0).sum(axis=1)
        if kind == XENT_PROB:
            loss = loss + SECOND_ORDER * cols * U * np.abs(np.where(nz, t * l, 0.0)).sum(axis=1)
        grad = abs(float(np.float32(scale))) * (P + SECOND_ORDER * 2 * U * np.abs(y - t)) + TINY
    return loss, grad


# ---- the special-value class map ----
def row_class(row):
    """'nan': the whole row comes out NaN (it holds a NaN or a +Inf, or nothing but -Inf); 'ok' otherwise"""
    row = np.asarray(row, np.float64)
    if np.isnan(row).any() or np.isposinf(row).any() or np.isneginf(row).all():
        return "nan"
    return "ok"


def element_class(row, mode):
    """per element: 'nan', 'zero' (+0.0 of a -Inf among finite values, softmax), 'ninf' (the same, log-softmax) or 'finite'"""
    row = np.asarray(row, np.float64)
    if row_class(row) == "nan":
        return ["nan"] * len(row)
    return [("zero" if mode == SOFTMAX else "ninf") if np.isneginf(v) else "finite" for v in row]


def classes_hold(out_row, in_row, mode):
    out_row = np.asarray(out_row)
    for v, c in zip(out_row, element_class(in_row, mode)):
        ok = {"nan": np.isnan(v), "zero": v == 0 and not np.signbit(v), "ninf": np.isneginf(v), "finite": np.isfinite(v)}[c]
        if not ok:
            return False
    return True


SPECIAL_ROWS = {
    "a nan": [0.5, np.nan, -1.0, 2.0, 0.0],
    "a +inf": [0.5, np.inf, -1.0, 2.0, 0.0],
    "all -inf": [-np.inf] * 5,
    "-inf among finite": [0.5, -np.inf, -1.0, -np.inf, 0.0],
    "nan and +inf": [np.inf, np.nan, -np.inf, 2.0, 0.0],
    "two +inf": [np.inf, 1.0, np.inf, 2.0, 0.0],
    "finite": [0.5, 3.0, -1.0, 2.0, 0.0],
}
INVALID_LABELS = [-1.0, 0.5, np.nan, np.inf, -np.inf, 2.0 ** 31, 1e30]      # and cols itself, which depends on the case


def special_matrix(cols, reps=1):
    """every special row padded to `cols` with copies of its last finite-or-not pattern (tiled), `reps` times, fp32 (rows, cols)"""
    rows = []
    for r in SPECIAL_ROWS.values():
        rows.append(np.resize(np.asarray(r, np.float32), cols))
    return np.tile(np.stack(rows), (reps, 1))


# ---- the exact family ----
EXACT_K = (1, 2, 4, 8, 16, 3, 5, 7)
EXACT_K_POW2 = (1, 2, 4, 8, 16)
EXACT_M = (0.0, -3.5, 17.0, 640.0, -1000.0)          # m - 200 is exact for each


def exact_rows(rng, rows, cols, filler="-inf", k_cycle=EXACT_K):
    """-> x (rows, cols) fp32, k (rows), maxima (rows, cols) bool.  Row r holds m at k_r random positions and -Inf (or m - 200)
    elsewhere; k cycles through k_cycle, a k above cols becomes the largest power of two that cols holds."""
    x = np.empty((rows, cols), np.float32)
    ks = np.empty(rows, np.int64)
    at = np.zeros((rows, cols), bool)
    for r in range(rows):
        k = k_cycle[r % len(k_cycle)]
        if k > cols:
            k = 1 << (int(cols).bit_length() - 1)
        m = np.float32(EXACT_M[(r // len(k_cycle)) % len(EXACT_M)])
        x[r] = -np.inf if filler == "-inf" else m - np.float32(200.0)
        pos = rng.choice(cols, k, replace=False)
        x[r, pos] = m
        ks[r], at[r, pos] = k, True
    return x, ks, at


def exact_softmax(ks, at):
    """float32(1) / float32(k) at the maxima, +0.0 elsewhere"""
    return np.where(at, (np.float32(1.0) / ks.astype(np.float32))[:, None], np.float32(0.0)).astype(np.float32)


def exact_log_softmax(x, ks, at):
    """rows with k == 1 only: +0.0 at the maximum, the filler's own d (-Inf, or -200) elsewhere"""
    assert (ks == 1).all()
    m = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return np.where(at, np.float32(0.0), x - m).astype(np.float32)


def exact_backward_softmax(rng, y):
    """small-integer dy for y in {0, 2^-j}: every product and partial sum is exact.  -> dy, dx (fp32)"""
    dy = rng.integers(-4, 5, y.shape).astype(np.float32)
    t = (dy.astype(np.float64) * y).sum(axis=1, keepdims=True)
    return dy, (y.astype(np.float64) * (dy - t)).astype(np.float32)


def exact_backward_log_softmax(rng, y):
    """y in {0, -Inf, -200} (k == 1): exp(y) is 1 or 0 exactly.  -> dy, dx (fp32)"""
    dy = rng.integers(-4, 5, y.shape).astype(np.float32)
    t = dy.astype(np.float64).sum(axis=1, keepdims=True)
    return dy, (dy - np.where(y == 0, 1.0, 0.0) * t).astype(np.float32)


def exact_cross_entropy(x, ks, at, labels, scale):
    """-> loss (rows; NaN where it is not exact: k > 1), dlogits (rows, cols), both fp32.  scale and k are powers of two for the gradient."""
    rows, cols = x.shape
    p = exact_softmax(ks, at)
    t = np.zeros((rows, cols), np.float32)
    t[np.arange(rows), labels] = 1.0
    grad = ((p - t) * np.float32(scale)).astype(np.float32)
    m = x.max(axis=1)
    with np.errstate(invalid="ignore"):
        loss = np.where(ks == 1, np.float32(0.0) - (x[np.arange(rows), labels] - m), np.nan).astype(np.float32)
    return loss + np.float32(0.0), grad


def gaussian(rng, shape, sigma):
    return (sigma * rng.standard_normal(shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def worst(got, want, bound):
    """the largest |got - want| / bound over the elements whose reference is finite; elements whose reference is not finite
    must match it exactly (NaN for NaN, the same infinity).  -> the ratio, or inf on a mismatch"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(want)
    with np.errstate(all="ignore"):
        if not np.all(np.where(fin, np.isfinite(got), (np.isnan(want) & np.isnan(got)) | (want == got))):
            return np.inf
        if not fin.any():
            return 0.0
        return float(np.max(np.abs(got - want)[fin] / bound[fin]))
