"""What the dense-layer tests compare with (no test here): the evaluator of np_linear.hip's stated orders, the exact family, the
restated launch rules, and NaN-framed buffers.

x (M, K), w (N, K), bias (N), y / dy / dz (M, N); act is None, 'relu', 'tanh' or 'sigmoid' (ACT maps it to np_conv_act).

    fma32(a, b, c)             ONE fused multiply-add in fp32: the product of two fp32 is exact in fp64; the fp64 sum is
                               corrected where it would round twice (its error term, by TwoSum, decides a tie)
    chain(A, B)                (R, L) . (L, C): every element ONE fma32 chain from +0.0f over l ascending, continued over the
                               zero-filled tail up to a multiple of STEP (a -0.0 becomes +0.0 there, as on the device)
    forward(x, w, b, act)      act(float32(chain + b)), the activation by tests/dnn_act_family.py (relu exact; tanh and sigmoid
                               through fp64: a reference, the device's bits only on dyadic data)
    pre_activation(x, w, b)    float32(chain + b): the bits the device's activation is applied to
    act_grad                   tests/dnn_act_family.py's
    grad_x(dz, w)              chain(dz, w)
    grad_w(dz, x)              per slice of dw_plan(M, K, N) a chain over the slice's rows, then the slices added in order
    grad_b(dz)                 per slice of act_plan(M, N) four chains of plain adds over rows m0 + g, m0 + g + 4, ..., added as
                               ((s0 + s1) + s2) + s3, then the slices added in order

exact(rng, M, K, N)  integers with |x|, |w|, |dy| <= 4 and every reduction length below 2^20: any order gives the same bits.
bound(L, a, b)       (L + 1) u sum |a||b| per element, the project's inner-product bound; one more u for the bias add.
"""
import numpy as np

from tests import dnn_act_family as A

ACT = A.ACT
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
# np_linear.hip / np_dnn_tile.h; np_debug_linear_bounds reports them in this order
TM_SMALL, TM_MID, TM_LARGE, TN, STEP = 32, 64, 128, 128, 32
WGRAD_MIN_STEPS, WGRAD_TARGET_GROUPS, WGRAD_MAX_SLICES = 8, 512, 256
ACT_COLS, ACT_GROUPS, ACT_MIN_ROWS, ACT_TARGET_GROUPS, ACT_MAX_SLICES = 64, 4, 256, 1024, 256
Y, DX, DW, DZDB = 0, 1, 2, 3          # the products of np_debug_linear_last_path
TILE, LIBRARY = 1, 2                  # the forms
# the dispatcher: product p takes the library form from LIB_MIN_WORK[p] multiply-adds M.K.N up (profiles/dnn/linear_sweep.log)
LIB_MIN_WORK = {Y: 1 << 18, DX: 1 << 18, DW: 1 << 18}
BOUNDS = (TM_SMALL, TM_MID, TM_LARGE, TN, STEP, WGRAD_MIN_STEPS, WGRAD_TARGET_GROUPS, WGRAD_MAX_SLICES,
          ACT_COLS, ACT_GROUPS, ACT_MIN_ROWS, ACT_TARGET_GROUPS, ACT_MAX_SLICES, LIB_MIN_WORK[Y], LIB_MIN_WORK[DX], LIB_MIN_WORK[DW])
EXACT_MAX, EXACT_REDUCTION = 4, 1 << 20


def ceil_div(a, b):
    return -(-a // b)


def pick_tm(rows):
    return TM_SMALL if rows <= TM_SMALL else TM_MID if rows <= TM_MID else TM_LARGE


def dw_plan(M, K, N):
    """-> (TM, steps per slice, S) of dw = dz^T . x, from the extents alone"""
    tm = pick_tm(N)
    tiles = ceil_div(N, tm) * ceil_div(K, TN)
    steps = ceil_div(M, STEP)
    want = max(1, min(steps // WGRAD_MIN_STEPS, ceil_div(WGRAD_TARGET_GROUPS, tiles), WGRAD_MAX_SLICES))
    per = ceil_div(steps, want)
    return tm, per, ceil_div(steps, per)


def act_plan(M, N):
    """-> (rows per slice, S') of the dz / db kernel, from (M, N) alone"""
    want = max(1, min(M // ACT_MIN_ROWS, ceil_div(ACT_TARGET_GROUPS, ceil_div(N, ACT_COLS)), ACT_MAX_SLICES))
    rows = ceil_div(ceil_div(M, want), ACT_GROUPS) * ACT_GROUPS
    return rows, ceil_div(M, rows)


def form_of(product, M, K, N, force=0):
    """the dispatcher restated: the forced form, else the library form from LIB_MIN_WORK[product] multiply-adds up"""
    return force if force else LIBRARY if M * K * N >= LIB_MIN_WORK[product] else TILE


def expected_forward_path(M, K, N, force=0):
    """(form, tm, slices, launches) of y; launches None: the library form's count is np_sgemm's business (at least 2: the transpose and a product)"""
    return (TILE, pick_tm(M), 1, 1) if form_of(Y, M, K, N, force) == TILE else (LIBRARY, 0, 0, None)


def expected_paths(M, K, N, act, dx=True, dw=True, db=True, force=0):
    """what np_debug_linear_last_path reports after a backward call: {product: (form, tm, slices, launches)}, launches None for the
    library form (np_sgemm's count)"""
    none = (0, 0, 0, 0)
    tm_w, _, s_w = dw_plan(M, K, N)
    s_b = act_plan(M, N)[1]
    lib = (LIBRARY, 0, 0, None)
    return {DX: none if not dx else (TILE, pick_tm(M), 1, 1) if form_of(DX, M, K, N, force) == TILE else lib,
            DW: none if not dw else (TILE, tm_w, s_w, 2 if s_w > 1 else 1) if form_of(DW, M, K, N, force) == TILE else lib,
            DZDB: (1, 0, s_b, 2 if db and s_b > 1 else 1) if (act is not None or db) else none}


def path_matches(got, want):
    """a probe record against an expected one; a None launch count stands for 'at least one'"""
    return got[:3] == want[:3] and (got[3] >= 1 if want[3] is None else got[3] == want[3])


def fma32(a, b, c):
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                            # exact: 48 bits
        s = np.asarray(c + p)                                # fresh, contiguous
        t = s - c
        e = (c - (s - t)) + (p - t)                          # TwoSum: s + e is the exact sum where everything is finite
        low = s.view(np.int64) & 0x1FFFFFFF
        tie = (low == 0x10000000) & np.isfinite(s) & np.isfinite(e) & (e != 0)
        s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def chain(Am, Bm):
    Am, Bm = np.asarray(Am, F32), np.asarray(Bm, F32)
    (R, L), C = Am.shape, Bm.shape[1]
    acc = np.zeros((R, C), F32)
    for l in range(L):
        acc = fma32(Am[:, l:l + 1], Bm[l:l + 1, :], acc)
    if L % STEP:
        acc = acc + F32(0.0)                                 # the zero-filled tail: fma(+0, +0, acc)
    return acc


def pre_activation(x, w, b=None):
    v = chain(x, np.asarray(w, F32).T)
    with np.errstate(invalid="ignore", over="ignore"):
        return v if b is None else (v + np.asarray(b, F32)[None, :]).astype(F32)


def forward(x, w, b=None, act=None):
    return A.activate(pre_activation(x, w, b), act)


act_grad = A.act_grad


def grad_x(dz, w):
    return chain(dz, w)


def grad_w(dz, x):
    dz, x = np.asarray(dz, F32), np.asarray(x, F32)
    (M, N), K = dz.shape, x.shape[1]
    _, per, S = dw_plan(M, K, N)
    rows = per * STEP
    out = None
    for s in range(S):
        part = chain(dz[s * rows:(s + 1) * rows].T, x[s * rows:(s + 1) * rows])
        with np.errstate(invalid="ignore", over="ignore"):
            out = part if out is None else (out + part).astype(F32)
    return out


def grad_b(dz):
    dz = np.asarray(dz, F32)
    M, N = dz.shape
    rows, S = act_plan(M, N)
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            m0, m1 = s * rows, min(M, (s + 1) * rows)
            groups = []
            for g in range(ACT_GROUPS):
                acc = np.zeros(N, F32)
                for m in range(m0 + g, m1, ACT_GROUPS):
                    acc = (acc + dz[m]).astype(F32)
                groups.append(acc)
            part = (((groups[0] + groups[1]).astype(F32) + groups[2]).astype(F32) + groups[3]).astype(F32)
            out = part if out is None else (out + part).astype(F32)
    return out


def backward(x, w, y, dy, act=None):
    """-> dz, dx, dw, db in the device's orders"""
    dz = act_grad(y, dy, act)
    return dz, grad_x(dz, w), grad_w(dz, x), grad_b(dz)


def exact(rng, M, K, N):
    """-> x, w, dy, b as fp32 arrays holding small integers: every partial sum in any order is an exact fp32 integer"""
    assert max(M, K, N) * EXACT_MAX * EXACT_MAX < 1 << 24 and max(M, K, N) < EXACT_REDUCTION
    draw = lambda *s: rng.integers(-EXACT_MAX, EXACT_MAX + 1, s).astype(F32)
    return draw(M, K), draw(N, K), draw(M, N), draw(N)


def gaussian(rng, M, K, N):
    draw = lambda *s: rng.standard_normal(s).astype(F32)
    return draw(M, K), draw(N, K), draw(M, N), draw(N)


def dyadic_outputs(rng, M, N, act):
    """y = k / 8 (tanh: |k| <= 7; sigmoid: 1 <= k <= 7) and integer dy: every operation of the backward rule is exact"""
    k = rng.integers(-7, 8, (M, N)) if act == "tanh" else rng.integers(1, 8, (M, N))
    return (k / 8.0).astype(F32), rng.integers(-4, 5, (M, N)).astype(F32)


def bound(L, a_abs, b_abs, extra=0):
    """(L + 1 + extra) u sum |a||b| per element, a_abs (R, L) and b_abs (L, C) in float64"""
    return (L + 1 + extra) * U * (np.asarray(a_abs, F64) @ np.asarray(b_abs, F64))


def worst_ratio(got, ref64, limit):
    err = np.abs(np.asarray(got, F64) - ref64)
    return float(np.max(err / np.maximum(limit, np.finfo(F64).tiny)))


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())


class Frame:
    """The operands and results of one call inside ONE NaN-filled image: each starts `residue` floats after a 16-byte boundary,
    at least four NaNs after the one before.  Results start as NaN (the canary); expect() writes what the call must leave and
    the WHOLE image is then compared, so one float written outside a result fails."""

    def __init__(self):
        self.items, self.size = [], 8

    def place(self, data_or_size, residue=0):
        data = np.full(data_or_size, np.nan, F32) if isinstance(data_or_size, (int, np.integer)) else np.asarray(data_or_size, F32).reshape(-1)
        start = ceil_div(self.size, 4) * 4 + 4 + residue
        self.items.append((start, data))
        self.size = start + data.size + 4
        return len(self.items) - 1

    def image(self):
        img = np.full(ceil_div(self.size, 4) * 4 + 8, np.nan, F32)
        for start, data in self.items:
            img[start:start + data.size] = data
        return img

    def offset(self, i):
        return self.items[i][0]

    def expect(self, img, i, data):
        start, old = self.items[i]
        data = np.asarray(data, F32).reshape(-1)
        assert data.size == old.size
        img[start:start + data.size] = data
