"""The definition of layer and group normalization (include/np_hip.h, np_groupnorm.hip) restated step by step in numpy, the data
families the tests use, the guard that says on which rows and parameters Gaussian data may be compared bit for bit, and the
dispatcher of the kernel forms.  No device and no library: test_groupnorm_reference_cpu.py holds this file to torch,
test_gpu_groupnorm.py holds the kernels to it.

Operands are float32 arrays of shape (N, G, D, inner): M = N.G rows of L = D.inner values, P = G.D parameters, element j of row r
using parameter (r mod G).D + j // inner.  Every per-row and per-parameter scalar that the definition rounds from fp64 to fp32 is
returned with its fp64 value (`wide`: a dict of arrays, one entry per row or parameter).  `_sum`, `_margin`, the guard's depth and
its bound formulas are batchnorm_family's, applied per row and per parameter (`guard` restates the formulas on arrays;
test_groupnorm_reference_cpu.py holds it to batchnorm_family.guard record by record)."""
import numpy as np

from tests import batchnorm_family as B

F32, F64 = np.float32, np.float64
U64 = B.U64
U32 = 2.0 ** -24                        # unit roundoff of fp32
ORDERS = B.ORDERS
DEPTH = B.DEPTH
MARGIN_FACTOR = 2.0 ** 10               # a scalar is guarded when its margin is at least this many times its bound
UNGUARDED_CAP = 0.02                    # the share of a case's rows, and of its parameters, that may be unguarded

ROW_SHORT, ROW_WAVE, ROW_GROUP, ROW_SPLIT = 1, 2, 3, 4
PARAM_NONE, PARAM_COLUMNS, PARAM_PLANES = 0, 1, 2
# np_debug_groupnorm_bounds: kShortMaxL, kWaveMaxL, kGroupSmallL, kGroupMaxL, kTargetGroups, kMaxSlices, kSliceMinSteps
BOUNDS = (32, 1024, 4096, 8192, 2048, 1024, 4)


def _ceil_div(a, b):
    return -(-a // b)


# ---- the dispatcher (pick_forms, plan_slices and the launch functions of np_groupnorm.hip) ----
def geometry(N, G, D, inner):
    """-> M, L, P, n (the values of one parameter)"""
    return N * G, D * inner, G * D, N * inner


def pick_row_form(L, bounds=BOUNDS):
    return ROW_SHORT if L <= bounds[0] else ROW_WAVE if L <= bounds[1] else ROW_GROUP if L <= bounds[3] else ROW_SPLIT


def pick_param_form(inner):
    return PARAM_COLUMNS if inner == 1 else PARAM_PLANES


def row_serves(form, L, bounds=BOUNDS):
    return {ROW_SHORT: L <= bounds[0], ROW_WAVE: L <= bounds[1], ROW_GROUP: L <= bounds[3], ROW_SPLIT: True}[form]


def param_serves(form, inner):
    return form == PARAM_PLANES or inner == 1


def _plan(units, per_step, blocks, bounds):
    S = max(1, min(_ceil_div(units, per_step) // bounds[6], bounds[4] // blocks, bounds[5]))
    per = _ceil_div(units, S)
    return _ceil_div(units, per), per


def row_slices(form, N, G, D, inner, bounds=BOUNDS):
    """S of the split form (0 for the others)"""
    M, L, _, _ = geometry(N, G, D, inner)
    return _plan(_ceil_div(L, 4), 256, M, bounds)[0] if form == ROW_SPLIT else 0


def _param_plan(form, N, G, D, inner, bounds):
    _, _, P, n = geometry(N, G, D, inner)
    if form == PARAM_COLUMNS:
        cw = 1
        while cw < 64 and cw < P:
            cw *= 2
        return _plan(N, 256 // cw, _ceil_div(P, cw), bounds) + (256 // cw,)
    return _plan(_ceil_div(n, 4), 256, P, bounds) + (256,)


def param_slices(form, N, G, D, inner, bounds=BOUNDS):
    return 0 if form == PARAM_NONE else _param_plan(form, N, G, D, inner, bounds)[0]


def launches(row_form, param_form):
    return (3 if row_form == ROW_SPLIT else 1) + (0 if param_form == PARAM_NONE else 2)


def row_depth(form, N, G, D, inner, bounds=BOUNDS):
    """the depth of the deepest chain of fp64 additions behind a row's sum in `form`: a lane's chain, the xor butterfly, the waves
    in order, and for the split form the fold (a lane's slices, then 6)"""
    M, L, _, _ = geometry(N, G, D, inner)
    if form == ROW_SHORT:
        return 1 + max(L - 1, 0).bit_length()
    if form == ROW_WAVE:
        return 4 * (1 if L <= 256 else 2 if L <= 512 else 4) + 6
    if form == ROW_GROUP:
        chunks, waves = (2, 4) if L <= bounds[2] // 2 else (4, 4) if L <= bounds[2] else (2, 16)
        return 4 * chunks + 6 + waves - 1
    S, per = _plan(_ceil_div(L, 4), 256, M, bounds)
    return 4 * _ceil_div(per, 256) + 6 + 3 + _ceil_div(S, 64) + 6


def param_depth(form, N, G, D, inner, bounds=BOUNDS):
    """the same for a parameter's sums: a lane's chain, the tree over the row lanes (columns) or the butterfly and the waves
    (planes), and the fold"""
    S, per, lanes = _param_plan(form, N, G, D, inner, bounds)
    fold = _ceil_div(S, 64) + 6
    if form == PARAM_COLUMNS:
        return _ceil_div(per, lanes) + (lanes.bit_length() - 1) + fold
    return 4 * _ceil_div(per, 256) + 6 + 3 + fold


# ---- the evaluator ----
def _sums(v, order):
    """batchnorm_family._sum for every row of the 2-D float64 array v: from +0.0, in one of three orders"""
    v = np.concatenate([np.zeros((v.shape[0], 1), F64), np.ascontiguousarray(v, F64)], axis=1)
    if order == "forward":
        return np.cumsum(v, axis=1)[:, -1]
    if order == "reversed":
        return np.cumsum(v[:, ::-1], axis=1)[:, -1]
    while v.shape[1] > 1:               # pairwise: neighbours, level by level
        if v.shape[1] % 2:
            v = np.concatenate([v, np.zeros((v.shape[0], 1), F64)], axis=1)
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _exact_sums(t):
    """For every row of the 2-D float64 array t: is the sum of its terms exact in EVERY order?  True when every term is a multiple
    of a quantum q (the lowest set bit over the row's terms) and sum |t| < 2^52 q: then every partial sum of every order is a
    multiple of q below 2^53 q, so it is representable and no addition rounds.  Such a sum has the same fp64 bits in the evaluator
    and in every kernel form, and so has every scalar computed from it alone, ties included (the sum of a few floats is a tie of
    the fp32 rounding more often than not, e.g. (a + b) / 2)."""
    t = np.abs(np.asarray(t, F64))
    with np.errstate(all="ignore"):
        mant, exp = np.frexp(t)
        m53 = (mant * 2.0 ** 53).astype(np.int64)
        low = np.where(m53 != 0, (m53 & -m53).astype(F64) * np.exp2(exp.astype(F64) - 53), np.inf)
        q = low.min(axis=1)
        return np.isfinite(t).all(axis=1) & (t.sum(axis=1) < 2.0 ** 52 * q)


def param_index(G, D, inner):
    """(G, L) -> the parameter of element j of a row of group g"""
    return (np.arange(G)[:, None] * D + np.arange(D * inner)[None, :] // inner).astype(np.int64)


def _per_row(a, N, G, D, inner):
    """a (P) parameter array -> (M, L), the value each element uses"""
    return np.tile(np.asarray(a)[param_index(G, D, inner)], (N, 1))


def _by_param(v, N, G, D, inner):
    """(M, L) values -> (P, n): row p holds the values that use parameter p, in memory order"""
    return np.ascontiguousarray(v.reshape(N, G * D, inner).transpose(1, 0, 2)).reshape(G * D, N * inner)


def apply(x, mean, invstd, gamma=None, beta=None):
    """the per-element expression: three separately rounded fp32 steps.  mean, invstd: (N, G)"""
    N, G, D, inner = x.shape
    rows = x.reshape(N * G, D * inner)
    with np.errstate(all="ignore"):
        h = (rows - np.asarray(mean, F32).reshape(-1, 1)) * np.asarray(invstd, F32).reshape(-1, 1)
        if gamma is not None:
            h = h * _per_row(np.asarray(gamma, F32), N, G, D, inner)
        if beta is not None:
            h = h + _per_row(np.asarray(beta, F32), N, G, D, inner)
    assert h.dtype == F32
    return h.reshape(x.shape)


def forward(x, gamma=None, beta=None, eps=1e-5, order="forward"):
    """-> dict: y (N, G, D, inner), save_mean and save_invstd (N, G), and `wide`, the fp64 values behind every rounded scalar of
    every row with what `guard` needs"""
    x = np.asarray(x, F32)
    N, G, D, inner = x.shape
    M, L = N * G, D * inner
    rows = x.reshape(M, L)
    with np.errstate(all="ignore"):
        K = rows[:, 0].astype(F64)
        d = rows.astype(F64) - K[:, None]                  # exact
        s1, s2 = _sums(d, order), _sums(d * d, order)
        m1 = s1 / F64(L)
        mean64 = K + m1
        var64 = s2 / F64(L) - m1 * m1
        inv64 = F64(1.0) / np.sqrt(var64 + F64(eps))
        mean, invstd = mean64.astype(F32).reshape(N, G), inv64.astype(F32).reshape(N, G)
        wide = {"n": L, "K": K, "m1": m1, "mean64": mean64, "var64": var64, "inv64": inv64, "eps": eps,
                "abs1": np.abs(d).sum(axis=1), "abs2": (d * d).sum(axis=1), "exact1": _exact_sums(d)}
    return {"y": apply(x, mean, invstd, gamma, beta), "save_mean": mean, "save_invstd": invstd, "wide": wide}


def backward(x, dy, gamma, save_mean, save_invstd, order="forward"):
    """-> dict: dx, dgamma and dbeta (P), wide (the rows' mb and mg), wide_param (the parameters' sums)"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    N, G, D, inner = x.shape
    M, L, P, n = geometry(N, G, D, inner)
    mean, invstd = np.asarray(save_mean, F32).reshape(M, 1), np.asarray(save_invstd, F32).reshape(M, 1)
    with np.errstate(all="ignore"):
        xh = (x.reshape(M, L) - mean) * invstd
        g = dy.reshape(M, L) if gamma is None else dy.reshape(M, L) * _per_row(np.asarray(gamma, F32), N, G, D, inner)
        assert xh.dtype == F32 and g.dtype == F32
        g64, h64 = g.astype(F64), xh.astype(F64)
        p = g64 * h64                                      # exact: 24 + 24 bits
        s1, s2 = _sums(g64, order), _sums(p, order)
        mb, mg = (s1 / F64(L)).astype(F32).reshape(M, 1), (s2 / F64(L)).astype(F32).reshape(M, 1)
        wide = {"n": L, "s1": s1, "s2": s2, "abs1": np.abs(g64).sum(axis=1), "abs2": np.abs(p).sum(axis=1),
                "exact1": _exact_sums(g64)}
        dx = invstd * ((g - mb) - xh * mg)
        assert dx.dtype == F32
        d64 = _by_param(dy.reshape(M, L).astype(F64), N, G, D, inner)
        q = d64 * _by_param(h64, N, G, D, inner)
        t1, t2 = _sums(d64, order), _sums(q, order)
        wide_param = {"n": n, "s1": t1, "s2": t2, "abs1": np.abs(d64).sum(axis=1), "abs2": np.abs(q).sum(axis=1),
                      "exact1": _exact_sums(d64)}
    return {"dx": dx.reshape(x.shape), "dgamma": t2.astype(F32), "dbeta": t1.astype(F32), "wide": wide, "wide_param": wide_param}


# ---- the guard ----
def _margins(v):
    """batchnorm_family._margin for every entry of v"""
    v = np.asarray(v, F64)
    with np.errstate(all="ignore"):
        f = v.astype(F32)
        lo, hi = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
        return np.minimum(np.abs(v - (lo.astype(F64) + f.astype(F64)) / 2), np.abs(v - (hi.astype(F64) + f.astype(F64)) / 2))


def guard(wide, kind, depth=DEPTH, exact=True):
    """batchnorm_family.guard on a dict of arrays: {name: (margins, bounds)}.  kind: 'forward' (save_mean, save_invstd of the rows),
    'rows' (mb, mg of the backward pass's rows) or 'params' (dbeta, dgamma).  The formulas, and why depth 64 covers the kernels,
    are in batchnorm_family.guard; `row_depth` and `param_depth` above compute the kernels' depth, and
    test_groupnorm_reference_cpu.py asserts that it stays within DEPTH at every shape of the GPU file.
    exact: the bound of a scalar that is computed from the first sum alone (save_mean, mb, dbeta) is 0 where `_exact_sums` has
    shown that no order of the additions rounds at all; exact=False gives batchnorm_family's bounds everywhere."""
    n, u = F64(wide["n"]), U64
    Dp = F64(min(depth, wide["n"]))
    with np.errstate(all="ignore"):
        if kind == "forward":
            m1, var64 = wide["m1"], wide["var64"]
            e1, e2 = Dp * u * wide["abs1"], (Dp + 1) * u * wide["abs2"]
            em = e1 / n + 2 * u * (np.abs(wide["K"]) + np.abs(m1))
            ev = e2 / n + 2 * np.abs(m1) * e1 / n + 4 * u * (wide["abs2"] / n + m1 * m1)
            if exact:
                em = np.where(wide["exact1"], 0.0, em)
            return {"save_mean": (_margins(wide["mean64"]), em),
                    "save_invstd": (_margins(wide["inv64"]), wide["inv64"] * (ev / (2 * (var64 + wide["eps"])) + 3 * u))}
        e1, e2 = Dp * u * wide["abs1"], Dp * u * wide["abs2"]
        zero = wide["exact1"] if exact else np.zeros(e1.shape, bool)
        if kind == "params":
            return {"dbeta": (_margins(wide["s1"]), np.where(zero, 0.0, e1)), "dgamma": (_margins(wide["s2"]), e2)}
        return {"mb": (_margins(wide["s1"] / n), np.where(zero, 0.0, e1 / n + u * np.abs(wide["s1"] / n))),
                "mg": (_margins(wide["s2"] / n), e2 / n + u * np.abs(wide["s2"] / n))}


def guarded(wide, kind):
    """a boolean per row or parameter: every scalar's margin is at least MARGIN_FACTOR times its bound (or its bound is 0, or it
    is not finite: a NaN has no neighbour to round to)"""
    ok = None
    for margin, bound in guard(wide, kind).values():
        with np.errstate(all="ignore"):
            this = (margin >= MARGIN_FACTOR * bound) | ~np.isfinite(margin) | ~np.isfinite(bound)
        ok = this if ok is None else ok & this
    return ok


# ---- per-element bounds, from u = 2^-24 per fp32 operation (first order, every term taken with its absolute value) ----
def y_bound(x, mean, inv, gamma, beta, em, ei):
    """how far the three rounded steps of y, taken with a mean that is off by at most em and an invstd off by at most ei, can lie
    from the exact y(mean, inv).  x (N, G, D, inner); mean, inv, em, ei (M) float64.
      d = x - mean:  ed = em + u (|d| + em).   h = d . inv:  eh = ed (inv + ei) + |d| ei + u (|h| + ed (inv + ei) + |d| ei).
      h . gamma:  eg = |gamma| eh + u (|h gamma| + |gamma| eh).   + beta:  ey = eg + u (|y| + eg)."""
    N, G, D, inner = x.shape
    M, L = N * G, D * inner
    u = U32
    mean, inv, em, ei = (np.asarray(a, F64).reshape(M, 1) for a in (mean, inv, em, ei))
    d = x.reshape(M, L).astype(F64) - mean
    ed = em + u * (np.abs(d) + em)
    h = d * inv
    e = ed * (inv + ei) + np.abs(d) * ei
    e = e + u * (np.abs(h) + e)
    if gamma is not None:
        ga = _per_row(np.asarray(gamma, F64), N, G, D, inner)
        h, e = h * ga, np.abs(ga) * e
        e = e + u * (np.abs(h) + e)
    if beta is not None:
        h = h + _per_row(np.asarray(beta, F64), N, G, D, inner)
        e = e + u * (np.abs(h) + e)
    return e.reshape(x.shape)


def dx_bound(g, xh, inv, mb, mg, eg, exh, emb, emg):
    """the same for dx = inv . ((g - mb) - xh . mg) with g off by eg, xh by exh, mb by emb, mg by emg (inv is an input and exact).
    g, xh, eg, exh (M, L); the rest (M) or scalars.
      t1 = g - mb:  e1 = eg + emb + u (|t1| + eg + emb).   t2 = xh . mg:  e2 = |xh| emg + |mg| exh + exh emg + u (|t2| + ...).
      t3 = t1 - t2:  e3 = e1 + e2 + u (|t3| + e1 + e2).   dx = inv . t3:  e = inv e3 + u (|dx| + inv e3)."""
    u = U32
    col = lambda a: np.asarray(a, F64).reshape(-1, 1) if np.ndim(a) == 1 else np.asarray(a, F64)
    g, xh, inv, mb, mg, eg, exh, emb, emg = (col(a) for a in (g, xh, inv, mb, mg, eg, exh, emb, emg))
    t1 = g - mb
    e1 = eg + emb
    e1 = e1 + u * (np.abs(t1) + e1)
    t2 = xh * mg
    e2 = np.abs(xh) * emg + np.abs(mg) * exh + exh * emg
    e2 = e2 + u * (np.abs(t2) + e2)
    t3 = t1 - t2
    e3 = e1 + e2
    e3 = e3 + u * (np.abs(t3) + e3)
    e = inv * e3
    return e + u * (np.abs(inv * t3) + e)


def unguarded_y_tolerance(x, ref, gamma, beta):
    """for a row whose saved scalars may be one ulp off the evaluator's: both results use a mean within 2 ulp and an invstd within
    2 ulp of a common one, so they differ by at most twice y_bound at those errors"""
    mean, inv = ref["save_mean"].reshape(-1).astype(F64), ref["save_invstd"].reshape(-1).astype(F64)
    return 2 * y_bound(x, mean, inv, gamma, beta, 2 * np.spacing(np.abs(ref["save_mean"].reshape(-1))).astype(F64),
                       2 * np.spacing(np.abs(ref["save_invstd"].reshape(-1))).astype(F64))


def unguarded_dx_tolerance(x, dy, gamma, save_mean, save_invstd, ref):
    """for a row whose mb or mg may be one ulp off the evaluator's: xh and g are the same bits in both (they come from the inputs),
    so only emb and emg act; twice dx_bound at 2 ulp each"""
    N, G, D, inner = x.shape
    M, L = N * G, D * inner
    mean, inv = np.asarray(save_mean, F32).reshape(M, 1), np.asarray(save_invstd, F32).reshape(M, 1)
    with np.errstate(all="ignore"):
        xh = ((x.reshape(M, L) - mean) * inv).astype(F64)
        g = (dy.reshape(M, L) if gamma is None else dy.reshape(M, L) * _per_row(np.asarray(gamma, F32), N, G, D, inner)).astype(F64)
        mb, mg = (ref["wide"]["s1"] / L).astype(F32), (ref["wide"]["s2"] / L).astype(F32)
        tol = 2 * dx_bound(g, xh, inv.astype(F64), mb.astype(F64), mg.astype(F64), 0.0, 0.0, 2 * np.spacing(np.abs(mb)).astype(F64),
                           2 * np.spacing(np.abs(mg)).astype(F64))
    return tol.reshape(x.shape)


# ---- the exact family ----
PATTERNS = B.PATTERNS      # 'pm1': devs (-1, +1), eps = 0;  'm3': devs (-3, 1, 1, 1), eps = s^2


def exact_family(N, G, D, inner, pattern, seed, constant=()):
    """row r: x = m_r + s_r . dev with integer m_r and s_r a power of two, the devs of `pattern` tiled over the row and permuted by
    `seed`.  'pm1': L even, eps = 0: var = s^2, invstd = 1 / s, xh = +-1.  'm3': L a multiple of 4, eps = s^2 (one s for all
    rows): var + eps = 4 s^2, invstd = 1 / (2 s), xh in (-1.5, 0.5).  Rows in `constant` hold m_r alone: xh = 0 and y = beta for
    eps > 0; NaN for eps = 0.  gamma is +-1, +-2 or +-4 and beta a small integer; per row g = p + q . xh + r . w with w orthogonal
    to 1 and to xh and q a multiple of 4, and dy = g / gamma, exactly: sum g = L p and sum g . xh = q . sum xh^2 are multiples of
    L, and every value on the way to y, dx, dgamma and dbeta is a dyadic number of a few bits, so that every sum is exact in any
    order.  -> dict with the operands and the closed form of every output."""
    devs, eps = PATTERNS[pattern]
    M, L, P, n = geometry(N, G, D, inner)
    assert L % len(devs) == 0
    rng = np.random.default_rng(seed)
    s_all = F64(2.0 ** int(rng.integers(-2, 3)))
    eps = F64(eps if eps is not None else s_all * s_all)
    gamma = (rng.choice([1.0, 2.0, 4.0], P) * rng.choice([-1.0, 1.0], P)).astype(F64)
    beta = rng.integers(-4, 5, P).astype(F64)
    ga, be = _per_row(gamma, N, G, D, inner), _per_row(beta, N, G, D, inner)
    x, g, xh, y, dx = (np.zeros((M, L), F64) for _ in range(5))
    mean, invstd = np.empty(M, F64), np.empty(M, F64)
    for r in range(M):
        m = F64(rng.integers(-3, 6))
        s = s_all if pattern == "m3" else F64(2.0 ** int(rng.integers(-2, 3)))
        dev = np.tile(np.array(devs, F64), L // len(devs))[rng.permutation(L)]
        if r in constant:
            dev[:] = 0
        with np.errstate(all="ignore"):
            inv = F64(1.0) / np.sqrt(s * s * (dev * dev).mean() + eps)
            h = dev * s * inv                      # a constant row with eps = 0: 0 . Inf = NaN
        w = np.zeros(L)
        for value in np.unique(dev):               # w: pairs of positions with the same dev
            at = np.flatnonzero(dev == value)
            at = at[:2 * (min(at.size, 64) // 2)]
            w[at[0::2]], w[at[1::2]] = 1 + (at[0::2] % 2), -(1 + (at[0::2] % 2))
        p, q, rr = F64(rng.integers(-2, 4)), F64(4 * rng.integers(-1, 3)), F64(rng.integers(1, 4))
        hz = np.where(np.isfinite(h), h, 0.0)
        x[r], g[r], xh[r] = m + s * dev, p + q * hz + rr * w, h
        mean[r], invstd[r] = m, inv
        with np.errstate(all="ignore"):
            y[r] = h * ga[r] + be[r]
            dx[r] = inv * ((g[r] - p) - h * ((q * (hz * hz).sum() + 0.0) / L))
    dy = g / ga
    with np.errstate(all="ignore"):
        dbeta = _by_param(dy, N, G, D, inner).sum(axis=1) + 0.0
        dgamma = (_by_param(dy, N, G, D, inner) * _by_param(xh, N, G, D, inner)).sum(axis=1) + 0.0
    shape = (N, G, D, inner)
    out = {"x": x, "dy": dy, "y": y, "dx": dx}
    for name, v in out.items():
        assert (np.isnan(v) | (v.astype(F32).astype(F64) == v)).all(), name
    out = {k: v.astype(F32).reshape(shape) for k, v in out.items()}
    out.update(gamma=gamma.astype(F32), beta=beta.astype(F32), eps=float(eps), save_mean=mean.astype(F32).reshape(N, G),
               save_invstd=invstd.astype(F32).reshape(N, G), dgamma=dgamma.astype(F32), dbeta=dbeta.astype(F32))
    return out


# ---- the Gaussian family ----
MEANS, SIGMAS = (1.0, 1e4, 0.0), (1.0, 1e-3)


def gaussian_family(N, G, D, inner, seed, zero_mean=True):
    """row r: mean MEANS[r % 3] (without zero_mean: MEANS[r % 2], never 0), sigma SIGMAS[(r // 3) % 2]; gamma, beta, dy standard
    normal.  A row of mean 0 has a save_mean near 0, whose fp32 spacing is small: it fails the guard with probability about
    2^-12 sqrt(L), so the long-row cases leave it out."""
    rng = np.random.default_rng(seed)
    M, L, P, _ = geometry(N, G, D, inner)
    x = np.empty((M, L), F32)
    for r in range(M):
        x[r] = (MEANS[r % (3 if zero_mean else 2)] + SIGMAS[(r // 3) % 2] * rng.standard_normal(L)).astype(F32)
    shape = (N, G, D, inner)
    return {"x": x.reshape(shape), "dy": rng.standard_normal(shape).astype(F32), "gamma": rng.standard_normal(P).astype(F32),
            "beta": rng.standard_normal(P).astype(F32), "eps": 1e-5}


# ---- the shapes of test_gpu_groupnorm.py ----
def _ln(M, L, seed=100, zero_mean=None):
    return (M, 1, L, 1, seed, L <= 64 if zero_mean is None else zero_mean)


# layer normalization, (N, G, D, inner, seed, zero_mean): every L of the issue's list and each form boundary +- 1, the M list, the
# rows a short-rows wave holds (64 / W) +- 1, one split case with S = 2 and the largest S under 2 . 10^5 elements
LAYER_CASES = tuple(
    [_ln(5, L) for L in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)]
    + [_ln(3, L) for L in (2047, 2048, 2049, 4095, 4096, 4097)] + [_ln(2, L) for L in (8191, 8192, 8193)]
    + [_ln(M, 7) for M in (1, 2, 3, 7, 8, 9, 63, 64, 65, 257)] + [_ln(M, 1) for M in (63, 64, 65)] + [_ln(M, 16) for M in (3, 4, 5)]
    + [_ln(M, 100) for M in (1, 3, 4, 5, 257)] + [_ln(65, 1100), _ln(1, 8200), _ln(3, 9000), _ln(1, 200000)])

# group normalization, (N, C, inner, G)
def _divisors(C):
    return [g for g in range(1, C + 1) if C % g == 0]


GROUP_SHAPES = tuple(
    [(2, C, inner, g) for C in (1, 2, 3, 6) for inner in (1, 2, 3, 4, 5, 49, 64) for g in _divisors(C)]
    + [(N, 6, 3, g) for N in (1, 5) for g in (1, 2, 3, 6)] + [(2, 64, inner, g) for inner in (1, 5) for g in _divisors(64)]
    + [(1, 6, 1025, g) for g in (1, 3, 6)] + [(2, 3, 1025, 1), (5, 64, 49, 32), (2, 64, 64, 4)]
    # a row that spans several parameters inside one 16-byte access: inner = 1, 2 with L % 4 == 0
    + [(2, 8, 1, 2), (3, 8, 2, 2), (2, 12, 1, 3)]
    # the parameter reduction's slices: columns with S = 1 and S > 1, planes with S = 1 and S > 1
    + [(5, 3, 1, 1), (1100, 3, 1, 3), (4099, 2, 1, 1), (2, 2, 49, 1), (3, 2, 4099, 2), (9, 2, 1025, 1)])
GROUP_CASES = tuple((N, g, C // g, inner, 100, C // g * inner <= 64) for (N, C, inner, g) in GROUP_SHAPES)

# a failing seed is replaced here (test_groupnorm_reference_cpu.py checks every case): (N, G, D, inner) -> seed
SEEDS = {(65, 1, 1100, 1): 101, (2, 1, 2, 49): 101, (2, 2, 3, 64): 101, (1, 3, 2, 1025): 101}
GAUSSIAN_CASES = tuple(dict.fromkeys((c[0], c[1], c[2], c[3], SEEDS.get(c[:4], c[4]), c[5]) for c in LAYER_CASES + GROUP_CASES))
# the shapes of the identity, special-value and surface tests: (N, G, D, inner, seed, zero_mean)
OTHER_CASES = {"identities": ((5, 1, 50, 1, 100, False), (5, 3, 2, 49, 100, False), (5, 1, 1500, 1, 100, False), (5, 1, 9001, 1, 100, False)),
               "special": ((4, 1, 20, 1, 100, False), (3, 2, 3, 50, 100, False), (3, 1, 2500, 1, 100, False), (3, 1, 8500, 1, 100, False)),
               "surface": ((6, 1, 35, 1, 100, False), (4, 3, 2, 15, 100, False)),
               "large_mean": ((12, 1, 63, 1, 100, False), (12, 1, 1500, 1, 100, False), (12, 1, 9001, 1, 105, False)),
               "one_group": ((5, 1, 7, 1, 100, False), (9, 1, 64, 1, 100, False), (3, 1, 300, 1, 100, False), (2, 1, 5000, 1, 100, False),
                             (2, 1, 9000, 1, 100, False))}
