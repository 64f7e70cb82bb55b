"""The definition of batch normalization (include/np_hip.h, np_batchnorm.hip) restated step by step in numpy, the data families the
tests use, the guard that makes bit-for-bit comparison of Gaussian data legitimate, and the dispatcher of the kernel forms.
No device and no library: test_batchnorm_reference_cpu.py holds this file to torch, test_gpu_batchnorm.py holds the kernels to it.

Operands are float32 arrays of shape (N, C, inner).  Every per-channel scalar that the definition rounds from fp64 to fp32 is
returned with its fp64 value, so that `guard` can say how far that value is from a rounding boundary and how far any summation
order can move it."""
import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53                      # unit roundoff of fp64

FORM_ONE, FORM_SPLIT, FORM_ROWS, FORM_APPLY = 1, 2, 3, 4
BOUNDS = (4096, 8192, 2048, 1024, 4)  # np_debug_batchnorm_bounds: kOneSmallN, kOneMaxN, kTargetGroups, kMaxSlices, kSliceMinSteps
ORDERS = ("forward", "reversed", "pairwise")


# ---- the dispatcher (pick_form and plan_of of np_batchnorm.hip) ----
def pick_form(N, C, inner, bounds=BOUNDS):
    return FORM_ROWS if inner == 1 else FORM_ONE if N * inner <= bounds[1] else FORM_SPLIT


def serves(form, N, C, inner, bounds=BOUNDS):
    return {FORM_ONE: N * inner <= bounds[1], FORM_SPLIT: True, FORM_ROWS: inner == 1}[form]


def slices(form, N, C, inner, bounds=BOUNDS):
    """S of the split and rows forms (0 for the one-launch form)"""
    if form == FORM_ONE:
        return 0
    ceil_div = lambda a, b: -(-a // b)
    if form == FORM_ROWS:
        cw = 1
        while cw < 64 and cw < C:
            cw *= 2
        units, per_step, blocks = N, 256 // cw, ceil_div(C, cw)
    else:
        units, per_step, blocks = ceil_div(N * inner, 4), 256, C
    S = max(1, min(ceil_div(units, per_step) // bounds[4], bounds[2] // blocks, bounds[3]))
    return ceil_div(units, ceil_div(units, S))


def kernel_depth(form, N, C, inner, bounds=BOUNDS):
    """the depth of the deepest chain of fp64 additions behind a channel's sum in `form`: a lane's chain, the xor butterfly (6), the
    waves in order (ONE: 3 or 15; SPLIT: 3) or the tree over the row lanes (ROWS), and the fold (a lane's slices, then 6)"""
    ceil_div = lambda a, b: -(-a // b)
    n = N * inner
    if form == FORM_ONE:
        lanes, vals = (256, bounds[0] // 256) if n <= bounds[0] else (1024, bounds[1] // 1024)
        return min(vals, ceil_div(n, lanes)) + 6 + (lanes // 64 - 1)
    S = slices(form, N, C, inner, bounds)
    fold = ceil_div(S, 64) + 6
    if form == FORM_ROWS:
        cw = 1
        while cw < 64 and cw < C:
            cw *= 2
        row_lanes = 256 // cw
        return ceil_div(ceil_div(N, S), row_lanes) + (row_lanes.bit_length() - 1) + fold
    return 4 * ceil_div(ceil_div(ceil_div(n, 4), S), 256) + 6 + 3 + fold


def launches(form):
    return 1 if form in (FORM_ONE, FORM_APPLY) else 3


# ---- the evaluator ----
def _sum(v, order):
    """a sum of float64 terms from +0.0 in one of three orders"""
    v = np.concatenate([np.zeros(1, F64), np.ascontiguousarray(v, F64)])
    if order == "forward":
        return F64(np.cumsum(v)[-1])
    if order == "reversed":
        return F64(np.cumsum(v[::-1])[-1])
    while v.size > 1:                  # pairwise: neighbours, level by level
        if v.size % 2:
            v = np.concatenate([v, np.zeros(1, F64)])
        v = v[0::2] + v[1::2]
    return F64(v[0])


def forward(x, gamma=None, beta=None, eps=1e-5, training=True, momentum=0.1, running_mean=None, running_var=None, order="forward"):
    """-> dict: y, and in training save_mean, save_invstd, running_mean, running_var (new arrays, None when not given) and `wide`,
    the fp64 values behind every rounded scalar with what `guard` needs."""
    x = np.asarray(x, F32)
    N, C, inner = x.shape
    n = N * inner
    out = {"wide": []}
    with np.errstate(all="ignore"):
        if training:
            mean, invstd = np.empty(C, F32), np.empty(C, F32)
            rm = None if running_mean is None else np.array(running_mean, F32)
            rv = None if running_var is None else np.array(running_var, F32)
            for c in range(C):
                xc = x[:, c, :].reshape(-1)
                K = F64(xc[0])
                d = xc.astype(F64) - K                       # exact
                s1, s2 = _sum(d, order), _sum(d * d, order)
                m1 = s1 / F64(n)
                mean64 = K + m1
                var64 = s2 / F64(n) - m1 * m1
                inv64 = F64(1.0) / np.sqrt(var64 + F64(eps))
                mean[c], invstd[c] = F32(mean64), F32(inv64)
                wide = {"c": c, "n": n, "K": K, "m1": m1, "mean64": mean64, "var64": var64, "inv64": inv64, "eps": eps,
                        "abs1": F64(np.abs(d).sum()), "abs2": F64((d * d).sum())}
                if rm is not None:
                    wide["rm64"] = (F64(1.0) - F64(momentum)) * F64(rm[c]) + F64(momentum) * mean64
                    rm[c] = F32(wide["rm64"])
                if rv is not None:
                    unbiased = var64 * F64(n) / (F64(n) - F64(1.0))
                    wide["rv64"] = (F64(1.0) - F64(momentum)) * F64(rv[c]) + F64(momentum) * unbiased
                    rv[c] = F32(wide["rv64"])
                wide["momentum"] = momentum
                out["wide"].append(wide)
            out.update(save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv)
        else:
            mean = np.asarray(running_mean, F32)
            invstd = (F64(1.0) / np.sqrt(np.asarray(running_var, F32).astype(F64) + F64(eps))).astype(F32)
        out["y"] = apply(x, mean, invstd, gamma, beta)
    return out


def apply(x, mean, invstd, gamma=None, beta=None):
    """the per-element expression: three separately rounded fp32 steps"""
    with np.errstate(all="ignore"):
        d = x - mean.reshape(1, -1, 1)
        h = d * invstd.reshape(1, -1, 1)
        if gamma is not None:
            h = h * np.asarray(gamma, F32).reshape(1, -1, 1)
        if beta is not None:
            h = h + np.asarray(beta, F32).reshape(1, -1, 1)
    assert h.dtype == F32
    return h


def backward(x, dy, gamma, save_mean, save_invstd, order="forward"):
    """-> dict: dx, dgamma, dbeta, wide"""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    N, C, inner = x.shape
    n = N * inner
    save_mean, save_invstd = np.asarray(save_mean, F32), np.asarray(save_invstd, F32)
    with np.errstate(all="ignore"):
        xh = (x - save_mean.reshape(1, -1, 1)) * save_invstd.reshape(1, -1, 1)
        dgamma, dbeta, mb, mg = (np.empty(C, F32) for _ in range(4))
        wides = []
        for c in range(C):
            g64, h64 = dy[:, c, :].reshape(-1).astype(F64), xh[:, c, :].reshape(-1).astype(F64)
            p = g64 * h64                                    # exact: 24 + 24 bits
            s1, s2 = _sum(g64, order), _sum(p, order)
            dbeta[c], dgamma[c] = F32(s1), F32(s2)
            mb[c], mg[c] = F32(s1 / F64(n)), F32(s2 / F64(n))
            wides.append({"c": c, "n": n, "s1": s1, "s2": s2, "abs1": F64(np.abs(g64).sum()), "abs2": F64(np.abs(p).sum())})
        k = save_invstd if gamma is None else np.asarray(gamma, F32) * save_invstd
        dx = k.reshape(1, -1, 1) * ((dy - mb.reshape(1, -1, 1)) - xh * mg.reshape(1, -1, 1))
    assert dx.dtype == F32
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "wide": wides}


# ---- the guard ----
def _margin(v):
    """the distance of the fp64 value v from the nearest boundary between two fp32 roundings"""
    v = F64(v)
    f = F32(v)
    lo, hi = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
    return min(abs(v - (F64(lo) + F64(f)) / 2), abs(v - (F64(hi) + F64(f)) / 2))


DEPTH = 64


def guard(wide, backward_pass=False, depth=DEPTH):
    """For one channel's `wide` record: {name: (margin, bound)} for every scalar rounded from fp64 to fp32.  margin: the distance
    of the fp64 value from the nearest fp32 rounding boundary.  bound: what any order of the fp64 additions whose tree is at most
    `depth` deep, and the few other fp64 roundings, can move the value: such a sum of terms t_i is within D u sum |t_i| of the exact
    sum, D = min(depth, n), u = 2^-53 (first order).  DEPTH = 64 covers every order the kernels use at the shapes of
    test_gpu_batchnorm.py (at most 2 . 10^5 elements): a lane's chain (16 values in the one-launch form; at most 7 steps of four
    in a split slice, 8 rows in a rows slice, since a slice holds 4 to 7 workgroup steps there), the butterfly (6), the waves
    (15 at most) or the row-lane tree (8), and the fold (16 slices a lane at most, and 6): `kernel_depth` computes it, and
    test_batchnorm_glue_cpu.py asserts from the library's constants that it stays within DEPTH at every shape of the GPU file.  The sequential orders of the evaluator
    are deeper; that they give the same bits is asserted case by case in test_batchnorm_reference_cpu.py.
      S1 = sum d:    e1 = D u sum|d|.      S2 = sum d^2:  e2 = (D + 1) u sum d^2  (each square is rounded once).
      mean64 = K + S1 / n:   e1 / n + 2 u (|K| + |S1 / n|).
      var64 = S2 / n - (S1 / n)^2:   e2 / n + 2 |m1| e1 / n + 4 u (S2 / n + m1^2).  Relative to var64 that is about
             D u (1 + (mean - K)^2 / var): the shifted cancellation factor; it is 1 where K is within a few sigma of the mean.
      invstd = 1 / sqrt(var64 + eps):   inv . (ev / (2 (var64 + eps)) + 3 u).
      running:  momentum . (the statistic's bound, times n / (n - 1) for the variance) + 4 u |value|.
      backward: sum dy: D u sum|dy|;  sum dy . xh: D u sum|dy . xh| (the products are exact);  mb, mg: those / n + u |value|."""
    n, u = F64(wide["n"]), U64
    D = F64(min(depth, wide["n"]))
    out = {}
    if backward_pass:
        e1, e2 = D * u * wide["abs1"], D * u * wide["abs2"]
        out["dbeta"] = (_margin(wide["s1"]), e1)
        out["dgamma"] = (_margin(wide["s2"]), e2)
        out["mb"] = (_margin(wide["s1"] / n), e1 / n + u * abs(wide["s1"] / n))
        out["mg"] = (_margin(wide["s2"] / n), e2 / n + u * abs(wide["s2"] / n))
        return out
    m1, var64 = wide["m1"], wide["var64"]
    e1, e2 = D * u * wide["abs1"], (D + 1) * u * wide["abs2"]
    em = e1 / n + 2 * u * (abs(wide["K"]) + abs(m1))
    ev = e2 / n + 2 * abs(m1) * e1 / n + 4 * u * (wide["abs2"] / n + m1 * m1)
    out["save_mean"] = (_margin(wide["mean64"]), em)
    out["save_invstd"] = (_margin(wide["inv64"]), wide["inv64"] * (ev / (2 * (var64 + wide["eps"])) + 3 * u))
    if "rm64" in wide:
        out["running_mean"] = (_margin(wide["rm64"]), wide["momentum"] * em + 4 * u * abs(wide["rm64"]))
    if "rv64" in wide:
        out["running_var"] = (_margin(wide["rv64"]), wide["momentum"] * ev * n / (n - 1) + 4 * u * abs(wide["rv64"]))
    return out


def guard_ratio(wides, backward_pass=False):
    """the smallest margin / bound over the channels' scalars (inf when every bound is 0)"""
    worst = np.inf
    for w in wides:
        for margin, bound in guard(w, backward_pass).values():
            if bound > 0:
                worst = min(worst, margin / bound)
    return worst


# ---- the exact family ----
PATTERNS = {"pm1": ((-1, 1), 0.0), "m3": ((-3, 1, 1, 1), None)}      # devs, eps (None: s_c^2 per call -> one s for the array)


def exact_family(N, C, inner, pattern, seed, constant=(), scale=None):
    """x = m_c + s_c . dev with integer m_c and s_c a power of two, the devs of `pattern` tiled over the n values of a channel and
    permuted by `seed`.  'pm1': (-1, +1), eps = 0, n even: var = s^2, invstd = 1 / s.  'm3': (-3, 1, 1, 1), eps = s^2 (one s for
    all channels), n a multiple of 4: var + eps = 4 s^2, invstd = 1 / (2 s).  Channels in `constant` hold m_c alone.
    gamma, beta are small integers; dy = p + q . xh + r . w with w orthogonal to 1 and xh, q a multiple of 4: sum dy = n p and
    sum dy . xh = q . sum xh^2 are multiples of n, and every intermediate of y, dx, dgamma, dbeta is exactly representable.
    -> dict with the operands and the closed form of every output (constant channels: y = beta for eps > 0)."""
    devs, eps = PATTERNS[pattern]
    n = N * inner
    assert n % len(devs) == 0
    rng = np.random.default_rng(seed)
    s_all = F64(scale if scale is not None else 2.0 ** int(rng.integers(-2, 3)))
    eps = F64(eps if eps is not None else s_all * s_all)
    x, dy, y, dx = (np.empty((N, C, inner), F32) for _ in range(4))
    gamma, beta = rng.integers(-3, 4, C).astype(F32), rng.integers(-4, 5, C).astype(F32)
    gamma[gamma == 0] = 2
    mean, invstd, dgamma, dbeta, variance = (np.empty(C, F64) for _ in range(5))
    for c in range(C):
        m = F64(rng.integers(-3, 6))
        s = s_all if pattern == "m3" else F64(2.0 ** int(rng.integers(-2, 3)))
        dev = np.tile(np.array(devs, F64), n // len(devs))[rng.permutation(n)]
        if c in constant:
            dev[:] = 0
        xc = m + s * dev
        var = s * s * (dev * dev).mean()
        with np.errstate(all="ignore"):
            inv = F64(1.0) / np.sqrt(var + eps)
        xh = dev * s * inv if c not in constant else np.zeros(n)
        # w: orthogonal to the ones and to xh, from pairs of positions with the same dev
        w = np.zeros(n)
        for value in np.unique(dev):
            at = np.flatnonzero(dev == value)
            at = at[:2 * (min(at.size, 64) // 2)]
            w[at[0::2]], w[at[1::2]] = 1 + (at[0::2] % 2), -(1 + (at[0::2] % 2))
        p, q, r = F64(rng.integers(-2, 4)), F64(4 * rng.integers(-1, 3)), F64(rng.integers(1, 4))
        g = p + q * xh + r * w
        x[:, c, :], dy[:, c, :] = xc.reshape(N, inner), g.reshape(N, inner)
        mean[c], invstd[c], variance[c] = m, inv, var
        sum_gx = q * (xh * xh).sum() + 0.0      # the sums start from +0.0: never -0.0
        dbeta[c], dgamma[c] = n * p, sum_gx
        if np.isfinite(inv):
            y[:, c, :] = (xh * gamma[c] + beta[c]).reshape(N, inner)
            dx[:, c, :] = ((F64(gamma[c]) * inv) * ((g - p) - xh * (sum_gx / n))).reshape(N, inner)
        else:                              # a constant channel with eps = 0: xh = 0 . Inf
            y[:, c, :], dx[:, c, :], dgamma[c] = np.nan, np.nan, np.nan
        assert (x[:, c, :].reshape(-1).astype(F64) == xc).all() and (dy[:, c, :].reshape(-1).astype(F64) == g).all()
    return {"x": x, "dy": dy, "gamma": gamma, "beta": beta, "eps": float(eps), "y": y, "dx": dx, "save_mean": mean.astype(F32),
            "save_invstd": invstd.astype(F32), "var": variance.astype(F32), "dgamma": dgamma.astype(F32), "dbeta": dbeta.astype(F32)}


# ---- the Gaussian family ----
MEANS, SIGMAS = (0.0, 1.0, 1e4), (1.0, 1e-3)


def gaussian_family(N, C, inner, seed):
    """channel c: mean MEANS[c % 3], sigma SIGMAS[(c // 3) % 2]; gamma, beta, dy standard normal"""
    rng = np.random.default_rng(seed)
    x = np.empty((N, C, inner), F32)
    for c in range(C):
        x[:, c, :] = (MEANS[c % 3] + SIGMAS[(c // 3) % 2] * rng.standard_normal((N, inner))).astype(F32)
    return {"x": x, "dy": rng.standard_normal((N, C, inner)).astype(F32), "gamma": rng.standard_normal(C).astype(F32),
            "beta": rng.standard_normal(C).astype(F32), "eps": 1e-5,
            "running_mean": rng.standard_normal(C).astype(F32), "running_var": (0.5 + rng.random(C)).astype(F32)}


# the shapes and seeds test_gpu_batchnorm.py runs on Gaussian data; test_batchnorm_reference_cpu.py checks the guard for each
# (a seed that fails there is replaced there).  (N, C, inner, seed)
GAUSSIAN_CASES = (
    (5, 3, 2, 104), (5, 2, 3, 100), (6, 3, 4, 100), (3, 2, 1024, 102),                                                 # inner 2, 3, 4 (the smallest 16-byte plane), 1024
    (2, 3, 5, 100), (3, 2, 49, 100), (5, 6, 63, 100), (64, 3, 64, 100), (65, 2, 63, 100), (17, 2, 241, 100),      # ONE on 256 lanes, n to 4096 +- 1
    (2, 3, 4096, 100), (1, 2, 8191, 100), (64, 2, 128, 100), (2, 65, 64, 100),                                    # ONE on 1024 lanes, n to 8192; C = 65
    (3, 2, 2731, 101), (9, 2, 1025, 103), (5, 3, 2049, 101), (3, 3, 21845, 101), (64, 3, 1023, 101), (1, 1, 200000, 100),            # SPLIT: S = 2 ... 49
    (2, 1, 1, 101), (64, 64, 1, 103), (65, 63, 1, 100), (36, 65, 1, 164), (1024, 3, 1, 100), (4099, 3, 1, 100), (200000, 1, 1, 100),      # ROWS: S = 1, 2 ... 195
)
# the shapes of the identity, special-value and surface tests, under the same guard
OTHER_CASES = {"identities": ((5, 5, 49, 100), (3, 5, 4099, 100), (65, 5, 1, 102)), "special": ((4, 3, 50, 100), (3, 3, 4099, 100), (130, 3, 1, 100)),
               "surface": ((6, 3, 35, 100), (33, 5, 1, 100))}
