"""The families and the evaluator of the attention tests (np_attention.hip); numpy only.

evaluate / evaluate_backward are the definition of include/np_hip.h in numpy: scores from a chain over d, one multiply by scale, the
online (maximum, rescaled sum) over key tiles, one division per output element; backward from the saved statistics.  They run in
float32 or float64, on any key-tile size and in two key orders, and carry the mutations the CPU tier uses to show that the checks
are not vacuous.

The exact family: q_i = (200 / scale) . onehot(g(i)), k_j = onehot(h(j)) or a zero row (a filler key), scale a power of two, v and
dout in {-1, 0, 1}.  A score is 200 at the keys of query i's class and 0 elsewhere, exp(0) = 1 and exp(-200) = +0.0f in fp32, so
every rescaling factor is exactly 1 or 0 and, with class sizes that are powers of two, every quantity of both passes is dyadic:
exact in any summation order, on any tiling.  closed_form() states the result without a loop over tiles.

The Gaussian family is compared against float64 inside the per-element bounds of bounds(), derived here:
  u = 2^-24.  A_i = scale . max_j sum_d |q_id||k_jd| bounds every |s_ij| of row i; nt = the key tiles of the row.
  score           the fmaf chain over D terms and the multiply by scale: |s~ - s| <= (D + 1) u A_i.  The subtraction of the maximum
                  rounds once more, |s - m| <= 2 A_i: 2 u A_i.  Every rescaling step exponentiates a difference of two maxima,
                  rounded once: 2 u A_i per step, at most nt steps.  E_i = (D + 3 + 2 nt) u A_i bounds the error of every exponent.
  exponential     fast_exp is one hardware exp2 (1 ulp) behind a two-fma argument reduction and an exact ldexp: 4 u relative.
  sums            a sum of Sk terms in any order: Sk u relative to the sum of magnitudes; a rescaling step multiplies by a
                  fast_exp: 5 u, at most nt steps; T = Sk + 5 nt + 5 counts these, the exponential and the final rounding.
  o = N / L       numerator and denominator each carry E_i + T u relative to their sums of magnitudes:
                  |o~ - o| <= 1.05 (2 E_i + 2 T u) sum_j p_ij |v_jd|, the factor 1.05 covering the second-order terms (the first-order
                  term is below 1e-2 on every case here).
  p (backward)    fast_exp(s~ - m~) / l~ with the saved statistics: rho_i = 2 E_i + (T + 5) u relative.
  delta           sum_d dout . o~: Delta_i = sum_d |dout_id| bound_o_id + D u sum_d |dout_id||o_id|.
  dp              D u sum_d |dout_id||v_jd| (the inner-product bound the conv tests use).
  ds = p (dp - delta)   eds_ij = p_ij (rho_i |dp_ij - delta_i| + edp_ij + Delta_i + 2 u (|dp_ij| + |delta_i|)).
  dq, dk          scale . (sum eds |k| + (Sk + 1) u sum |ds||k|), and the same over i with q and Sq + 1.
  dv              sum_i (rho_i + Sq u) p_ij |dout_id|.
  each times 1.05.  No constant was fitted to a device's error."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
BOUNDS = (128, 32, 32, 64, 128, 32, 128)      # np_debug_attention_bounds: query rows, key tile, three D classes, wave rows, dk/dv keys
M_HIGH = 200.0


# ---- the dispatcher, restated --------------------------------------------------------------------------------------------------------------------------
def d_class(D, bounds=BOUNDS):
    for c in bounds[2:5]:
        if D <= c:
            return c
    raise ValueError("D above the largest class")


def key_tiles_of(q0, Sq, Sk, causal, bounds=BOUNDS):
    """the key tiles the workgroup of query rows q0 .. q0 + bounds[0] - 1 visits"""
    TQ, TK = bounds[0], bounds[1]
    nkt = -(-Sk // TK)
    if not causal:
        return nkt
    last = min(q0 + TQ, Sq) - 1
    return min(nkt, last // TK + 1)


def key_tiles_last(Sq, Sk, causal, bounds=BOUNDS):
    return key_tiles_of((-(-Sq // bounds[0]) - 1) * bounds[0], Sq, Sk, causal, bounds)


def skipped(Sq, Sk, causal, bounds=BOUNDS):
    nkt = -(-Sk // bounds[1])
    return sum(nkt - key_tiles_of(q0, Sq, Sk, causal, bounds) for q0 in range(0, Sq, bounds[0]))


def launches(backward, grads=(True, True, True)):
    """forward: 1.  backward: delta, dk/dv unless both are absent, dq unless absent; nothing at all when every gradient is absent"""
    if not backward:
        return 1
    dq, dk, dv = grads
    return 0 if not (dq or dk or dv) else 1 + (1 if dk or dv else 0) + (1 if dq else 0)


def probe(Sq, Sk, D, causal, backward=False, grads=(True, True, True), bounds=BOUNDS):
    """what np_debug_attention_last_path reports"""
    return d_class(D, bounds), bounds[0], bounds[1], launches(backward, grads), key_tiles_last(Sq, Sk, causal, bounds), skipped(Sq, Sk, causal, bounds)


def default_scale(D):
    return float(F32(1.0) / np.sqrt(F32(D)))


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------------------------
def _ref(m):
    """the reference of an exponent: m floored at the most negative finite value"""
    lo = np.finfo(m.dtype).min
    return np.where(m > lo, m, lo).astype(m.dtype)


def _scores(q, k, scale, dtype):
    """(BH, Sq, Sk): the chain over d ascending from +0, rounded to dtype after every step, then ONE multiply by scale"""
    s = np.zeros(q.shape[:2] + (k.shape[1],), dtype)
    with np.errstate(all="ignore"):
        for d in range(q.shape[2]):
            s = (s.astype(F64) + q[:, :, None, d].astype(F64) * k[:, None, :, d].astype(F64)).astype(dtype)
        return (s * dtype(scale)).astype(dtype)


def _visible(Sq, Sk, causal, shift=0):
    i, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
    return (j <= i + shift) if causal else np.ones((Sq, Sk), bool)


def evaluate(q, k, v, causal=False, scale=None, dtype=F32, tile=32, reverse=False, mutate=None):
    """-> (o, save_max, save_sum) in dtype.  reverse: the keys of a tile are taken in descending order.  mutate: None, "drop_key"
    (the heaviest key of row 0 is left out), "no_rescale", "scale2", "mask_plus", "mask_minus" """
    BH, Sq, D = q.shape
    Sk = k.shape[1]
    scale = default_scale(D) if scale is None else scale
    q, k, v = (a.astype(dtype) for a in (q, k, v))
    s = _scores(q, k, scale * (2.0 if mutate == "scale2" else 1.0), dtype)
    vis = _visible(Sq, Sk, causal, {"mask_plus": 1, "mask_minus": -1}.get(mutate, 0))
    if mutate == "mask_minus":
        vis[:, 0] = True
    s = np.where(vis[None], s, dtype(-np.inf))
    if mutate == "drop_key":
        s[:, 0, np.argmax(np.where(np.isnan(s[0, 0]), -np.inf, s[0, 0]))] = -np.inf
    m = np.full((BH, Sq), -np.inf, dtype)
    l = np.zeros((BH, Sq), dtype)
    acc = np.zeros((BH, Sq, D), dtype)
    with np.errstate(all="ignore"):
        for j0 in range(0, Sk, tile):
            js = np.arange(j0, min(j0 + tile, Sk))
            js = js[::-1] if reverse else js
            st = s[:, :, js]
            tm = np.full((BH, Sq), -np.inf, dtype)
            for c in range(len(js)):
                tm = np.where(st[:, :, c] > tm, st[:, :, c], tm)
            up = tm > m
            f = np.where(up, np.exp(_ref(m) - _ref(np.where(up, tm, m))), dtype(1)).astype(dtype)
            m = np.where(up, tm, m)
            if mutate != "no_rescale":
                l = (l * f).astype(dtype)
                acc = (acc * f[:, :, None]).astype(dtype)
            e = np.exp(st - _ref(m)[:, :, None]).astype(dtype)
            for c in range(len(js)):
                l = (l + e[:, :, c]).astype(dtype)
                acc = (acc + e[:, :, c, None] * v[:, None, js[c], :]).astype(dtype)
        l = np.where(m == -np.inf, dtype(np.nan), l).astype(dtype)      # nothing but -Inf was seen: fast_exp(-Inf + Inf)
        return (acc / l[:, :, None]).astype(dtype), m, l


def evaluate_backward(q, k, v, o, dout, save_max, save_sum, causal=False, scale=None, dtype=F32, tile=32, reverse=False, mutate=None):
    """-> (dq, dk, dv) in dtype, accumulated over key tiles.  mutate: None, "no_delta", "swap" (dk and dv exchanged), "scale2",
    "mask_plus", "mask_minus" """
    BH, Sq, D = q.shape
    Sk = k.shape[1]
    scale = default_scale(D) if scale is None else scale
    q, k, v, o, dout, m, l = (a.astype(dtype) for a in (q, k, v, o, dout, save_max, save_sum))
    s = _scores(q, k, scale * (2.0 if mutate == "scale2" else 1.0), dtype)
    vis = _visible(Sq, Sk, causal, {"mask_plus": 1, "mask_minus": -1}.get(mutate, 0))
    if mutate == "mask_minus":
        vis[:, 0] = True
    s = np.where(vis[None], s, dtype(-np.inf))
    with np.errstate(all="ignore"):
        p = (np.exp(s - _ref(m)[:, :, None]).astype(dtype) / l[:, :, None]).astype(dtype)
        delta = np.zeros((BH, Sq), dtype)
        for d in range(D):
            delta = (delta + (dout[:, :, d] * o[:, :, d]).astype(dtype)).astype(dtype)
        if mutate == "no_delta":
            delta = np.zeros_like(delta)
        dp = _scores(dout, v, 1.0, dtype)
        ds = (p * (dp - delta[:, :, None]).astype(dtype)).astype(dtype)
        dq = np.zeros_like(q)
        for j0 in range(0, Sk, tile):
            js = np.arange(j0, min(j0 + tile, Sk))
            for j in (js[::-1] if reverse else js):
                dq = (dq + ds[:, :, j, None] * k[:, None, j, :]).astype(dtype)
        dk, dv = np.zeros_like(k), np.zeros_like(v)
        for i0 in range(0, Sq, tile):
            rows = np.arange(i0, min(i0 + tile, Sq))
            for i in (rows[::-1] if reverse else rows):
                dv = (dv + p[:, i, :, None] * dout[:, i, None, :]).astype(dtype)
                dk = (dk + ds[:, i, :, None] * q[:, i, None, :]).astype(dtype)
        dq, dk = (dq * dtype(scale)).astype(dtype), (dk * dtype(scale)).astype(dtype)
    return (dq, dv, dk) if mutate == "swap" else (dq, dk, dv)


def reference64(q, k, v, dout, causal, scale):
    """the materialised computation in float64 -> dict with every quantity the bounds need"""
    q, k, v, dout = (a.astype(F64) for a in (q, k, v, dout))
    Sq, Sk = q.shape[1], k.shape[1]
    s = np.einsum("bid,bjd->bij", q, k) * scale
    s = np.where(_visible(Sq, Sk, causal)[None], s, -np.inf)
    m = s.max(-1)
    e = np.exp(s - m[:, :, None])
    l = e.sum(-1)
    p = e / l[:, :, None]
    o = p @ v
    delta = (dout * o).sum(-1)
    dp = np.einsum("bid,bjd->bij", dout, v)
    ds = p * (dp - delta[:, :, None])
    return {"o": o, "save_max": m, "save_sum": l, "p": p, "delta": delta, "dp": dp, "ds": ds, "dv": np.einsum("bij,bid->bjd", p, dout),
            "dk": np.einsum("bij,bid->bjd", ds, q) * scale, "dq": (ds @ k) * scale}


def bounds(q, k, v, dout, causal, scale, ref=None, key_tile=BOUNDS[1]):
    """the per-element bounds of the module docstring -> dict o, dq, dk, dv (and save_max, save_sum)"""
    r = reference64(q, k, v, dout, causal, scale) if ref is None else ref
    q, k, v, dout = (np.abs(a.astype(F64)) for a in (q, k, v, dout))
    BH, Sq, D = q.shape
    Sk = k.shape[1]
    nt = -(-Sk // key_tile)
    A = scale * np.einsum("bid,bjd->bij", q, k).max(-1)
    E = (D + 3 + 2 * nt) * U * A
    T = Sk + 5 * nt + 5
    p, ds = r["p"], r["ds"]
    bo = 1.05 * (2 * E + 2 * T * U)[:, :, None] * (p @ v)
    rho = 2 * E + (T + 5) * U
    Delta = (dout * bo).sum(-1) + D * U * (dout * np.abs(r["o"])).sum(-1)
    edp = D * U * np.einsum("bid,bjd->bij", dout, v)
    eds = p * (rho[:, :, None] * np.abs(r["dp"] - r["delta"][:, :, None]) + edp + Delta[:, :, None] + 2 * U * (np.abs(r["dp"]) + np.abs(r["delta"])[:, :, None]))
    return {"o": bo, "save_max": (D + 1) * U * A + U * np.abs(r["save_max"]), "save_sum": 1.05 * (E + T * U) * r["save_sum"],
            "dq": 1.05 * scale * (eds @ k + (Sk + 1) * U * (np.abs(ds) @ k)),
            "dk": 1.05 * scale * (np.einsum("bij,bid->bjd", eds, q) + (Sq + 1) * U * np.einsum("bij,bid->bjd", np.abs(ds), q)),
            "dv": 1.05 * np.einsum("bij,bid->bjd", (rho[:, :, None] + Sq * U) * p, dout)}


def worst_fraction(got, ref, bound):
    """max |got - ref| / bound; NaN or Inf anywhere counts as +Inf"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if not np.isfinite(got).all():
        return np.inf
    with np.errstate(all="ignore"):
        frac = np.abs(got - ref) / bound
    return float(np.nanmax(np.where(bound > 0, frac, np.where(got == ref, 0.0, np.inf))))


# ---- Gaussian data ---------------------------------------------------------------------------------------------------------------------------------------
# (BH, Sq, Sk, D, causal, sigma of q): Sq and Sk from {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257} crossed sparsely, both ways
# round; D from {1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128}; sigma 6 gives sharp rows
GAUSSIAN_CASES = (
    (1, 1, 1, 1, False, 1.0), (3, 2, 33, 2, False, 1.0), (1, 31, 2, 3, True, 1.0), (1, 32, 63, 31, False, 6.0),
    (5, 33, 31, 32, True, 1.0), (1, 63, 129, 33, False, 1.0), (3, 64, 64, 63, True, 6.0), (1, 65, 257, 64, False, 1.0),
    (1, 127, 65, 65, True, 1.0), (1, 128, 128, 127, False, 6.0), (3, 129, 127, 128, True, 1.0), (1, 257, 32, 64, False, 6.0),
    (1, 257, 257, 64, True, 6.0), (1, 129, 1, 16, False, 1.0), (1, 1, 129, 128, True, 1.0), (5, 65, 8, 8, False, 1.0),
)


def gaussian(BH, Sq, Sk, D, sigma_q=1.0, seed=0):
    rng = np.random.default_rng(seed * 7919 + BH * 1000003 + Sq * 10007 + Sk * 101 + D)
    g = lambda *s: rng.standard_normal(s).astype(F32)
    return {"q": (g(BH, Sq, D) * F32(sigma_q)).astype(F32), "k": g(BH, Sk, D), "v": g(BH, Sk, D), "dout": g(BH, Sq, D)}


# ---- the exact family ------------------------------------------------------------------------------------------------------------------------------------
def exact_family(BH, Sq, Sk, D, causal=False, sizes=(1, 2, 4, 8, 16), scale=None, layout="permuted", seed=0):
    """-> dict q, k, v, dout, scale, causal and the closed form (o, save_max, save_sum, dq, dk, dv; backward_ok says whether every
    row's support is a power of two, so that the gradients are exact too).
    layout "permuted": the members of class c (sizes[c % len(sizes)] of them, as far as Sk allows) lie at pseudo-random key positions,
    so the maxima straddle key tiles and arrive before and after lower tiles; query i has class i mod (the classes with a member).
    layout "diagonal" (for causal gradients): class c has its first member at key c and, where sizes allows two, a second at
    c + classes, so every row sees one or two members of its class whatever Sq and Sk are."""
    scale = default_scale(D) if scale is None else float(scale)
    assert np.log2(scale) == np.round(np.log2(scale)), "scale must be a power of two"
    rng = np.random.default_rng(seed * 31 + Sq * 1009 + Sk * 13 + D)
    cls_of_key = np.full(Sk, -1)
    if layout == "diagonal":
        nc = min(D, Sq, Sk)
        cls_of_key[:nc] = np.arange(nc)
        if max(sizes) >= 2:
            second = np.arange(nc, min(2 * nc, Sk))
            cls_of_key[second] = second - nc
    else:
        order, at, nc = rng.permutation(Sk), 0, 0
        while nc < D and at + sizes[nc % len(sizes)] <= Sk:
            n = sizes[nc % len(sizes)]
            cls_of_key[order[at:at + n]] = nc
            at, nc = at + n, nc + 1
        if nc == 0:      # Sk smaller than the first size: one class of all the keys there are
            cls_of_key[:], nc = 0, 1
    g = np.arange(Sq) % nc
    q = np.zeros((BH, Sq, D), F32)
    q[:, np.arange(Sq), g] = F32(M_HIGH / scale)
    k = np.zeros((BH, Sk, D), F32)
    member = cls_of_key >= 0
    k[:, np.flatnonzero(member), cls_of_key[member]] = 1.0
    v = rng.integers(-1, 2, (BH, Sk, D)).astype(F32)
    dout = rng.integers(-1, 2, (BH, Sq, D)).astype(F32)
    d = {"q": q, "k": k, "v": v, "dout": dout, "scale": scale, "causal": causal}
    d.update(closed_form(d, g, cls_of_key))
    return d


def closed_form(d, g, cls_of_key):
    q, k, v, dout, scale = (d[n] for n in ("q", "k", "v", "dout", "scale"))
    Sq, Sk = q.shape[1], k.shape[1]
    vis = _visible(Sq, Sk, d["causal"])
    support = (cls_of_key[None, :] == g[:, None]) & vis
    seen = support.any(1)
    support = np.where(seen[:, None], support, vis)      # a row that sees no member of its class: every visible key at score 0
    count = support.sum(1)
    o64 = (support.astype(F64) @ v.astype(F64)) / count[None, :, None]
    o = o64.astype(F32)                                  # ONE rounding of an exact quotient of small integers
    m = np.broadcast_to(np.where(seen, M_HIGH, 0.0).astype(F32), q.shape[:2]).copy()
    l = np.broadcast_to(count.astype(F32), q.shape[:2]).copy()
    ok = bool(((count & (count - 1)) == 0).all() and count.max() <= 16)
    out = {"o": o, "save_max": m, "save_sum": l, "backward_ok": ok, "support": support}
    if ok:
        p = support.astype(F64) / count[:, None]
        do, q64, k64, v64 = dout.astype(F64), q.astype(F64), k.astype(F64), v.astype(F64)
        delta = (do * o64).sum(-1)
        ds = p[None] * (np.einsum("bid,bjd->bij", do, v64) - delta[:, :, None])
        out.update({"dv": np.einsum("ij,bid->bjd", p, do).astype(F32), "dk": (np.einsum("bij,bid->bjd", ds, q64) * scale).astype(F32),
                    "dq": ((ds @ k64) * scale).astype(F32)})
    return out


# the shapes of the exact tests: (BH, Sq, Sk, D, causal, sizes, layout, scale).  D in {4, 16, 64} takes the default scale (a power
# of two); other D take scale = 1.  Sizes {3, 5, 7} and the permuted layout under causal are forward-only.
EXACT_CASES = (
    (1, 1, 1, 4, False, (1,), "permuted", None), (3, 2, 33, 4, False, (1, 2, 4, 8, 16), "permuted", None),
    (1, 33, 31, 16, False, (1, 2, 4, 8), "permuted", None), (5, 65, 129, 64, False, (1, 2, 4, 8, 16), "permuted", None),
    (1, 129, 257, 16, False, (16, 8, 4, 2, 1), "permuted", None), (1, 257, 65, 64, False, (1, 2), "permuted", None),
    (1, 128, 128, 128, False, (1, 2, 4), "permuted", 1.0), (3, 127, 63, 33, False, (2, 1), "permuted", 1.0),
    (1, 64, 64, 3, False, (16, 8, 4), "permuted", 1.0), (1, 63, 257, 31, False, (3, 5, 7, 1), "permuted", 1.0),
    (1, 257, 129, 64, False, (7, 5, 3), "permuted", None),
    (1, 33, 33, 16, True, (1,), "diagonal", None), (3, 129, 129, 64, True, (1, 2), "diagonal", None),
    (1, 257, 64, 4, True, (1, 2), "diagonal", None), (1, 65, 257, 128, True, (1, 2), "diagonal", 1.0),
    (1, 257, 257, 64, True, (1, 2, 4, 8, 16), "permuted", None), (5, 129, 65, 16, True, (3, 5, 7), "permuted", None),
    (1, 2, 129, 1, True, (1,), "diagonal", 1.0), (1, 31, 32, 2, True, (1, 2), "diagonal", 1.0),
)
