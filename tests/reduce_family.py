"""Inputs on which every correct reduction returns the same bits, whatever its order — the exact family behind
tests/test_reduce_reference_cpu.py (the family against the oracle and against numpy in several orders) and
tests/test_gpu_reduce_exact.py (the device kernels against the family).  Plain numpy, seeded, no device.

A tolerance test of a sum over n elements allows an error larger than one element as soon as n is a few thousand: a kernel
that drops or double-counts the element at a chunk edge passes it.  Here nothing rounds:

  ints      nonzero integers +-1 .. +-amp with sum |x| < 2^24 over every reduced slice: every partial sum in every order is an
            integer below 2^24, which fp32 holds exactly.  A dropped or doubled element moves the sum by at least 1.
  prods     -1 everywhere except k2 <= 60 entries of 2 and kh <= 60 entries of 0.5 per slice: every partial product in every
            order is +-2^e with |e| <= 60.  There is no +1: a dropped or doubled element flips the sign or moves the exponent.
  extremes  a background strictly inside (-1, 1) and per slice one 2.0 and one -2.0 at chosen positions of the axis.
  specials  NaN / Inf planted into a base array of one of the families above.

expected() computes what a reduction must return FROM THE ARRAY ITSELF in integer arithmetic (never from a float sum), and
refuses an array that leaves the exact range.  min / max follow the reference's loop (ndarray.c:752-772, 939-959; the axis forms
:818-839): start from position 0 of the slice, replace on a strict compare — so a NaN in position 0 is the result and a NaN
anywhere else is ignored.
"""
import numpy as np

OPS = ("sum", "prod", "min", "max", "mean")
EXACT_LIMIT = 1 << 24      # fp32 holds every integer up to here
PROD_LIMIT = 60            # 2s and 0.5s per slice: partial products stay inside 2^-60 .. 2^60
LOOP_MAX = 2048            # expected(min / max) walks the reference's loop itself up to this axis length

# kinds of specials(): what a slice was given
FINITE, NAN_FIRST, NAN_LATER, NAN_ALL, INF_ALONE, INF_BOTH, INF_NEXT_TO_NAN = range(7)
SPECIAL_KINDS = (NAN_FIRST, NAN_LATER, NAN_ALL, INF_ALONE, INF_BOTH, INF_NEXT_TO_NAN)


def _slices(x, axis):
    """x as (outer, n, inner); axis None: the flat array as one slice."""
    x = np.asarray(x)
    if axis is None:
        return x.reshape(1, x.size, 1)
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    return x.reshape(outer, x.shape[axis], inner)


def _out_shape(shape, axis):
    return () if axis is None else tuple(shape[:axis]) + tuple(shape[axis + 1:])


def positions(n):
    """Where along an axis of n elements a kernel's seams lie: both ends, and around every 2^j, 3 * 2^j, 1000 * 2^j, 3000 * 2^j."""
    p = set(range(0, 9)) | set(range(n - 9, n))
    for unit in (1, 1000):
        m = unit
        while m <= n:
            for k in (1, 3):
                p.update((k * m - 1, k * m, k * m + 1))
            m *= 2
    return sorted(q for q in p if 0 <= q < n)


def ints(shape, seed, amp, axis=None):
    """Nonzero integers in +-1 .. +-amp as fp32; refuses a shape whose slices along `axis` could reach 2^24."""
    if amp < 1:
        raise ValueError("ints: amp must be at least 1")
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape, dtype=np.int64))
    mag = rng.integers(1, amp + 1, size=size, dtype=np.int8)
    x = np.where(rng.integers(0, 2, size=size, dtype=np.int8) == 1, mag, -mag).astype(np.float32).reshape(shape)
    bound = int(np.abs(_slices(x, axis)).astype(np.int64).sum(axis=1).max()) if size else 0
    if bound >= EXACT_LIMIT:
        raise ValueError("ints: sum |x| = %d over a slice leaves the exact fp32 range (2^24)" % bound)
    return x


def prods(shape, axis, seed):
    """-1 with k2 entries of 2 and kh entries of 0.5 per slice (k2, kh in 0 .. 60, drawn per slice), spread over the axis."""
    rng = np.random.default_rng(seed)
    x = np.full(shape, -1.0, np.float32)
    v = _slices(x, axis)          # a view: x is contiguous
    outer, n, inner = v.shape
    k2 = rng.integers(0, min(PROD_LIMIT, n) + 1, size=(outer, 1, inner))
    kh = rng.integers(0, PROD_LIMIT + 1, size=(outer, 1, inner))
    kh = np.minimum(kh, n - k2)
    # rank of position i in slice (o, j): a bijection of 0 .. n-1 that differs from slice to slice
    mult = next(m for m in (7919, 7907, 104729, 1) if np.gcd(m, n) == 1)
    start = rng.integers(0, n, size=(outer, 1, inner))
    rank = (np.arange(n, dtype=np.int64).reshape(1, n, 1) * mult + start) % n
    v[rank < k2] = 2.0
    v[(rank >= k2) & (rank < k2 + kh)] = 0.5
    return x


def extreme_rounds(shape, axis, pos):
    """How often extremes() has to be called (round = 0, 1, ...) until every position has held a maximum and a minimum."""
    outputs = max(1, int(np.prod(_out_shape(shape, axis), dtype=np.int64)))
    return (len(pos) + outputs - 1) // outputs


def extremes(shape, axis, pos, seed, round=0, background=None):
    """Background in (-1, 1); slice number s holds its only 2.0 at pos[(round * outputs + s) % len] and its only -2.0 half the
    list further on (an axis of one element holds the 2.0 alone).  Returns (array, background) — hand the background back in
    for the next round of the same shape."""
    if background is None:
        rng = np.random.default_rng(seed)
        background = rng.uniform(-0.96875, 0.96875, size=shape).astype(np.float32)
        background[background == 0.0] = 0.5
    x = background.copy()
    v = _slices(x, axis)
    outer, n, inner = v.shape
    pos = np.asarray(pos, dtype=np.int64)
    if pos.size == 0 or pos.min() < 0 or pos.max() >= n:
        raise ValueError("extremes: positions outside the axis")
    s = np.arange(outer * inner, dtype=np.int64)
    at = round * outer * inner + s
    hi = pos[at % pos.size]
    lo = pos[(at + max(1, pos.size // 2)) % pos.size]
    o, j = s // inner, s % inner
    if n > 1:
        lo = np.where(lo == hi, (hi + 1) % n, lo)
        v[o, lo, j] = -2.0
    v[o, hi, j] = 2.0
    return x, background


def specials(base, axis, pos, seed=0, round=0, limit=192):
    """A copy of `base` in which every other slice (the odd ones; the first too when there is only one) holds a special
    pattern, its kinds dealt in turn and its positions from `pos`; the slices between them stay finite.  Of more than `limit`
    such slices only the first, the middle and the last limit / 3 are used.  Returns (array, kinds)."""
    x = np.array(base, dtype=np.float32, copy=True)
    v = _slices(x, axis)
    outer, n, inner = v.shape
    pos = [p for p in pos if 0 <= p < n]
    kinds = np.zeros(outer * inner, dtype=np.int64)
    single = outer * inner == 1
    t = round + seed
    chosen = [0] if single else list(range(1, outer * inner, 2))
    if len(chosen) > limit:
        third, mid = limit // 3, len(chosen) // 2
        chosen = chosen[:third] + chosen[mid - third // 2:mid - third // 2 + third] + chosen[-third:]
    for s in chosen:
        kind = SPECIAL_KINDS[t % len(SPECIAL_KINDS)]
        p = pos[(t // len(SPECIAL_KINDS) + t) % len(pos)]
        t += 1
        o, j = s // inner, s % inner
        if kind == NAN_FIRST:
            v[o, 0, j] = np.nan
        elif kind == NAN_LATER:
            if n == 1:
                kind = FINITE
            else:
                v[o, max(p, 1), j] = np.nan
        elif kind == NAN_ALL:
            v[o, :, j] = np.nan
        elif kind == INF_ALONE:
            v[o, p, j] = np.inf
        elif kind == INF_BOTH:
            if n == 1:
                v[o, p, j] = -np.inf
            else:
                v[o, p, j] = np.inf
                v[o, (p + n // 2) % n if (p + n // 2) % n != p else (p + 1) % n, j] = -np.inf
        else:   # an Inf with a NaN right behind it (in front of it at the very end of the axis); never a NaN in position 0
            if n == 1:
                v[o, p, j] = np.inf
            elif n == 2:
                v[o, 0, j], v[o, 1, j] = np.inf, np.nan
            else:
                q = min(max(p, 1), n - 2)
                v[o, q, j], v[o, q + 1, j] = np.inf, np.nan
        kinds[s] = kind
    return x, kinds.reshape(_out_shape(x.shape, axis))


def zero_extremes(shape, axis, seed):
    """Slices whose minimum is a zero, with +0 and -0 both present (their order differs from slice to slice), and whose
    maximum is a zero likewise in the negated array: the sign of such an extreme is the one thing a tree order does not fix."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.125, 0.96875, size=shape).astype(np.float32)
    v = _slices(x, axis)
    outer, n, inner = v.shape
    if n < 2:
        raise ValueError("zero_extremes: needs two positions")
    s = np.arange(outer * inner, dtype=np.int64)
    a = rng.integers(0, n, size=s.size)
    b = (a + 1 + rng.integers(0, n - 1, size=s.size)) % n
    v[s // inner, a, s % inner] = 0.0
    v[s // inner, b, s % inner] = -0.0
    return x


def minmax_loop(x, axis, op):
    """The reference's loop, literally: start from position 0, replace on a strict compare."""
    v = _slices(x, axis)
    m = v[:, 0, :].copy()
    with np.errstate(invalid="ignore"):
        for i in range(1, v.shape[1]):
            e = v[:, i, :]
            take = (e > m) if op == "max" else (e < m)
            m = np.where(take, e, m)
    return m.reshape(_out_shape(np.shape(x), axis)).astype(np.float32)


def _minmax_closed(x, axis, op):
    """What that loop returns without walking it: position 0 if it is a NaN, else the extreme of the slice's numbers."""
    v = _slices(x, axis)
    first = v[:, 0, :]
    with np.errstate(invalid="ignore"):
        m = (np.fmax if op == "max" else np.fmin).reduce(v, axis=1)
    m = np.where(np.isnan(first), first, m)
    return m.reshape(_out_shape(np.shape(x), axis)).astype(np.float32)


def expected(x, axis, op):
    """What `op` over `axis` (None: the flat array) must return for a member of the family, as fp32, computed without a float
    accumulation; ValueError for an array outside the exact range of that op."""
    x = np.asarray(x, dtype=np.float32)
    v = _slices(x, axis)
    outer, n, inner = v.shape
    shape = _out_shape(x.shape, axis)
    if op in ("min", "max"):
        return (minmax_loop if n <= LOOP_MAX else _minmax_closed)(x, axis, op)
    nan = np.isnan(v).any(axis=1)
    pinf = (v == np.inf).any(axis=1)
    ninf = (v == -np.inf).any(axis=1)
    finite = np.isfinite(v)
    if op in ("sum", "mean"):
        f = np.where(finite, v, np.float32(0))
        if (f != np.rint(f)).any():
            raise ValueError("expected(%s): not integers" % op)
        i = f.astype(np.int64)
        if int(np.abs(i).sum(axis=1).max()) >= EXACT_LIMIT:
            raise ValueError("expected(%s): sum |x| over a slice leaves the exact fp32 range (2^24)" % op)
        r = i.sum(axis=1).astype(np.float32)
        with np.errstate(invalid="ignore"):
            r = np.where(pinf, np.float32(np.inf), r)
            r = np.where(ninf, np.float32(-np.inf), r)
            r = np.where(nan | (pinf & ninf), np.float32(np.nan), r).astype(np.float32)
            if op == "mean":
                r = (r / np.float32(n)).astype(np.float32)      # one correctly rounded division: __fdiv_rn(r, n)
        return r.reshape(shape)
    if op != "prod":
        raise ValueError("expected: unknown op %r" % (op,))
    ok = ~finite | (v == -1.0) | (v == 2.0) | (v == 0.5)
    if not ok.all():
        raise ValueError("expected(prod): values other than -1, 2, 0.5")
    k2, kh = (v == 2.0).sum(axis=1), (v == 0.5).sum(axis=1)
    if int(k2.max()) > PROD_LIMIT or int(kh.max()) > PROD_LIMIT:
        raise ValueError("expected(prod): more than %d factors of 2 or 0.5 in a slice" % PROD_LIMIT)
    negative = ((v == -1.0) | (v == -np.inf)).sum(axis=1)
    sign = np.where(negative % 2 == 1, np.float32(-1), np.float32(1))
    r = np.ldexp(sign, (k2 - kh).astype(np.int32)).astype(np.float32)
    r = np.where(pinf | ninf, sign * np.float32(np.inf), r)
    r = np.where(nan, np.float32(np.nan), r).astype(np.float32)
    return r.reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mismatches(got, want, either_zero=None):
    """Outputs whose bits differ from the expected ones.  Any NaN matches any NaN (the payload is not part of the contract);
    where `either_zero` is set, +0 and -0 match each other (zero_extremes)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    if either_zero is not None:
        same = same | (np.asarray(either_zero, dtype=bool) & (got == 0.0) & (want == 0.0))
    return np.flatnonzero(~same.reshape(-1))
