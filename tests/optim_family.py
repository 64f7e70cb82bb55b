"""The definition of the optimizer steps and of the gradient norm (include/np_hip.h, np_optim.hip) restated step by step in numpy,
one np.float32 operation per step of the header's text; the norm in three summation orders with the guard that makes its
bit-for-bit comparison legitimate; the data families the tests use; and the dispatcher (launches, chunks, tensors by access form).
No device and no library: test_optim_reference_cpu.py holds this file to torch, test_gpu_optim.py holds the kernels to it."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53                      # unit roundoff of fp64

# np_debug_optim_bounds: the elements of a step chunk, kOptimMaxTensors, the elements behind one partial of the norm, the
# workgroups per CU that cap a grid, the bytes of the list as a kernel argument
BOUNDS = (4096, 64, 8192, 8, 3152)
CHUNK, MAX_TENSORS, NORM_CHUNK, WG_PER_CU, ARG_BYTES = BOUNDS
ORDERS = ("forward", "reversed", "pairwise")


# ---- the dispatcher (mode_of and launch_steps of np_optim.hip) ----
def mode_of(addresses, force_scalar=False):
    """addresses: the byte addresses of a tensor's pointers (absent ones left out) -> 0 .. 3, the floats between the 16-byte
    boundary and the tensor when all residues mod 16 agree, or None for scalar accesses"""
    residues = {a % 16 for a in addresses}
    if force_scalar or len(residues) != 1:
        return None
    return residues.pop() // 4


def chunks_of(n, mode, chunk=CHUNK):
    return -(-((mode or 0) + n) // chunk)


def plan(tensors, force_scalar=False, bounds=BOUNDS):
    """tensors: [(n, addresses)] -> (launches, chunks, vec_tensors, scalar_tensors) of a step"""
    modes = [mode_of(a, force_scalar) for _, a in tensors]
    return (-(-len(tensors) // bounds[1]), sum(chunks_of(n, m, bounds[0]) for (n, _), m in zip(tensors, modes)),
            sum(m is not None for m in modes), sum(m is None for m in modes))


def norm_plan(counts, bounds=BOUNDS):
    """-> (launches, chunks) of np_grad_norm: a launch per bounds[1] tensors and the fold; a partial per bounds[2] elements"""
    return -(-len(counts) // bounds[1]) + 1, sum(-(-n // bounds[2]) for n in counts)


def grid(chunks, cus, bounds=BOUNDS):
    cap = cus * bounds[3]
    return max(1, chunks) if chunks <= cap else cap | 1


# ---- coefficients: computed in double from the double arguments, rounded to fp32 ONCE ----
def sgd_coefficients(lr, momentum=0.0, dampening=0.0, weight_decay=0.0):
    return {"lr": F32(lr), "wd": F32(weight_decay), "mu": F32(momentum), "omd": F32(1.0 - dampening)}


def adam_coefficients(step, lr, beta1, beta2, eps, weight_decay):
    return {"wd": F32(weight_decay), "lrwd": F32(lr * weight_decay), "b1": F32(beta1), "omb1": F32(1.0 - beta1), "b2": F32(beta2),
            "omb2": F32(1.0 - beta2), "bc2s": F32(math.sqrt(1.0 - math.pow(beta2, float(step)))), "eps": F32(eps),
            "ss": F32(lr / (1.0 - math.pow(beta1, float(step))))}


# ---- the element: every line is ONE fp32 operation ----
def sgd_step(p, g, b=None, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=False, scale=None):
    """-> (p, b) after one np_sgd_step; b is None without a momentum.  scale: the value of *grad_scale, or None"""
    k = sgd_coefficients(lr, momentum, dampening, weight_decay)
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    with np.errstate(all="ignore"):
        if scale is not None:
            g = g * F32(scale)
        if weight_decay != 0.0:
            t = k["wd"] * p
            g = g + t
        d = g
        if momentum != 0.0:
            if first_step:
                b = g.copy()
            else:
                t1 = k["mu"] * np.asarray(b, F32)
                t2 = k["omd"] * g
                b = t1 + t2
            if nesterov:
                t = k["mu"] * b
                d = g + t
            else:
                d = b
        else:
            b = None
        u = k["lr"] * d
        p = p - u
    return p, b


def adam_step(p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, scale=None):
    """-> (p, m, v) after one np_adam_step"""
    k = adam_coefficients(step, lr, betas[0], betas[1], eps, weight_decay)
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if scale is not None:
            g = g * F32(scale)
        p1 = p
        if weight_decay != 0.0:
            if decoupled:
                t = k["lrwd"] * p
                p1 = p - t
            else:
                t = k["wd"] * p
                g = g + t
        m1 = k["b1"] * m
        m2 = k["omb1"] * g
        m = m1 + m2
        v1 = k["b2"] * v
        v2 = k["omb2"] * g
        v3 = v2 * g
        v = v1 + v3
        r = np.sqrt(v)
        q = r / k["bc2s"]
        den = q + k["eps"]
        w = m / den
        u = k["ss"] * w
        p = p1 - u
    return p, m, v


# ---- the norm ----
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


def grad_norm(grads, max_norm=math.inf, order="forward"):
    """-> (np.array([norm, coefficient], float32), wide): the fp64 values behind the norm, for `guard`"""
    with np.errstate(all="ignore"):
        x = np.concatenate([np.asarray(g, F32).reshape(-1) for g in grads]).astype(F64)
        S = _sum(x * x, order)                     # each square is exact in double
        norm64 = np.sqrt(S)
        norm = F32(norm64)
        c = F64(max_norm) / (F64(norm) + F64(1e-6))
        coefficient = F32(c if c < 1.0 else c if c != c else 1.0)
    return np.array([norm, coefficient], F32), {"n": x.size, "S": S, "norm64": norm64}


def guard(wide):
    """True when no order of the n additions can move f32(sqrt(S)).  The terms are not negative, so any order's sum is within
    (n - 1) . u64 . S of the exact one (relatively, to first order, with a factor two kept in hand); the square root halves a
    relative error and adds one rounding of its own.  That interval around norm64 must not reach a rounding boundary of fp32:
    the midpoints between f32(norm64) and its two neighbours."""
    norm64, n = wide["norm64"], wide["n"]
    if not np.isfinite(norm64) or norm64 == 0.0:
        return True                                   # a class, not a value: every order gives it
    r = F32(norm64)
    lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
    margin = min(abs(norm64 - (F64(lo) + F64(r)) / 2.0), abs((F64(hi) + F64(r)) / 2.0 - norm64))
    return margin > 2.0 * norm64 * (n * U64 / 2.0 + U64)


# ---- data families ----
# the norm cases of test_gpu_optim.py: (seed, the tensors' element counts); test_optim_reference_cpu.py shows that the guard clears for each
NORM_CASES = ((1, (1,)), (2, (5, 3)), (3, (8191, 8192, 8193)), (4, (16385, 1, 4099)), (5, tuple([3] * 63)), (6, tuple([2] * 64)),
              (7, tuple([1] * 65)), (8, tuple([5] * 129)), (9, (40000,)))


def norm_data(seed, counts):
    rng = np.random.default_rng(1000 + seed)
    return [gaussian(rng, n) for n in counts]


def gaussian(rng, n, scale=1.0):
    return (rng.standard_normal(n) * scale).astype(F32)


def exact_family(n, steps=5):
    """Operands and closed forms on which every intermediate of momentum SGD and of Adam is representable, so the closed form holds
    by bits.  -> dict.  SGD: p = 64, g = i mod 7 - 3 (small integers), lr = 2^-3, mu = 2^-1, wd = 0: after k steps the buffer is
    g . (2 - 2^(1-k)) and p = 64 - lr . g . sum of the buffers' factors.  Adam, a ONE-step case: m = 0, v = 0, g = +-2^j, beta1 = 2^-1, beta2 = 3/4, eps = 0, step = 1, lr = 2^-4:
    m' = g / 2, v' = g^2 / 4 (a perfect square), bc2s = sqrt(1/4) = 1/2, den = (|g| / 2) / (1/2) = |g|, ss = lr / (1/2) = 2^-3,
    p' = p - 2^-3 . sign(g) / 2."""
    i = np.arange(n)
    g = ((i % 7) - 3).astype(F32)
    p0 = np.full(n, 64.0, F32)
    factors, b, total = [], 0.0, 0.0
    for k in range(steps):
        b = 1.0 if k == 0 else 0.5 * b + 1.0
        total += b
        factors.append((b, total))
    sgd = {"p0": p0, "g": g, "lr": 0.125, "momentum": 0.5,
           "closed": [((p0.astype(F64) - 0.125 * g.astype(F64) * t).astype(F32), (g.astype(F64) * bf).astype(F32)) for bf, t in factors]}
    ga = (np.where(i % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 9) - 4)).astype(F32)
    pa = ((i % 5) - 2).astype(F32)
    adam = {"p0": pa, "g": ga, "lr": 2.0 ** -4, "betas": (0.5, 0.75), "eps": 0.0,
            "closed": ((pa.astype(F64) - 2.0 ** -3 * np.sign(ga) / 2.0).astype(F32), (ga.astype(F64) / 2.0).astype(F32),
                       (ga.astype(F64) ** 2 / 4.0).astype(F32))}
    return {"sgd": sgd, "adam": adam}
