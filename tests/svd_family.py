"""Inputs, metrics and the CPU calibration of the SVD tests (tests/test_gpu_svd.py, tests/test_svd_reference_cpu.py).

Inputs
  exact_case      a = P diag(d) Q with signed permutations P (m x k, orthonormal signed-unit columns) and Q (k x n) and d a
                  shuffled set of DISTINCT values j 2^e, j odd in 1 .. 4095, e in -3 .. 3.  The columns of a are orthogonal,
                  every dot product has one non-zero term, every squared norm j^2 4^e is exact (j^2 < 2^24) and its root is
                  exact: any correct Jacobi SVD returns S = sort(d) bit for bit, factors with entries 0 / +-1, info = 0.
  hadamard_case   (H_m[:, :n] / sqrt(m)) diag(n .. 1) (H_n / sqrt(n))^T, Sylvester Hadamard matrices, m and n powers of
                  four: exact in fp32 (asserted), singular values n .. 1.
  shifted_square  G + 2 sqrt(n) I, G standard normal: s_min / s_0 about 0.2 whatever n.
  gaussian        plain standard normal (rectangular cases).
  scaled_case     standard normal with the columns scaled by logspace(0, -2).
  rank_case       G(m x r) G(r x n) formed in fp32.

Metrics (float64 arithmetic on the fp32 results, eps = 2^-23, k = min(m, n), live = s_i > max(m, n) eps s_0)
  rec    ||a - U diag(S) Vt||_F / ||a||_F
  orthA  ||Q^T Q - I||_F / sqrt(k) of the accumulated factor (all k vectors): Vt for m >= n, U for m < n
  orthN  the same of the normalised factor over its live vectors only
  serr   max |s_i - sigma_i| / sigma_0, sigma from numpy's float64 SVD of the fp32 input (or a closed form)

jacobi_svd_emulated is the calibration of the bound tests: one-sided cyclic Jacobi, fp32 storage, fp32 dot products, fp64
rotations rounded once, unblocked, round-robin pairs — the same algorithm class as the device code and independent of it
(no blocking, numpy's summation order)."""
import numpy as np

EPS = 2.0 ** -23
f32 = np.float32

EXACT_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (63, 63), (64, 64), (65, 65), (64, 200), (200, 64), (1000, 1000),
                (1024, 4096), (4097, 4097)]
HADAMARD_SHAPES = [(64, 64), (256, 64), (256, 256), (1024, 1024), (4096, 1024)]
SQUARE_SIZES = [1, 2, 3, 4, 7, 8, 31, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1024, 2047, 2048, 4096]
RECT_SHAPES = [(17, 5), (130, 64), (64, 130), (700, 300), (300, 700), (4096, 512)]
SCALED_SHAPES = [(512, 256), (2048, 1024)]
RANK_CASES = [(200, 96, 20), (1024, 1024, 100)]


def exact_values(k, rng):
    """k distinct values j 2^e, shuffled (14336 of them exist)."""
    assert k <= 2048 * 7
    pick = rng.choice(2048 * 7, size=k, replace=False)
    j, e = 2 * (pick % 2048) + 1, pick // 2048 - 3
    return np.ldexp(j.astype(np.float64), e).astype(f32)


def exact_case(m, n, seed=0):
    """-> a, d (in the order of the columns of P), U0 (m x k), Vt0 (k x n) with a = U0 diag(d) Vt0 exactly"""
    rng = np.random.default_rng(4242 + 100003 * m + n + 7919 * seed)
    k = min(m, n)
    d = exact_values(k, rng)
    U0, Vt0 = np.zeros((m, k), f32), np.zeros((k, n), f32)
    U0[rng.permutation(m)[:k], np.arange(k)] = rng.choice(np.array([-1, 1], f32), k)
    Vt0[np.arange(k), rng.permutation(n)[:k]] = rng.choice(np.array([-1, 1], f32), k)
    a = (U0 * d) @ Vt0                       # one non-zero term per entry: exact
    assert np.count_nonzero(a) == k
    return a, d, U0, Vt0


def hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n
    return H


def hadamard_case(m, n):
    """-> a (fp32, exact), sigma = n .. 1"""
    sigma = np.arange(n, 0, -1, dtype=np.float64)
    a64 = (hadamard(m)[:, :n] / np.sqrt(m)) * sigma @ (hadamard(n) / np.sqrt(n)).T
    a = a64.astype(f32)
    assert np.array_equal(a.astype(np.float64), a64)
    return a, sigma


def shifted_square(n):
    rng = np.random.default_rng(31000 + n)
    return (rng.standard_normal((n, n)) + 2.0 * np.sqrt(n) * np.eye(n)).astype(f32)


def gaussian(m, n):
    rng = np.random.default_rng(32000 + 1009 * m + n)
    return rng.standard_normal((m, n)).astype(f32)


def scaled_case(m, n):
    rng = np.random.default_rng(33000 + 1009 * m + n)
    return (rng.standard_normal((m, n)) * np.logspace(0, -2, n)).astype(f32)


def rank_case(m, n, r):
    rng = np.random.default_rng(34000 + 1009 * m + n + r)
    return rng.standard_normal((m, r)).astype(f32) @ rng.standard_normal((r, n)).astype(f32)


def sigma64(a):
    return np.linalg.svd(a.astype(np.float64), compute_uv=False)


def live_count(S, m, n):
    S = np.asarray(S, np.float64)
    return int(np.count_nonzero(S > max(m, n) * EPS * S[0])) if S.size else 0


def _orth(Q):
    """columns of Q"""
    Q = Q.astype(np.float64)
    k = Q.shape[1]
    return float(np.linalg.norm(Q.T @ Q - np.eye(k)) / np.sqrt(k)) if k else 0.0


def metrics(a, U, S, Vt, sigma=None):
    """-> dict(rec, orthA, orthN, serr, live) in units of 1 (divide by EPS to read them)"""
    m, n = a.shape
    a64, U64, S64, Vt64 = a.astype(np.float64), U.astype(np.float64), S.astype(np.float64), Vt.astype(np.float64)
    if sigma is None:
        sigma = sigma64(a)
    na = np.linalg.norm(a64)
    live = live_count(S, m, n)
    acc, nrm = (Vt64.T, U64) if m >= n else (U64, Vt64.T)      # columns = vectors
    return {"rec": float(np.linalg.norm(a64 - (U64 * S64) @ Vt64) / na) if na > 0 else 0.0,
            "orthA": _orth(acc), "orthN": _orth(nrm[:, :live]),
            "serr": float(np.abs(S64 - sigma).max() / sigma[0]) if sigma[0] > 0 else 0.0, "live": live}


def round_robin_steps(n):
    """n - 1 steps (n padded to even) of n / 2 disjoint pairs: position 0 stays, the others go round"""
    ne = n + (n & 1)
    idx = np.arange(ne)
    for _ in range(ne - 1):
        p, q = idx[: ne // 2], idx[::-1][: ne // 2]
        lo, hi = np.minimum(p, q), np.maximum(p, q)
        keep = hi < n
        yield lo[keep], hi[keep]
        idx = np.concatenate(([idx[0]], [idx[-1]], idx[1:-1]))


def _dot32(x, y):
    return np.einsum("ij,ij->i", x, y, dtype=f32) if x.ndim == 2 else f32(np.dot(x, y))


def jacobi_svd_emulated(A, tol=4 * EPS, max_sweeps=30):
    """-> U (m x k), S, Vt (k x n), sweeps taken, converged; fp32 storage, fp64 rotations, unblocked"""
    A = np.asarray(A, f32)
    if A.shape[0] < A.shape[1]:
        U, S, Vt, sweeps, ok = jacobi_svd_emulated(A.T, tol, max_sweeps)
        return Vt.T.copy(), S, U.T.copy(), sweeps, ok
    m, n = A.shape
    W, Vt = A.T.astype(f32).copy(), np.eye(n, dtype=f32)
    thr = max(m, n) * EPS
    sweeps, ok = 0, False
    for sweeps in range(1, max_sweeps + 1):
        worst = 0.0
        big = float(np.sqrt(np.einsum("ij,ij->i", W, W, dtype=f32).astype(np.float64)).max())
        for p, q in round_robin_steps(n):
            if p.size == 0:
                continue
            a = _dot32(W[p], W[p]).astype(np.float64)
            b = _dot32(W[q], W[q]).astype(np.float64)
            g = _dot32(W[p], W[q]).astype(np.float64)
            ok_ab = (a > 0) & (b > 0)
            off = np.where(ok_ab, np.abs(g) / np.sqrt(np.where(ok_ab, a * b, 1.0)), 0.0)
            negligible = (np.sqrt(a) <= thr * big) & (np.sqrt(b) <= thr * big)    # the null space does not rotate noise
            off = np.where(negligible, 0.0, off)
            worst = max(worst, float(off.max()))
            do = off > tol
            if not do.any():
                continue
            z = (b - a) / (2.0 * np.where(do, g, 1.0))
            t = np.where(z >= 0, 1.0, -1.0) / (np.abs(z) + np.sqrt(1.0 + z * z))
            c64 = 1.0 / np.sqrt(1.0 + t * t)
            c = np.where(do, c64, 1.0).astype(f32)[:, None]
            s = np.where(do, c64 * t, 0.0).astype(f32)[:, None]
            for M in (W, Vt):
                Mp, Mq = M[p], M[q]
                M[p], M[q] = c * Mp - s * Mq, s * Mp + c * Mq
        if worst <= tol:
            ok = True
            break
    S = np.sqrt(np.einsum("ij,ij->i", W, W, dtype=f32))
    order = np.argsort(-S, kind="stable")
    S, W, Vt = S[order], W[order], Vt[order]
    with np.errstate(divide="ignore", invalid="ignore"):
        Un = np.where(S[:, None] > 0, W / S[:, None], f32(0))
    return Un.T.astype(f32).copy(), S.astype(f32), Vt, sweeps, ok


def bound(m, n):
    """the convention of tests/test_gpu_linalg.py::_bound"""
    return max(2.0, max(m, n) / 4.0) * EPS
