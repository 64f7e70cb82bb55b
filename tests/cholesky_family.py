"""The two input families of the Cholesky tests (tests/test_gpu_cholesky.py, tests/test_cholesky_reference_cpu.py).

exact_case   L0 lower triangular, strict-lower entries in -2 .. 2, diagonal entries in {1, 2, 4}; A = L0 L0^T.  Every
             partial sum of A's entries and of any correct factorization order is an integer of magnitude <= 4 n + 16
             < 2^24, every square root is of a perfect square and every scaling is by a power of two, so the fp32 Cholesky
             factor of A is exactly L0 in any order of summation.  For the same reason the fp32 product below IS the int64
             product cast to fp32 (checked outright up to n = 300), which keeps n = 16385 affordable.
spd_case     A = X X^T / n + I with X standard normal, symmetrised from its lower triangle: well conditioned, so the
             residual of a backward-stable factorization sits well below eps whatever n.
residual     ||A - L L^T||_1 / ||A||_1 in float64."""
import numpy as np

EPS = 2.0 ** -23


def exact_case(n, seed=None):
    rng = np.random.default_rng(77000 + n if seed is None else 1000003 * seed + n)
    L0 = np.tril(rng.integers(-2, 3, (n, n), dtype=np.int8), -1)
    L0[np.diag_indices(n)] = rng.choice(np.array([1, 2, 4], np.int8), n)
    Lf = L0.astype(np.float32)
    A = Lf @ Lf.T
    if n <= 300:
        L64 = L0.astype(np.int64)
        assert np.array_equal(A, (L64 @ L64.T).astype(np.float32))
    assert float(np.abs(A).max()) <= 4 * n + 16 < 2 ** 24
    return Lf, A


def spd_case(n):
    rng = np.random.default_rng(1000 + 7 * n)
    X = rng.standard_normal((n, n)).astype(np.float32)
    A = X @ X.T / np.float32(n) + np.eye(n, dtype=np.float32)
    return np.tril(A) + np.tril(A, -1).T


def residual(A, L):
    A64, L64 = A.astype(np.float64), np.asarray(L).astype(np.float64)
    return float(np.abs(A64 - L64 @ L64.T).sum(axis=0).max() / np.abs(A64).sum(axis=0).max())
