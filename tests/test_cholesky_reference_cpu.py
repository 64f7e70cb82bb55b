"""The exact input family of the Cholesky tests is passable by the reference's arithmetic before a GPU is involved: numpy's
fp32 linalg.cholesky (LAPACK spotrf, what the reference's NDArray_Cholesky calls) returns L0 bit for bit on A = L0 L0^T,
and the residual family gives it the residuals the GPU test's comparative bound is built on (tests/cholesky_family.py)."""
import numpy as np
import pytest

from tests.cholesky_family import EPS, exact_case, residual, spd_case

SIZES = list(range(1, 70)) + [127, 128, 129, 191, 192, 193, 300, 1000, 1024, 2049]


@pytest.mark.parametrize("n", SIZES)
def test_lapack_returns_l0_bit_for_bit(n):
    L0, A = exact_case(n)
    assert A.dtype == np.float32 and np.array_equal(A, A.T)
    got = np.linalg.cholesky(A)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), L0.view(np.uint32))


def test_lapack_returns_l0_at_4097():
    L0, A = exact_case(4097)
    assert np.abs(A).max() <= 4 * 4097 + 16
    assert np.array_equal(np.linalg.cholesky(A), L0)


def test_family_entries_and_seeds():
    L0, A = exact_case(500)
    assert set(np.unique(np.diagonal(L0))) <= {1.0, 2.0, 4.0}
    assert np.abs(np.tril(L0, -1)).max() == 2.0 and not np.triu(L0, 1).any()
    L1, _ = exact_case(500, seed=5)
    assert not np.array_equal(L0, L1)
    assert np.array_equal(exact_case(500)[0], L0)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 64, 300, 1000])
def test_lapack_residual_on_the_bound_family_is_below_eps(n):
    A = spd_case(n)
    assert np.array_equal(A, A.T)
    r = residual(A, np.linalg.cholesky(A))
    assert r <= EPS, r / EPS
    assert residual(A, np.zeros_like(A)) == 1.0 and residual(A, np.eye(n, dtype=np.float32)) > 0.05   # a wrong factor is O(1)
