"""CPU-tier checks of what tests/test_gpu_eigh.py measures the device eigensolver against (tests/eig_family.py): the closed-form
spectra are the spectra numpy's float64 eigvalsh finds, the Hadamard inputs are exact in fp32, the emulator that calibrates the
bound tests stays within max(8, n) eps on every metric and follows the order and sign rules the device code documents.

max(8, n) eps: every row of Vt and of W takes part in n - 1 rotations per sweep, each adding about 1.5 eps of relative rounding
(c and s rounded once, two products and a sum); over the 8 to 17 sweeps these inputs take that is a random walk of some
1.5 sqrt(17 n) eps, under n eps from n = 40 on, and the floor of 8 eps covers the sizes below.  A dropped or mis-paired
rotation gives O(1).  (Measured: 0.08 to 0.22 n eps from n = 64 on, up to 3.7 eps at n = 7.)"""
import numpy as np
import pytest

from tests import eig_family as F

EPS = F.EPS


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.parametrize("n", F.TOEPLITZ_SIZES)
def test_toeplitz_closed_form(n):
    a, lam, vec = F.toeplitz(n)
    assert np.array_equal(a, a.T) and np.all(np.diff(lam) > 0)
    assert np.abs(F.w64(a) - lam).max() <= 64 * np.finfo(np.float64).eps * 4
    r = a.astype(np.float64) @ vec - vec * lam
    assert np.abs(r).max() <= 1e-13 and np.abs(vec.T @ vec - np.eye(n)).max() <= 1e-13


@pytest.mark.parametrize("n", F.HADAMARD_SIZES)
def test_hadamard_inputs_are_exact_and_have_the_stated_spectrum(n):
    a, d = F.hadamard_case(n)                                   # asserts exactness and symmetry itself
    assert a.dtype == np.float32 and np.array_equal(d, np.arange(-n // 2, n // 2))
    assert np.abs(F.w64(a) - d).max() <= 1e-10 * n


@pytest.mark.parametrize("n", F.EXCHANGE_SIZES)
def test_exchange_spectrum(n):
    a, lam = F.exchange(n)
    assert not np.diag(a)[: n // 2].any() and np.array_equal(a, a.T)
    assert np.abs(F.w64(a) - lam).max() <= 1e-12
    assert np.count_nonzero(lam == -1) == n // 2 and np.count_nonzero(lam == 1) == n - n // 2


@pytest.mark.parametrize("n", [5, 64, 130])
def test_rank_one_shift_spectrum(n):
    a, lam = F.rank_one_shift(n)
    assert np.array_equal(a, a.T) and np.array_equal(a.astype(np.float64), a.astype(np.float64).round())
    assert np.abs(F.w64(a) - lam).max() <= 1e-11 * lam[-1]


@pytest.mark.parametrize("n", [1, 2, 3, 33, 65])
def test_exact_diagonal_family(n):
    a, d = F.exact_diagonal(n)
    assert a.dtype == np.float32 and np.array_equal(_bits(np.diag(a)), _bits(d)) and np.count_nonzero(a) == np.count_nonzero(d)
    assert np.unique(d).size == n - (1 if n >= 3 else 0)       # distinct but for the two zeros
    if n >= 3:
        assert (d < 0).any() and np.count_nonzero(np.signbit(d) & (d == 0)) == 1 and np.count_nonzero(d == 0) == 2
    w, order = F.sorted_stable(d)
    assert np.all(np.diff(w) >= 0) and np.array_equal(_bits(w), _bits(d[order]))


@pytest.mark.parametrize("family", sorted(F.BOUND_FAMILIES))
@pytest.mark.parametrize("n", [s for s in F.BOUND_SIZES if s <= 257])
def test_the_emulator_meets_its_own_bound(family, n):
    a = F.BOUND_FAMILIES[family](n)
    assert np.array_equal(a, a.T)
    w, v, sweeps, ok = F.jacobi_eigh_emulated(a)
    got = F.metrics(a, w, v)
    print("emulator %s n %d sweeps %d (eps) %s" % (family, n, sweeps, {k: round(got[k] / EPS, 2) for k in F.METRICS}))
    assert ok and sweeps <= 20
    for key in F.METRICS:
        assert got[key] <= max(8.0, n) * EPS, (key, got[key] / EPS)


def test_the_emulator_reads_the_lower_triangle_only_and_follows_the_order_and_sign_rules():
    a = F.random_symmetric(24)
    b = a.copy()
    b[np.triu_indices(24, 1)] = np.nan
    w, v, _, ok = F.jacobi_eigh_emulated(a)
    w2, v2, _, ok2 = F.jacobi_eigh_emulated(b)
    assert ok and ok2 and np.array_equal(_bits(w), _bits(w2)) and np.array_equal(_bits(v), _bits(v2))
    assert np.all(np.diff(w) >= 0)
    at = np.argmax(np.abs(v), axis=0)                            # the first index of the largest magnitude
    assert np.all(v[at, np.arange(24)] > 0)
    d = np.array([3, -1, 0.0, 3, -0.0, 2], np.float32)
    w, v, sweeps, ok = F.jacobi_eigh_emulated(np.diag(d))
    assert ok and sweeps == 1
    assert np.array_equal(_bits(w), _bits(np.array([-1, 0.0, -0.0, 2, 3, 3], np.float32)))   # ties in diagonal order
    assert np.array_equal(v, np.eye(6, dtype=np.float32)[:, [1, 2, 4, 5, 0, 3]])
    x, lam = F.exchange(2)
    w, v, sweeps, ok = F.jacobi_eigh_emulated(x)
    assert ok and sweeps == 2 and np.array_equal(w, lam.astype(np.float32))
    assert np.array_equal(np.sign(v), np.array([[1, 1], [-1, 1]], np.float32))


def test_sign_rule_helper_takes_the_first_of_equal_magnitudes():
    v = np.array([[-0.5, 0.5], [0.5, -0.5], [0.1, 0.7]], np.float32)
    out = F.apply_sign_rule(v)
    assert np.array_equal(out[:, 0], -v[:, 0]) and np.array_equal(out[:, 1], v[:, 1])
