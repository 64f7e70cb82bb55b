"""The calibration of the SVD bound tests, held to its own bound without a GPU (tests/svd_family.py).

jacobi_svd_emulated (fp32 storage and dot products, fp64 rotations, unblocked one-sided Jacobi) is what the device results
are compared with for max(m, n) <= 512; here it must stay, on every such input, under twice max(2, max(m, n) / 4) eps — the
convention of tests/test_gpu_linalg.py::_bound, twice because the tightest case sits close to the convention and numpy's
fp32 summation order differs between builds.  The input families are checked too: the exact family is exact, the Hadamard
family is exact in fp32 with the closed-form spectrum, the conditioning figures the GPU tests rely on hold."""
import numpy as np
import pytest

from tests import svd_family as F

SMALL_SQUARES = [n for n in F.SQUARE_SIZES if n <= 300]
SMALL_RECT = [s for s in F.RECT_SHAPES if max(s) <= 512]


def _check(a, sigma=None, excluded=0):
    m, n = a.shape
    U, S, Vt, sweeps, ok = F.jacobi_svd_emulated(a)
    mt = F.metrics(a, U, S, Vt, sigma)
    print(a.shape, "sweeps", sweeps, {k: (round(v / F.EPS, 2) if k != "live" else v) for k, v in mt.items()})
    assert ok and sweeps < 30
    assert mt["live"] == min(m, n) - excluded
    assert np.all(S[:-1] >= S[1:])
    for key in ("rec", "orthA", "orthN", "serr"):
        assert mt[key] <= 2 * F.bound(m, n), (key, mt[key] / F.EPS)


@pytest.mark.parametrize("n", SMALL_SQUARES)
def test_emulator_on_shifted_squares(n):
    _check(F.shifted_square(n))


@pytest.mark.parametrize("shape", SMALL_RECT)
def test_emulator_on_rectangles(shape):
    _check(F.gaussian(*shape))


def test_emulator_on_scaled_columns():
    _check(F.scaled_case(512, 256))


def test_emulator_on_the_rank_deficient_product():
    m, n, r = F.RANK_CASES[0]
    _check(F.rank_case(m, n, r), excluded=min(m, n) - r)


@pytest.mark.parametrize("shape", [s for s in F.HADAMARD_SHAPES if max(s) <= 512])
def test_emulator_on_the_known_spectrum(shape):
    a, sigma = F.hadamard_case(*shape)
    _check(a, sigma)


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (63, 63), (64, 200), (200, 64)])
def test_emulator_is_exact_on_the_exact_family(shape):
    a, d, U0, Vt0 = F.exact_case(*shape)
    U, S, Vt, sweeps, ok = F.jacobi_svd_emulated(a)
    assert ok and sweeps == 1
    assert np.array_equal(S, np.sort(d)[::-1])
    assert set(np.unique(np.abs(U))) <= {0.0, 1.0} and set(np.unique(np.abs(Vt))) <= {0.0, 1.0}
    assert np.array_equal((U * S) @ Vt, a)


def test_exact_family_values_are_distinct_and_exactly_squarable():
    rng = np.random.default_rng(1)
    d = F.exact_values(4097, rng).astype(np.float64)
    assert len(np.unique(d)) == 4097
    sq = (d * d).astype(np.float32).astype(np.float64)
    assert np.array_equal(sq, d * d) and np.array_equal(np.sqrt(sq), d)


def test_exact_case_reconstructs_in_float64():
    a, d, U0, Vt0 = F.exact_case(65, 200)
    assert np.array_equal((U0.astype(np.float64) * d.astype(np.float64)) @ Vt0.astype(np.float64), a.astype(np.float64))
    assert np.allclose(F.sigma64(a), np.sort(d.astype(np.float64))[::-1], rtol=1e-13, atol=0)   # LAPACK in float64: not bit for bit


@pytest.mark.parametrize("shape", F.HADAMARD_SHAPES[:4])
def test_hadamard_family_is_exact_with_the_closed_form_spectrum(shape):
    a, sigma = F.hadamard_case(*shape)                       # asserts exactness in fp32 itself
    assert np.allclose(F.sigma64(a), sigma, rtol=0, atol=1e-9 * sigma[0])


@pytest.mark.parametrize("case", ["square300", "rect", "scaled", "rank"])
def test_conditioning_figures_the_gpu_tests_rely_on(case):
    if case == "rank":
        m, n, r = F.RANK_CASES[0]
        s = F.sigma64(F.rank_case(m, n, r))
        thr = max(m, n) * F.EPS
        assert s[r - 1] / s[0] > 16 * thr and s[r] / s[0] < thr / 16
        return
    a = {"square300": F.shifted_square(300), "rect": F.gaussian(130, 64), "scaled": F.scaled_case(512, 256)}[case]
    s = F.sigma64(a)
    assert s[-1] / s[0] >= 16 * max(a.shape) * F.EPS
