"""tests/linalg_exact.py pinned on the CPU: its host reference (getf2_ref, det_ref) and every construction against
LAPACK's sgetrf / dgetrf (scipy), the constructions through getf2_ref, and the exactness certificate refusing inexact
inputs.  These are the expected values of tests/test_gpu_linalg_exact.py."""
import numpy as np
import pytest

from tests import linalg_exact as le

SIZES = [1, 2, 3, 4, 7, 16, 17, 63, 64, 65, 128, 129, 200, 300]


def _lapack():
    return pytest.importorskip("scipy.linalg.lapack", reason="scipy is not installed: no LAPACK to pin the reference")


def _check_lapack(M, ipiv, info, packed):
    """sgetrf and dgetrf on M give exactly these pivots, info and factors (LAPACK: 1-based pivots, info = first zero)."""
    lp = _lapack()
    for fn, dt in ((lp.sgetrf, np.float32), (lp.dgetrf, np.float64)):
        lu, piv, inf = fn(np.asarray(M, dt), overwrite_a=False)
        assert inf == info, (fn.__name__, inf, info)
        assert (piv == ipiv).all(), fn.__name__      # scipy already returns LAPACK's pivots 0-based
        assert (lu.astype(np.float64) == packed).all(), fn.__name__


def _check_case(case):
    case.certify()
    M = case.dense_M()
    assert (M.astype(np.float32) == M).all()
    packed = case.packed()
    lu, piv, info = le.getf2_ref(M)
    assert (piv == case.ipiv).all() and info == case.info and (lu == packed).all()
    # P M = L U, P from perm (laswp order)
    assert (case.P() @ M == case.L() @ case.U()).all()
    _check_lapack(M, case.ipiv, case.info, packed)
    return M


def test_scipy_pivots_are_zero_based():
    lu, piv, info = _lapack().sgetrf(np.array([[1.0, 2.0], [3.0, 4.0]], np.float32))
    assert list(piv) == [1, 1] and info == 0


@pytest.mark.parametrize("n", SIZES)
def test_generic(n):
    _check_case(le.generic(n, seed=n))


@pytest.mark.parametrize("n", [1, 5, 64, 129, 257])
def test_generic_dense_u(n):
    _check_case(le.generic(n, seed=3 * n, per=n))


@pytest.mark.parametrize("n", [40, 70, 130, 300])
def test_ties_pick_the_first_row(n):
    ties = [(0, 1), (1, 2), (3, 31), (5, n // 3), (15, 1), (16, 1), (n // 2, 1), (n - 2, 1)]
    ties = [(k, d) for k, d in ties if k + d < n]
    case = le.generic(n, seed=n + 1, ties=ties)
    M = _check_case(case)
    # a tie really is one: at that step some later row has |value| equal to the pivot's
    for k, _ in ties:
        assert (np.abs(case.L()[k + 1:, k]) == 1.0).any(), k


def test_ties_across_waves_and_register_slots():
    n = 1100
    ties = [(0, 64), (1, 1024), (16, 1), (64, 64), (65, 1), (70, 1024)]
    case = le.generic(n, seed=11, ties=ties)
    case.certify()
    lu, piv, info = le.getf2_ref(case.dense_M())
    assert (piv == case.ipiv).all() and info == 0 and (lu == case.packed()).all()


@pytest.mark.parametrize("n,zeros", [(1, [0]), (2, [0]), (2, [1]), (17, [16]), (20, [1, 15]), (130, [0, 64]),
                                     (130, [127, 129]), (300, [65, 200])])
def test_zero_pivots(n, zeros):
    case = le.generic(n, seed=n + sum(zeros), zero_pivots=zeros)
    assert case.info == zeros[0] + 1
    _check_case(case)
    assert case.det() == 0.0


@pytest.mark.parametrize("n", [1, 2, 3, 10, 64, 100, 128])
def test_wilkinson(n):
    case = le.wilkinson(n)
    M = case.dense_M()
    le.certify_stepwise(M)
    W = np.eye(n) - np.tril(np.ones((n, n)), -1)
    W[:, -1] = 1.0
    assert (M == W).all()
    lu, piv, info = le.getf2_ref(M)
    assert (piv == np.arange(n)).all() and info == 0 and (lu == case.packed()).all()
    _check_lapack(M, case.ipiv, 0, case.packed())
    assert case.det() == np.float32(2.0 ** (n - 1))


@pytest.mark.parametrize("n,band", [(129, 128), (200, 40), (300, 299)])
def test_banded_wilkinson(n, band):
    _check_case(le.banded_wilkinson(n, band))


@pytest.mark.parametrize("n", [1, 2, 9, 64, 129, 200])
def test_exact_inverse(n):
    case, inv = le.exact_inverse(n, seed=n)
    M = _check_case(case)
    case.certify(x=inv)
    assert (M @ inv == np.eye(n)).all() and (inv @ M == np.eye(n)).all()
    assert (inv.astype(np.float32) == inv).all()


def test_sparse_product_matches_dense():
    case = le.generic(700, seed=5, per=6)
    M = case.L() @ case.U()
    want = np.zeros_like(M)
    want[case.perm] = M
    assert (case.dense_M() == want).all()
    x = np.arange(700, dtype=np.float64) % 7 - 3
    assert (case.matvec(x) == want @ x).all()


def test_parity_is_forced():
    for par in (0, 1):
        for n in (129, 1000, 4097):
            case = le.generic(n, seed=n + par, parity=par, zero_pivots=[], ties=[(3, 1)])
            assert np.count_nonzero(case.ipiv != np.arange(n)) % 2 == par


def test_large_cases_are_exact_in_linear_time():
    case = le.generic(46341, seed=1)
    case.certify(x=np.full(46341, 4.0))
    r, c, v = case.M_coords()
    assert len(v) > 8 * 46341 and (np.abs(v) < 2 ** 16).all()


def test_det_ref_is_the_references_fp32_loop():
    big, small = 2.0 ** 100, 2.0 ** -100
    ident = np.arange(4)
    assert le.det_ref([big, big, small, small], ident, 0) == np.float32(np.inf)
    assert le.det_ref([-big, big, small, small], ident, 0) == np.float32(-np.inf)
    z = le.det_ref([small, small, big, big], ident, 0)
    assert z == 0.0 and not np.signbit(z)
    z = le.det_ref([small, -small, big, big], ident, 0)
    assert z == 0.0 and np.signbit(z)
    z = le.det_ref([small, small, big, big], np.array([1, 1, 2, 3]), 0)   # one exchange: -(+0)
    assert np.signbit(z)
    assert le.det_ref([big, small, big, small], ident, 0) == 1.0          # float64 det is 1 either way
    assert le.det_ref([2.0, 3.0], np.array([1, 1]), 0) == -6.0
    assert le.det_ref([2.0, 0.0], ident[:2], 2) == 0.0


def test_certificate_rejects_inexact_inputs():
    case = le.generic(64, seed=1)
    case.Uv = case.Uv.copy()
    off = np.nonzero(case.Ur != case.Uc)[0][0]
    case.Uv[off] = 2.0 ** 22 + 1                       # one product no longer fits 24 bits
    with pytest.raises(AssertionError):
        case.certify()
    case = le.generic(64, seed=1)
    case.Lv = case.Lv.copy()
    case.Lv[0] = 1.0 / 3.0                             # not dyadic
    with pytest.raises(AssertionError):
        case.certify()
    case = le.generic(64, seed=1)
    case.Uv = case.Uv.copy()
    case.Uv[0] = 3.0                                   # a diagonal entry that is not a power of two
    case.diag[case.Ur[0]] = 3.0
    with pytest.raises(AssertionError):
        case.certify()
    with pytest.raises(AssertionError):                 # Wilkinson past 2^24 is not blocked-exact
        le.wilkinson(40).certify()
    with pytest.raises(AssertionError):
        le.certify_stepwise(np.array([[3.0, 1.0], [1.0, 1.0]]))   # 1/3 is no fp32 number


def test_partners_are_uniform_over_the_room():
    """L's rows below each column and U's columns right of each row are uniform random subsets of the room: their
    offsets, relative to the room, spread evenly over (0, 1) (a sampler that kept the smallest draws sat near 0.17)."""
    n = 4097
    case = le.generic(n, seed=n)
    for a, b in ((case.Lc, case.Lr), (case.Ur, case.Uc)):
        keep = (b > a) & (b != n - 1)                          # U's last column is there by design
        rel = (b[keep] - a[keep] - 0.5) / (n - 1 - a[keep])
        assert 0.45 < np.median(rel) < 0.55 and np.quantile(rel, 0.9) > 0.85, np.quantile(rel, [0.5, 0.9])


def _large_cases():
    for n in le.LARGE_GETRF:
        yield "getrf-%d" % n, le.large_getrf_case(n)
    for n in le.LARGE_ND:
        yield "nd-%d" % n, le.large_nd_case(n)
        yield "inv-%d" % n, le.large_inverse_case(n)[0]
    yield "solve-%d" % le.LARGE_SOLVE, le.large_solve_case()


def test_large_cases_reach_every_trailing_tile():
    """The cases of test_gpu_linalg_exact.py's large tests: the first step exchanges rows (what perm_kernel's global
    branch has to apply first), every panel's U12 reaches the last column tile of its trailing block, and the panels'
    L21 U12 products reach at least 90 % of the 128 x 128 tiles: an error confined to a far tile changes a compared value."""
    for name, case in _large_cases():
        assert case.ipiv[0] != 0, name
        panels, reach_last, frac = le.trailing_coverage(case)
        assert reach_last == panels, (name, reach_last, panels)
        assert frac >= 0.9, (name, frac)


def test_inverse_coordinates_are_exact():
    for n in (3, 64, 257, 700):
        case, (r, c, v) = le.exact_inverse(n, seed=n, dense=False, first_swap=True)
        case.certify(x_coords=(r, c, v))
        inv = np.zeros((n, n))
        inv[r, c] = v
        M = case.dense_M()
        assert (M @ inv == np.eye(n)).all() and (inv @ M == np.eye(n)).all()
        assert case.ipiv[0] != 0
    case, (r, c, v) = le.large_inverse_case(16385)
    case.certify(x_coords=(r, c, v))
    # the inverse's columns through M: M (M^-1 e_j) = e_j for a few j, from coordinates only
    for j in (0, 1, 8191, 16384):
        sel = c == j
        col = np.zeros(16385)
        col[r[sel]] = v[sel]
        e = case.matvec(col)
        assert e[j] == 1.0 and np.count_nonzero(e) == 1, j
