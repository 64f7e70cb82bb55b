"""det / inv / solve / lu on the device LU (np_lu.hip, host/numpower_linalg.cpp, DESIGN.md "LU").

Known answers are exact; everything else is checked against numpy in float64 with normwise bounds
(eps = 2^-23): inv ||a x - I|| / (||a|| ||x||), solve ||a x - b|| / (||a|| ||x||) and lu ||P a - L U|| / ||a||
within n eps / 4, det of I + G / (4 sqrt n) within n eps relative.  LAPACK fp32 sits at 0.002-0.03 of n eps on
these inputs; a wrong pivot or a dropped update gives O(1).  Below n = 8 the bound is floored at 2 eps: one
correctly rounded division alone may cost eps / 2."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
SIZES = [1, 2, 3, 7, 31, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1024, 2047, 4096]
SINGULAR = "LU factorization failed. Unable to compute the matrix inverse.\n"


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _bound(n):
    return max(n * EPS / 4, 2 * EPS)


def _gauss(n, k=None, seed=0):
    rng = np.random.default_rng(1000 + 7 * n + (k or 0) + seed)
    return rng.standard_normal((n, n if k is None else k)).astype(np.float32)


def _fro(x):
    return float(np.linalg.norm(x))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _gpu(a):
    return _nd().array(a).gpu()


# ---- known answers ----------------------------------------------------------------------------------------------

def test_inv_known_answer_is_exact():
    # the reference's tests/linalg/002-ndarray-inv.phpt prints exactly -2, 1, 1.5, -0.5
    got = _nd().inv(_gpu([[1.0, 2.0], [3.0, 4.0]])).cpu().numpy()
    assert (_bits(got) == _bits([[-2.0, 1.0], [1.5, -0.5]])).all(), got


def test_det_known_answers_are_exact():
    nd = _nd()
    assert nd.det(_gpu([[1.0, 2.0], [3.0, 4.0]])) == -2.0
    for perm, sign in (([0, 1, 2], 1.0), ([1, 0, 2], -1.0), ([1, 2, 0], 1.0), ([2, 1, 0], -1.0), ([3, 0, 2, 1], 1.0)):
        p = np.eye(len(perm), dtype=np.float32)[perm]
        sign = float(round(np.linalg.det(p)))
        assert nd.det(_gpu(p)) == sign, perm
    # triangular: the product of the diagonal (entries that make every elimination step exact)
    assert nd.det(_gpu([[8.0, 0.0, 0.0], [1.0, 4.0, 0.0], [2.0, 1.0, 2.0]])) == 64.0
    assert nd.det(_gpu([[8.0, 1.0, 2.0], [0.0, 4.0, 1.0], [0.0, 0.0, 2.0]])) == 64.0
    assert nd.det(_gpu([[-3.0, 0.0], [5.0, 2.0]])) == -6.0
    # a 3 x 3 whose factorization takes two row exchanges
    assert nd.det(_gpu([[0.0, 2.0, 1.0], [0.0, 0.0, 3.0], [4.0, 0.0, 0.0]])) == 24.0


def test_lu_known_answer_with_two_exchanges():
    a = np.array([[1, 1, 1], [2, 3, 5], [4, 6, 8]], np.float32)
    p, l, u = (x.cpu().numpy() for x in _nd().lu(_gpu(a)))
    np.testing.assert_array_equal(p, [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
    np.testing.assert_array_equal(l, [[1, 0, 0], [0.25, 1, 0], [0.5, 0, 1]])
    np.testing.assert_array_equal(u, [[4, 6, 8], [0, -0.5, -1], [0, 0, 1]])


# ---- bounds ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_inv_bound(n):
    a = _gauss(n)
    x = _nd().inv(_gpu(a)).cpu().numpy()
    a64, x64 = a.astype(np.float64), x.astype(np.float64)
    r = _fro(a64 @ x64 - np.eye(n)) / (_fro(a64) * _fro(x64))
    assert r <= _bound(n), (n, r / (n * EPS))


@pytest.mark.parametrize("n", SIZES)
def test_solve_bound(n):
    a = _gauss(n)
    ga = _gpu(a)
    a64 = a.astype(np.float64)
    for k in sorted({1, 3, n}):
        b = _gauss(n, k, seed=1)
        x = _nd().solve(ga, _gpu(b)).cpu().numpy()
        assert x.shape == (n, k)
        x64 = x.astype(np.float64)
        r = _fro(a64 @ x64 - b.astype(np.float64)) / (_fro(a64) * _fro(x64))
        assert r <= _bound(n), (n, k, r / (n * EPS))


@pytest.mark.parametrize("n", SIZES)
def test_lu_bound_and_structure(n):
    a = _gauss(n)
    p, l, u = (x.cpu().numpy() for x in _nd().lu(_gpu(a)))
    # P: an exact permutation matrix
    assert set(np.unique(p)) <= {0.0, 1.0}
    assert (p.sum(0) == 1).all() and (p.sum(1) == 1).all()
    # L: exactly unit lower with |L| <= 1, U: exactly upper
    assert (np.triu(l, 1) == 0).all() and (np.diag(l) == 1).all() and (np.abs(l) <= 1).all()
    assert (np.tril(u, -1) == 0).all()
    perm = p.argmax(1)
    r = _fro(a.astype(np.float64)[perm] - l.astype(np.float64) @ u.astype(np.float64)) / _fro(a.astype(np.float64))
    assert r <= _bound(n), (n, r / (n * EPS))


@pytest.mark.parametrize("n", SIZES)
def test_det_bound(n):
    a = (np.eye(n) + _gauss(n) / (4 * np.sqrt(n))).astype(np.float32)
    got = _nd().det(_gpu(a))
    want = np.linalg.det(a.astype(np.float64))
    assert abs(got - want) <= max(n * EPS, 2 * EPS) * abs(want), (n, got, want)


def test_solve_large_single_rhs():
    n = 8192
    a = _gauss(n)
    b = _gauss(n, 1, seed=1)
    x = _nd().solve(_gpu(a), _gpu(b)).cpu().numpy().astype(np.float64)
    a64 = a.astype(np.float64)
    r = _fro(a64 @ x - b.astype(np.float64)) / (_fro(a64) * _fro(x))
    assert r <= _bound(n), r / (n * EPS)


# ---- singular and special inputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 50, 300])
def test_zero_column_is_singular(n):
    nd = _nd()
    a = _gauss(n)
    a[:, n // 2] = 0.0
    ga, gb = _gpu(a), _gpu(_gauss(n, 2, seed=1))
    assert nd.det(ga) == 0.0
    before = nd.live_device_allocations()
    with pytest.raises(Exception, match="LU factorization failed"):
        nd.inv(ga)
    with pytest.raises(Exception) as e:
        nd.solve(ga, gb)
    assert str(e.value) == SINGULAR
    assert nd.live_device_allocations() == before


@pytest.mark.parametrize("n", [6, 200])
def test_nan_input_finishes(n):
    nd = _nd()
    a = _gauss(n)
    a[n // 3, n // 2] = np.nan
    ga = _gpu(a)
    assert np.isnan(nd.det(ga))
    nd.inv(ga).cpu().numpy()
    nd.solve(ga, _gpu(_gauss(n, 1, seed=1))).cpu().numpy()
    for x in nd.lu(ga):
        x.cpu().numpy()


# ---- errors ------------------------------------------------------------------------------------------------------

def test_shape_and_device_errors():
    nd = _nd()
    vec, rect, sq = _gpu([1.0, 2.0, 3.0]), _gpu(np.ones((2, 3), np.float32)), _gpu(np.eye(3, dtype=np.float32))
    for fn in (nd.det, nd.inv, nd.lu):
        with pytest.raises(Exception, match="Array must be at least two-dimensional"):
            fn(vec)
        with pytest.raises(Exception, match="Array must be square"):
            fn(rect)
    with pytest.raises(Exception, match="Incompatible shapes"):
        nd.solve(sq, _gpu(np.ones((4, 1), np.float32)))
    with pytest.raises(Exception, match="Incompatible shapes"):
        nd.solve(sq, _gpu([1.0, 2.0, 3.0]))
    with pytest.raises(Exception, match="Incompatible shapes"):
        nd.solve(rect, _gpu(np.ones((2, 1), np.float32)))
    with pytest.raises(Exception, match="Both NDArray must be in the same device."):
        nd.solve(sq, nd.array(np.ones((3, 1), np.float32)))


# ---- determinism, views, the GEMM ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [100, 1024, 4096])
def test_bit_identical_from_run_to_run(n):
    nd = _nd()
    a, b = _gauss(n, seed=3), _gauss(n, 5, seed=4)
    ga, gb = _gpu(a), _gpu(b)
    runs = []
    for _ in range(2):
        runs.append([nd.inv(ga).cpu().numpy(), nd.solve(ga, gb).cpu().numpy(), np.float32(nd.det(ga))]
                    + [x.cpu().numpy() for x in nd.lu(ga)])
    for r0, r1 in zip(*runs):
        assert (_bits(r0) == _bits(r1)).all()


@pytest.mark.parametrize("n", [40, 300])
def test_views_give_the_bits_of_their_contiguous_copy(n):
    nd = _nd()
    big = _gauss(2 * n, seed=5)
    gbig = _gpu(big)
    view = gbig.slice([0, n], [n, 2 * n])          # a strided window of a larger array
    copy = _gpu(np.ascontiguousarray(big[:n, n:]))
    t = nd.transpose(copy)
    tcopy = _gpu(np.ascontiguousarray(big[:n, n:].T))
    b = _gpu(_gauss(n, 2, seed=6))
    for x, y in ((view, copy), (t, tcopy)):
        assert (_bits(nd.inv(x).cpu().numpy()) == _bits(nd.inv(y).cpu().numpy())).all()
        assert (_bits(nd.solve(x, b).cpu().numpy()) == _bits(nd.solve(y, b).cpu().numpy())).all()
        assert np.float32(nd.det(x)).view(np.uint32) == np.float32(nd.det(y)).view(np.uint32)
        for p, q in zip(nd.lu(x), nd.lu(y)):
            assert (_bits(p.cpu().numpy()) == _bits(q.cpu().numpy())).all()


def _sgemm_bits(hip, M, N, K):
    rng = np.random.default_rng(M + N + K)
    A = hip.DeviceArray.from_host(rng.standard_normal((M, K)).astype(np.float32))
    B = hip.DeviceArray.from_host(rng.standard_normal((K, N)).astype(np.float32))
    return hip.sgemm(A, B).to_host().view(np.uint32)


def test_lu_leaves_the_gemm_alone(hip):
    shapes = [(4096, 4096, 4096), (1000, 777, 1500)]
    before = [_sgemm_bits(hip, *s) for s in shapes]
    nd = _nd()
    a = _gauss(1500, seed=7)
    nd.inv(_gpu(a)).cpu().numpy()
    nd.solve(_gpu(a), _gpu(_gauss(1500, 9, seed=8))).cpu().numpy()
    after = [_sgemm_bits(hip, *s) for s in shapes]
    for x, y in zip(before, after):
        assert (x == y).all()


# ---- the C ABI directly ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [50, 500])
def test_getrf_getrs_abi(hip, n):
    from numpower_amd import _lib
    lib = _lib.load()
    a = _gauss(n, seed=9)
    b = _gauss(n, 4, seed=10)
    da = hip.DeviceArray.from_host(a.T)               # the column-major a
    db = hip.DeviceArray.from_host(b.T)               # column-major n x 4
    dpiv, dinfo = hip.DeviceArray((n,)), hip.DeviceArray((1,))   # int32 storage
    _lib.check(lib.np_getrf(da.ptr, n, dpiv.ptr, dinfo.ptr))
    _lib.check(lib.np_getrs(da.ptr, dpiv.ptr, n, 4, db.ptr))
    piv = dpiv.to_host().view(np.int32)
    info = dinfo.to_host().view(np.int32)
    x = db.to_host()
    assert info[0] == 0
    assert (piv >= np.arange(n)).all() and (piv < n).all()
    assert piv[0] == int(np.argmax(np.abs(a[:, 0])))   # isamax of the first column
    x64 = x.T.astype(np.float64)
    a64 = a.astype(np.float64)
    r = _fro(a64 @ x64 - b.astype(np.float64)) / (_fro(a64) * _fro(x64))
    assert r <= _bound(n)
    assert lib.np_getrf(None, n, dpiv.ptr, dinfo.ptr) == -1   # NP_ERR_INVALID
    assert lib.np_inverse(da.ptr, n, None, C.byref(C.c_int())) == -1


# ---- the lazy binding ------------------------------------------------------------------------------------------------

def test_pending_chain_input():
    nd = _nd()
    n = 96
    g = _gauss(n, seed=11)
    eye = nd.identity(n).gpu()
    x = nd.exp(_gpu(g) * 0.25) * 0.1 + eye           # a pending chain when the lazy binding is on
    ref = x.cpu().numpy().astype(np.float64)           # computes it
    y = nd.exp(_gpu(g) * 0.25) * 0.1 + eye           # pending again
    inv = nd.inv(y).cpu().numpy().astype(np.float64)
    r = _fro(ref @ inv - np.eye(n)) / (_fro(ref) * _fro(inv))
    assert r <= _bound(n)
    z = nd.exp(_gpu(g) * 0.25) * 0.1 + eye
    got = nd.det(z)
    assert abs(got - np.linalg.det(ref)) <= n * EPS * abs(np.linalg.det(ref))


def test_whole_file_with_the_lazy_binding():
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, NP_LAZY_BINDING="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        str(Path(__file__)), "-k", "not whole_file and not large_single_rhs"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def test_with_hip_early_outs_compute_gpu_operands():
    """The text tools/apply_with_hip.py inserts into the reference's NDArray_Det / Inverse / LU / Solve, run as a program
    (linalg_bodies, built by build()): GPU operands never reach the reference's code, the known answers are exact, a
    singular matrix raises the reference's message, nothing leaks."""
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "linalg_bodies"
    r = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 calls reached the reference's own code, 0 failures" in r.stdout
