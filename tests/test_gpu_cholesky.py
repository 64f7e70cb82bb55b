"""The device Cholesky factorization (np_cholesky.hip: np_potrf / np_cholesky, NDArray.cholesky).

Exact tests.  L0 is lower triangular with strict-lower entries in -2 .. 2 and diagonal entries in {1, 2, 4}, A = L0 L0^T.
Every intermediate of any correct factorization order is an integer of magnitude <= 4 n + 16 < 2^24, every square root is
of a perfect square and every scaling is by a power of two (so a division and a multiplication by the reciprocal agree):
the fp32 factor is exactly L0 for LAPACK and for any correct device algorithm, in any order of summation
(tests/test_cholesky_reference_cpu.py holds numpy's LAPACK to that).  Results are compared with array_equal and info == 0.
For the same reason A itself may be formed by an fp32 product: each partial sum of a row of L0 against a row of L0 is an
integer below 2^24, so it equals the int64 product the small sizes are checked against.

Bound tests.  A = X X^T / n + I with X standard normal, symmetrised from its lower triangle;
r = ||A - L L^T||_1 / ||A||_1 in float64, eps = 2^-23.  r <= n eps / 4 floored at 2 eps (the convention of
tests/test_gpu_linalg.py::_bound) and, because that is loose here, r <= max(2 eps, 8 r_ref) with r_ref from numpy's fp32
linalg.cholesky on the same input: LAPACK sits at 0.31 - 0.57 eps on this family whatever n; the factor 8 is room for
another order of summation (64-wide panels, MFMA accumulation), a dropped update or a wrong diagonal block gives O(1)."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.cholesky_family import EPS, exact_case, residual, spd_case

pytestmark = pytest.mark.gpu

NOT_PD = "Error calculating the cholesky decomposition. (Is $a not positive definite?)"
NOT_SQUARE = "NDArray_Cholesky: $a must be a square matrix."
EXACT_SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000, 1024, 4096, 4097, 8193]
BOUND_SIZES = [1, 2, 3, 4, 7, 8, 31, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1024, 2047, 2048, 4096, 8192]


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _potrf(hip, A):
    """np_potrf on a copy of A on the device: (the buffer afterwards, info)"""
    _l, lib = _lib()
    n = A.shape[0]
    da, dinfo = hip.DeviceArray.from_host(A), hip.DeviceArray((1,))
    _l.check(lib.np_potrf(da.ptr, n, dinfo.ptr))
    out, info = da.to_host(), int(dinfo.to_host().view(np.int32)[0])
    da.free()
    dinfo.free()
    return out, info


def _cholesky(hip, A):
    """np_cholesky: (out, info, the input buffer afterwards)"""
    _l, lib = _lib()
    n = A.shape[0]
    da, dout = hip.DeviceArray.from_host(A), hip.DeviceArray((n, n))
    info = C.c_int(-1)
    _l.check(lib.np_cholesky(da.ptr, n, dout.ptr, C.byref(info)))
    out, a_after = dout.to_host(), da.to_host()
    da.free()
    dout.free()
    return out, info.value, a_after


def _check_exact_all_layers(hip, n, seed=None):
    L0, A = exact_case(n, seed)
    low = np.tril_indices(n)
    up = np.triu_indices(n, 1)
    got, info = _potrf(hip, A)
    assert info == 0
    assert np.array_equal(got[low], L0[low])
    assert np.array_equal(_bits(got[up]), _bits(A[up]))       # the caller's strict upper triangle, bit for bit
    del got
    out, info, a_after = _cholesky(hip, A)
    assert info == 0
    assert np.array_equal(out, L0)
    assert not np.signbit(out[up]).any()                         # +0.0f
    assert np.array_equal(_bits(a_after), _bits(A))
    del out, a_after
    assert np.array_equal(_nd().cholesky(_gpu(A)).cpu().numpy(), L0)


# ---- exact: the size ladder ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_ladder(hip, n):
    _check_exact_all_layers(hip, n)


@pytest.mark.parametrize("n", range(4, 63))
def test_exact_every_small_size(hip, n):
    L0, A = exact_case(n)
    out, info, _ = _cholesky(hip, A)
    assert info == 0 and np.array_equal(out, L0)


@pytest.mark.parametrize("n", [16384, 16385])
def test_exact_largest(hip, n):
    """np_potrf in place and np_cholesky, read back whole: 1 GiB each."""
    L0, A = exact_case(n)
    got, info = _potrf(hip, A)
    assert info == 0
    assert np.array_equal(np.tril(got), L0)
    assert np.array_equal(_bits(np.triu(got, 1)), _bits(np.triu(A, 1)))
    del got
    out, info, _ = _cholesky(hip, A)
    assert info == 0 and np.array_equal(out, L0)


def test_empty_and_null(hip):
    _l, lib = _lib()
    dinfo = hip.DeviceArray.from_host(np.array([7], np.int32).view(np.float32))
    d = hip.DeviceArray((1,))
    _l.check(lib.np_potrf(d.ptr, 0, dinfo.ptr))
    assert int(dinfo.to_host().view(np.int32)[0]) == 0
    info = C.c_int(7)
    _l.check(lib.np_cholesky(d.ptr, 0, d.ptr, C.byref(info)))
    assert info.value == 0
    assert lib.np_potrf(None, 4, dinfo.ptr) == -1 and lib.np_potrf(d.ptr, 4, None) == -1     # NP_ERR_INVALID
    assert lib.np_cholesky(None, 4, d.ptr, C.byref(info)) == -1 and lib.np_cholesky(d.ptr, 4, None, C.byref(info)) == -1
    assert lib.np_cholesky(d.ptr, 4, d.ptr, None) == -1
    assert lib.np_potrf(d.ptr, 65537, dinfo.ptr) == -1 and b"65536" in lib.np_last_error()
    assert lib.np_cholesky(d.ptr, 65537, d.ptr, C.byref(info)) == -1


# ---- exact: only the lower triangle is read -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 64, 65, 129, 700])
@pytest.mark.parametrize("junk", [np.nan, np.inf, 1e30])
def test_upper_triangle_is_ignored_and_kept(hip, n, junk):
    L0, A = exact_case(n)
    up = np.triu_indices(n, 1)
    low = np.tril_indices(n)
    B = A.copy()
    B[up] = junk
    got, info = _potrf(hip, B)
    assert info == 0
    assert np.array_equal(got[low], L0[low])
    assert np.array_equal(_bits(got[up]), _bits(B[up]))          # exactly what was put there
    out, info, b_after = _cholesky(hip, B)
    assert info == 0
    assert np.array_equal(_bits(out), _bits(L0))                 # +0.0f above the diagonal: the same bits as L0's zeros
    assert np.array_equal(_bits(b_after), _bits(B))
    assert np.array_equal(_bits(_nd().cholesky(_gpu(B)).cpu().numpy()), _bits(L0))


# ---- exact: info is the first failing column ------------------------------------------------------------------------

def _failing_columns(n):
    return sorted({j for j in (0, 1, 62, 63, 64, 65, 127, 128, n - 1) if j < n})


def _good_call_follows(hip, n=70):
    L0, A = exact_case(n, seed=5)
    out, info, _ = _cholesky(hip, A)
    assert info == 0 and np.array_equal(out, L0)
    hip.sync()                                                   # np_sync: no device error word raised


@pytest.mark.parametrize("n", [100, 129, 1100])
def test_info_is_the_first_failing_column(hip, n):
    L0, A = exact_case(n)
    for j in _failing_columns(n):
        for what, value in (("zero pivot", A[j, j] - L0[j, j] ** 2), ("negative pivot", A[j, j] - L0[j, j] ** 2 - 1),
                            ("NaN on the diagonal", np.nan)):
            B = A.copy()
            B[j, j] = value
            got, info = _potrf(hip, B)
            assert info == j + 1, (what, j, info)
            assert np.array_equal(np.tril(got)[:, :j], L0[:, :j]), (what, j)
            out, info, _ = _cholesky(hip, B)
            assert info == j + 1, (what, j, info)
            assert np.array_equal(out[:, :j], L0[:, :j]), (what, j)
    _good_call_follows(hip)


@pytest.mark.parametrize("n", [100, 129, 1100])
def test_info_with_nan_below_the_diagonal_and_two_failures(hip, n):
    L0, A = exact_case(n)
    cols = _failing_columns(n)
    for j in cols:
        for i in sorted({j + 1, min(j + 64, n - 1), n - 1}):
            if i <= j or i >= n:
                continue
            B = A.copy()
            B[i, j] = np.nan                                     # l_ij is NaN, so pivot i is: info == i + 1
            _, info = _potrf(hip, B)
            assert info == i + 1, (i, j, info)
            _, info, _ = _cholesky(hip, B)
            assert info == i + 1, (i, j, info)
    for j1, j2 in zip(cols, cols[1:]):
        B = A.copy()
        B[j2, j2] = -1.0
        B[j1, j1] = A[j1, j1] - L0[j1, j1] ** 2                  # the smaller index wins
        _, info = _potrf(hip, B)
        assert info == j1 + 1, (j1, j2, info)
    _good_call_follows(hip)


# ---- bit identity ---------------------------------------------------------------------------------------------------

def test_bit_identical_from_run_to_run(hip):
    A = spd_case(4097)
    runs = [_cholesky(hip, A)[0] for _ in range(2)]
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    g = _gpu(A)
    nd = _nd()
    assert np.array_equal(_bits(nd.cholesky(g).cpu().numpy()), _bits(nd.cholesky(g).cpu().numpy()))
    assert np.array_equal(_bits(_potrf(hip, A)[0]), _bits(_potrf(hip, A)[0]))


# ---- views and the lazy binding -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 300])
def test_views_and_a_pending_chain(n):
    nd = _nd()
    L0, A = exact_case(n)
    assert np.array_equal(nd.cholesky(nd.transpose(_gpu(A))).cpu().numpy(), L0)       # a transposed view of a symmetric matrix
    k = 7
    big = np.full((n + 2 * k, n + 2 * k), 3.0, np.float32)
    big[k:k + n, k:k + n] = A
    window = _gpu(big).slice([k, k + n], [k, k + n])                                   # [k:k+n, k:k+n] of a larger array
    assert np.array_equal(nd.cholesky(window).cpu().numpy(), L0)
    ga = _gpu(A)
    assert np.array_equal(nd.cholesky((ga + ga) * 0.5).cpu().numpy(), L0)              # pending when the lazy binding is on


def test_views_and_a_pending_chain_with_the_lazy_binding():
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, NP_LAZY_BINDING="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", str(Path(__file__)),
                        "-k", "test_views_and_a_pending_chain and not lazy_binding or test_errors"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


# ---- errors -----------------------------------------------------------------------------------------------------------

def test_errors_through_the_method():
    nd = _nd()
    L0, A = exact_case(90)
    bad = A.copy()
    bad[70, 70] = -1.0
    operands = [(_gpu([1.0, 2.0, 3.0]), NOT_SQUARE), (_gpu(np.ones((2, 3), np.float32)), NOT_SQUARE), (_gpu(bad), NOT_PD),
                (_gpu([[1.0, 2.0], [2.0, 1.0]]), NOT_PD)]
    for g, message in operands:
        before = nd.live_device_allocations()
        with pytest.raises(Exception) as e:
            nd.cholesky(g)
        assert str(e.value) == message
        assert nd.live_device_allocations() == before
        g.cpu().numpy()                                            # the operand is still usable
    assert np.array_equal(nd.cholesky(_gpu(A)).cpu().numpy(), L0)


# ---- bounds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BOUND_SIZES)
def test_residual_bounds(hip, n):
    A = spd_case(n)
    L = _nd().cholesky(_gpu(A)).cpu().numpy()
    assert np.array_equal(L, np.tril(L)) and (np.diagonal(L) > 0).all()
    r = residual(A, L)
    r_ref = residual(A, np.linalg.cholesky(A))
    print("cholesky n = %d: r / eps = %.3f, numpy fp32 r_ref / eps = %.3f, r / (n eps) = %.2e" % (n, r / EPS, r_ref / EPS, r / (n * EPS)))
    assert r <= max(n * EPS / 4, 2 * EPS), r / EPS
    assert r <= max(2 * EPS, 8 * r_ref), (r / EPS, r_ref / EPS)
    if n in (65, 1000):                                           # np_potrf gives the same factor
        got, info = _potrf(hip, A)
        assert info == 0 and np.array_equal(_bits(np.tril(got)), _bits(L))


# ---- the --with-hip early-out ------------------------------------------------------------------------------------------

def test_with_hip_early_out_computes_gpu_operands():
    """The text tools/apply_with_hip.py inserts into the reference's NDArray_Cholesky, run as a program (cholesky_bodies, built
    by build()): GPU operands never reach the reference's code, the known answer is exact, both throws carry the
    reference's messages, nothing leaks."""
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "cholesky_bodies"
    r = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 calls reached the reference's own code, 0 failures" in r.stdout
