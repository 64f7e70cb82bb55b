"""The device LU (np_lu.hip) on exact-arithmetic inputs: element-for-element against the expected factors.

Every input is a tests/linalg_exact.py construction M = Q L U whose exactness certificate holds, so fp32 partial pivoting
must return exactly its pivots, info, L and U whatever the order of summation, and a solve with an integer x must return
x.  Factors, solutions and inverses are compared with == (so -0.0 == 0.0), det by its fp32 bits.  det and inv factor the
buffer as LAPACK sees it (a^T), solve and lu factor a (host/numpower_linalg.cpp): det / inv get a = M^T.

Above a few thousand the inputs are built from coordinates straight into device buffers and the results are read back in
row blocks: count_nonzero plus the values at the expected coordinates, no dense host copy of the whole matrix."""
import gc
import resource

import numpy as np
import pytest

from tests import linalg_exact as le

pytestmark = pytest.mark.gpu

LADDER = [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 131, 132, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025,
          2047, 2048, 2049, 3073, 4095, 4097, 8193]
SINGULAR = "LU factorization failed. Unable to compute the matrix inverse.\n"
CHUNK_BYTES = 256 << 20
SMALL_LDS_FLOATS = 156 * 1024 // 4   # np_linalg_common.h kSmallLdsFloats: the n <= 128 path's LDS budget


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


def _host(x):
    return x.cpu().numpy()


def _xvec(n, k, seed):
    """integer right-hand-side solutions in -4 .. 4"""
    return np.random.default_rng(seed).integers(-4, 5, (n, k)).astype(np.float64)


def _eq(got, want):
    got = np.asarray(got)
    assert got.shape == np.shape(want)
    bad = np.nonzero(got != want)
    assert len(bad[0]) == 0, ("%d entries differ, first at %s: got %r, want %r"
                              % (len(bad[0]), [int(b[0]) for b in bad], got[tuple(b[0] for b in bad)],
                                 np.asarray(want)[tuple(b[0] for b in bad)]))


# ---- the C ABI on dense inputs -----------------------------------------------------------------------------------

def _getrf(hip, M):
    """np_getrf on M (its column-major buffer): (packed L\\U row-major, ipiv, info, the device buffers)"""
    _l, lib = _lib()
    n = M.shape[0]
    da = hip.DeviceArray.from_host(np.ascontiguousarray(M.T, np.float32))
    dpiv, dinfo = hip.DeviceArray((n,)), hip.DeviceArray((1,))
    _l.check(lib.np_getrf(da.ptr, n, dpiv.ptr, dinfo.ptr))
    return da.to_host().T, dpiv.to_host().view(np.int32).astype(np.int64), int(dinfo.to_host().view(np.int32)[0]), (da, dpiv)


def _getrs(hip, da, dpiv, n, B):
    """np_getrs against the factored buffer: X for B (n x k, row-major in and out)"""
    _l, lib = _lib()
    db = hip.DeviceArray.from_host(np.ascontiguousarray(B.T, np.float32))
    _l.check(lib.np_getrs(da.ptr, dpiv.ptr, n, B.shape[1], db.ptr))
    return db.to_host().T


def _check_getrf(hip, case, M32, x=None):
    lu, piv, info, (da, dpiv) = _getrf(hip, M32)
    _eq(piv, case.ipiv)
    assert info == case.info
    _eq(lu, case.packed())
    if x is not None:
        _eq(_getrs(hip, da, dpiv, case.n, (case.dense_M() @ x).astype(np.float32)), x)
    da.free()
    dpiv.free()


# ---- the size ladder ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LADDER)
def test_ladder(hip, n):
    nd = _nd()
    case = le.generic(n, seed=n, parity=n % 2)
    x = _xvec(n, 3, n)
    case.certify(x)
    M = case.dense_M()
    M32 = M.astype(np.float32)
    _check_getrf(hip, case, M32, x)
    # lu factors a = M: P M = L U
    p, l, u = (_host(t) for t in nd.lu(_gpu(M32)))
    _eq(p, case.P())
    _eq(l, case.L())
    _eq(u, case.U())
    # solve factors a = M
    ga = _gpu(M32)
    b = (M @ x).astype(np.float32)
    _eq(_host(nd.solve(ga, _gpu(b))), x)
    _eq(_host(nd.solve(ga, _gpu(b[:, :1]))), x[:, :1])
    # det factors a^T
    d = np.float32(nd.det(_gpu(M32.T)))
    assert d.view(np.uint32) == case.det().view(np.uint32), (d, case.det())
    # inv factors a^T: inv(M^T) = (M^-1)^T
    ci, inv = le.exact_inverse(n, seed=n + 1)
    ci.certify(inv)
    _eq(_host(nd.inv(_gpu(ci.dense_M().T.astype(np.float32)))), inv.T)


# ---- ties --------------------------------------------------------------------------------------------------------

TIE_CASES = [
    # (n, [(step, rows after the designed pivot row)]): within a wave (1, 2, 31), across waves (64), across a
    # thread's register slots (1024); at leaf boundaries (15, 16) and panel boundaries (63, 64, 127, 128)
    (40, [(0, 1), (1, 31), (15, 2), (16, 1), (30, 5)]),
    (100, [(0, 64), (1, 1), (15, 64), (16, 2), (33, 64), (63, 1), (64, 1)]),
    (128, [(0, 64), (15, 1), (16, 64), (63, 64), (64, 1), (126, 1)]),
    (300, [(0, 1), (0, 64), (15, 64), (16, 1), (63, 64), (64, 64), (65, 1), (127, 1), (128, 64), (200, 64), (298, 1)]),
    (1100, [(0, 1024), (1, 64), (15, 1024), (16, 1), (63, 1024), (64, 1), (70, 64), (127, 64), (128, 1)]),
    (2049, [(0, 1024), (16, 1024), (64, 1024), (128, 1024), (700, 1024), (1000, 64), (2000, 1)]),
    (4097, [(0, 1024), (1, 2048), (2, 3072), (1024, 1024), (3000, 1024), (4000, 64)]),
]


@pytest.mark.parametrize("n,ties", TIE_CASES, ids=[str(c[0]) for c in TIE_CASES])
def test_ties_go_to_the_first_row(hip, n, ties):
    case = le.generic(n, seed=100 + n, ties=ties)
    x = _xvec(n, 2, n)
    case.certify(x)
    M = case.dense_M()
    if n <= 1100:   # the host reference agrees with the construction
        lu, piv, info = le.getf2_ref(M)
        assert (piv == case.ipiv).all() and info == 0 and (lu == case.packed()).all()
    _check_getrf(hip, case, M.astype(np.float32), x)
    p, l, u = (_host(t) for t in _nd().lu(_gpu(M.astype(np.float32))))
    _eq(p, case.P())
    _eq(l, case.L())


@pytest.mark.parametrize("n", [2, 3, 4, 16, 17, 33, 63, 64, 65, 100, 127, 128])
def test_wilkinson_never_exchanges(hip, n):
    case = le.wilkinson(n)
    M = case.dense_M()
    le.certify_stepwise(M)
    M32 = M.astype(np.float32)
    _check_getrf(hip, case, M32)
    p, l, u = (_host(t) for t in _nd().lu(_gpu(M32)))
    _eq(p, np.eye(n))
    _eq(l, case.L())
    _eq(u, case.U())
    d = np.float32(_nd().det(_gpu(M32.T)))
    assert d.view(np.uint32) == np.float32(2.0 ** (n - 1)).view(np.uint32)


@pytest.mark.parametrize("n", [129, 1025])
def test_banded_wilkinson_never_exchanges(hip, n):
    case = le.banded_wilkinson(n, n - 1)
    x = _xvec(n, 2, n)
    case.certify(x)
    M = case.dense_M()
    _check_getrf(hip, case, M.astype(np.float32), x)
    assert (case.ipiv == np.arange(n)).all()


# ---- zero pivots -------------------------------------------------------------------------------------------------

ZERO_CASES = sorted({(n, k) for n in (20, 100, 128, 300, 1100) for k in (0, 1, 15, 16, 63, 64, 65, 127, n - 1) if k < n})


@pytest.mark.parametrize("n,k", ZERO_CASES)
def test_zero_pivot(hip, n, k):
    nd = _nd()
    case = le.generic(n, seed=7 * n + k, zero_pivots=[k])
    case.certify()
    M32 = case.dense_M().astype(np.float32)
    _check_getrf(hip, case, M32)
    assert case.info == k + 1
    # det and inv factor a^T, solve factors a: each is given the matrix that makes it factor M
    gt, ga, gb = _gpu(M32.T), _gpu(M32), _gpu(np.ones((n, 2), np.float32))
    d = np.float32(nd.det(gt))
    assert d.view(np.uint32) == 0
    gc.collect()   # arrays of earlier tests held in reference cycles (tracebacks) are freed now, not mid-count
    before = nd.live_device_allocations()
    for call in (lambda: nd.inv(gt), lambda: nd.solve(ga, gb)):
        with pytest.raises(Exception) as e:
            call()
        assert str(e.value) == SINGULAR
        del e
    gc.collect()
    assert nd.live_device_allocations() == before


@pytest.mark.parametrize("n,zeros", [(50, [10, 3]), (200, [150, 64]), (1100, [1099, 700, 65])])
def test_two_zero_pivots_report_the_first(hip, n, zeros):
    case = le.generic(n, seed=n, zero_pivots=zeros)
    case.certify()
    assert case.info == min(zeros) + 1
    _check_getrf(hip, case, case.dense_M().astype(np.float32))


# ---- det ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [129, 257, 1025, 2049, 4097])
@pytest.mark.parametrize("parity", [0, 1])
def test_det_sign_with_many_exchanges(hip, n, parity):
    case = le.generic(n, seed=3 * n + parity, parity=parity, swap_prob=0.9)
    case.certify()
    assert np.count_nonzero(case.ipiv != np.arange(n)) > n // 2
    d = np.float32(_nd().det(_gpu(case.dense_M().T.astype(np.float32))))
    assert d.view(np.uint32) == case.det().view(np.uint32), (d, case.det())


def _scaled(n, at, values, seed):
    diag = np.ones(n)
    diag[list(at)] = values
    case = le.generic(n, seed=seed, u_offdiag=False, diag=diag)
    case.certify()
    return case


BIG, SMALL = 2.0 ** 100, 2.0 ** -100
ORDERS = {"overflow": [BIG, BIG, SMALL, SMALL], "underflow": [SMALL, SMALL, BIG, BIG],
          "neg_overflow": [BIG, -BIG, SMALL, SMALL], "neg_underflow": [-SMALL, SMALL, BIG, BIG],
          "balanced": [BIG, SMALL, BIG, SMALL]}


@pytest.mark.parametrize("n,at", [(4, (0, 1, 2, 3)), (100, (10, 40, 70, 99)), (128, (0, 63, 64, 127)),
                                  (300, (1, 64, 128, 299)), (2100, (1022, 1023, 1024, 2047))])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_det_overflow_and_underflow_follow_the_fp32_loop(hip, n, at, order):
    case = _scaled(n, at, ORDERS[order], seed=n + len(order))
    want = case.det()
    d = np.float32(_nd().det(_gpu(case.dense_M().T.astype(np.float32))))
    assert d.view(np.uint32) == want.view(np.uint32), (d, want)
    if order in ("overflow", "underflow", "balanced"):
        assert abs(np.linalg.det(np.diag(ORDERS[order]))) == 1.0   # what the order-free product would say


# ---- right-hand-side counts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,nrhs", [(128, 182), (128, 183), (128, 364), (128, 365), (64, 559), (1, 39934),
                                    (129, 127), (129, 128), (129, 129), (129, 65535), (129, 65543)])
def test_many_right_hand_sides(hip, n, nrhs):
    nd = _nd()
    case = le.generic(n, seed=n + nrhs)
    x = _xvec(n, nrhs, nrhs)
    case.certify(x)
    M = case.dense_M()
    M32 = M.astype(np.float32)
    b = (M @ x).astype(np.float32)
    ga = _gpu(M32)
    got = _host(nd.solve(ga, _gpu(b)))
    _eq(got, x)
    cols = {0, 1, nrhs // 2, nrhs - 1}
    if n <= 128:   # lu_small_kernel's passes through LDS: cw columns each, both sides of every pass boundary
        cw = (SMALL_LDS_FLOATS - n * n - 2 * n) // n
        cols |= {c for p in range(cw, nrhs, cw) for c in (p - 1, p)}
    for c in sorted(cols):                                # a column alone gives the same bits
        one = _host(nd.solve(ga, _gpu(b[:, c:c + 1])))
        assert (_bits(one[:, 0]) == _bits(got[:, c])).all(), c
    if n > 1:
        lu, piv, info, (da, dpiv) = _getrf(hip, M32)
        _eq(_getrs(hip, da, dpiv, n, b), x)


# ---- views of b --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 300])
def test_b_views_give_the_bits_of_their_contiguous_copy(n):
    nd = _nd()
    case = le.generic(n, seed=n)
    x = _xvec(n, 4, n)
    case.certify(x)
    M = case.dense_M()
    ga = _gpu(M.astype(np.float32))
    b = (M @ x).astype(np.float32)
    want = _host(nd.solve(ga, _gpu(b)))
    _eq(want, x)
    bt = nd.transpose(_gpu(np.ascontiguousarray(b.T)))                # a transposed view
    assert (_bits(_host(nd.solve(ga, bt))) == _bits(want)).all()
    big = np.zeros((n + 3, 11), np.float32)
    big[2:n + 2, 3:7] = b
    sl = _gpu(big).slice([2, n + 2], [3, 7])                        # a strided window
    assert (_bits(_host(nd.solve(ga, sl))) == _bits(want)).all()


# ---- large sizes: panels and permutation paths that no other test reaches ---------------------------------------

def _rows_per_chunk(n):
    return max(1, CHUNK_BYTES // (4 * n))


def _fill(ptr, n, rows, cols, vals):
    """the row-major n x n device buffer at ptr := zeros with buf[rows, cols] = vals, one block of rows at a time"""
    _l, lib = _lib()
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order].astype(np.float32)
    step = _rows_per_chunk(n)
    cuts = np.searchsorted(rows, np.arange(0, n + step, step))
    for i, r0 in enumerate(range(0, n, step)):
        r1 = min(n, r0 + step)
        blk = np.zeros((r1 - r0, n), np.float32)
        s, e = cuts[i], cuts[i + 1]
        blk[rows[s:e] - r0, cols[s:e]] = vals[s:e]
        _l.check(lib.np_memcpy_h2d(ptr + 4 * r0 * n, blk.ctypes.data, blk.nbytes))


def _compare(ptr, n, rows, cols, vals):
    """the row-major n x n device buffer at ptr holds exactly vals at (rows, cols) and zeros (of either sign) elsewhere"""
    _l, lib = _lib()
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    step = _rows_per_chunk(n)
    cuts = np.searchsorted(rows, np.arange(0, n + step, step))
    for i, r0 in enumerate(range(0, n, step)):
        r1 = min(n, r0 + step)
        blk = np.empty((r1 - r0, n), np.float32)
        _l.check(lib.np_memcpy_d2h(blk.ctypes.data, ptr + 4 * r0 * n, blk.nbytes))
        s, e = cuts[i], cuts[i + 1]
        got = blk[rows[s:e] - r0, cols[s:e]]
        _eq(got, vals[s:e])
        assert np.count_nonzero(blk) == e - s, ("nonzeros where zeros belong in rows", r0, r1)


def _peak_host_gib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20


@pytest.mark.parametrize("n", le.LARGE_GETRF)
def test_large_getrf_getrs(hip, n):
    """8193: panel R = 16; 16384: perm_kernel with exactly 64 KiB of LDS; 16385: R = 32 down to 1 and perm_kernel's
    global-memory branch; 32769: R = 64, W = 1; 46341: n^2 > 2^31, an LU beyond 2^31 elements"""
    _l, lib = _lib()
    case = le.large_getrf_case(n)       # its reach into every trailing tile: test_linalg_reference_cpu.py
    assert case.ipiv[0] != 0
    x = _xvec(n, 2, n)
    case.certify(x)
    r, c, v = case.M_coords()
    da = hip.DeviceArray((n, n))
    _fill(da.ptr, n, c, r, v)                 # column-major M: buffer row c = column c
    dpiv, dinfo = hip.DeviceArray((n,)), hip.DeviceArray((1,))
    _l.check(lib.np_getrf(da.ptr, n, dpiv.ptr, dinfo.ptr))
    _eq(dpiv.to_host().view(np.int32).astype(np.int64), case.ipiv)
    assert int(dinfo.to_host().view(np.int32)[0]) == 0
    pr, pc, pv = case.packed_coords()
    _compare(da.ptr, n, pc, pr, pv)
    b = case.matvec(x).astype(np.float32)
    _eq(_getrs(hip, da, dpiv, n, b), x)
    for d in (da, dpiv, dinfo):
        d.free()
    print("n = %d: peak host RSS %.2f GiB, device %.2f GiB for the matrix" % (n, _peak_host_gib(), 4 * n * n / 2 ** 30))


def _nd_from_coords(n, rows, cols, vals):
    """a GPU NDArray n x n (row-major) with these entries, built on the device block by block"""
    nd = _nd()
    from numpower_amd.ndarray import GPU
    g = nd.zeros([n, n], GPU)
    _fill(g._p.contents.data, n, rows, cols, vals)
    return g


@pytest.mark.parametrize("n", le.LARGE_ND)
def test_large_nd_entry_points(n):
    nd = _nd()
    case = le.large_nd_case(n)
    assert case.ipiv[0] != 0
    x = _xvec(n, 3, n)
    case.certify(x)
    r, c, v = case.M_coords()
    ga = _nd_from_coords(n, r, c, v)
    b = case.matvec(x).astype(np.float32)
    _eq(_host(nd.solve(ga, _gpu(b))), x)
    p, l, u = nd.lu(ga)
    _compare(p._p.contents.data, n, np.arange(n), case.perm, np.ones(n))
    _compare(l._p.contents.data, n, np.concatenate([np.arange(n), case.Lr]), np.concatenate([np.arange(n), case.Lc]),
             np.concatenate([np.ones(n), case.Lv]))
    _compare(u._p.contents.data, n, case.Ur, case.Uc, case.Uv)
    del p, l, u
    gt = _nd_from_coords(n, c, r, v)          # det factors a^T: a = M^T
    d = np.float32(nd.det(gt))
    assert d.view(np.uint32) == case.det().view(np.uint32), (d, case.det())
    del ga, gt
    # inv factors a^T: given a = M^T it returns (M^-1)^T, compared block by block with M^-1's coordinates transposed
    ci, (ir, ic, iv) = le.large_inverse_case(n)
    assert ci.ipiv[0] != 0
    ci.certify(x_coords=(ir, ic, iv))
    r, c, v = ci.M_coords()
    gi = nd.inv(_nd_from_coords(n, c, r, v))
    _compare(gi._p.contents.data, n, ic, ir, iv)


def test_solve_one_rhs_beyond_2_31_elements():
    n = le.LARGE_SOLVE
    nd = _nd()
    case = le.large_solve_case()
    assert case.ipiv[0] != 0
    x = _xvec(n, 1, 5)
    case.certify(x)
    r, c, v = case.M_coords()
    ga = _nd_from_coords(n, r, c, v)
    b = case.matvec(x).astype(np.float32)
    _eq(_host(nd.solve(ga, _gpu(b))), x)
    print("n = %d solve: peak host RSS %.2f GiB" % (n, _peak_host_gib()))
