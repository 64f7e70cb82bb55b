"""The device Householder QR (np_qr.hip: np_geqrf / np_qr / np_lstsq; NDArray.qr, NDArray.lstsq).

Exact tests.  A = S P [R0; 0] (tests/qr_family.py): every reflector is an exchange of two rows or the identity, so Q, R and x are
compared with == against numpy.linalg.qr (which LAPACK's sgeqrf / sorgqr and the fp32 emulator reproduce bit for bit on this
family, tests/test_qr_reference_cpu.py) through np_qr, np_geqrf, NDArray.qr and qr_bodies.

Bound tests.  res, colres, orth, xerr (qr_family.metrics; float64 arithmetic on the fp32 results):
  up to 513 x 257   metric <= 4 x the same metric of the fp32 emulator of the blocked algorithm on the same matrix; the factor 4 is
                    room for another summation order in the GEMMs, a dropped reflector or a wrong T gives O(1)
  2048 x 2048, 4096 x 512, 16384 x 128   res and orth <= 4 x qr_family.RECORDED_GROWTH x sqrt(n) eps, the emulator's growth
                    recorded in profiles/linalg/qr_accuracy.log
Each bound case prints its figures before it asserts."""
import ctypes as C
import functools
import gc
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import qr_family as F

pytestmark = pytest.mark.gpu
EPS = F.EPS
BOUND_SHAPES = [(64, 64), (65, 64), (129, 65), (200, 130), (513, 257)]
LARGE_SHAPES = [(2048, 2048), (4096, 512), (16384, 128)]


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _qr(hip, a):
    """np_qr: (q, r, the input buffer afterwards)"""
    _l, lib = _lib()
    m, n = a.shape
    da, dq, dr = hip.DeviceArray.from_host(a), hip.DeviceArray((m, n)), hip.DeviceArray((n, n))
    _l.check(lib.np_qr(da.ptr, m, n, dq.ptr, dr.ptr))
    out = dq.to_host(), dr.to_host(), da.to_host()
    for d in (da, dq, dr):
        d.free()
    return out


def _geqrf(hip, a):
    """np_geqrf: (the packed factor, tau)"""
    _l, lib = _lib()
    m, n = a.shape
    da, dt = hip.DeviceArray.from_host(a), hip.DeviceArray((n,))
    _l.check(lib.np_geqrf(da.ptr, m, n, dt.ptr))
    out = da.to_host(), dt.to_host()
    da.free()
    dt.free()
    return out


def _lstsq(hip, a, b, fill=-77.0):
    """np_lstsq into an x prefilled with `fill`: (x, info, a and b afterwards)"""
    _l, lib = _lib()
    (m, n), nrhs = a.shape, b.shape[1]
    da, db = hip.DeviceArray.from_host(a), hip.DeviceArray.from_host(b)
    dx = hip.DeviceArray.from_host(np.full((n, nrhs), fill, np.float32))
    info = C.c_int(-1)
    _l.check(lib.np_lstsq(da.ptr, db.ptr, m, n, nrhs, dx.ptr, C.byref(info)))
    out = dx.to_host(), info.value, da.to_host(), db.to_host()
    for d in (da, db, dx):
        d.free()
    return out


def _nd_qr(a):
    q, r = _nd().qr(a if not isinstance(a, np.ndarray) else _gpu(a))
    return q.cpu().numpy(), r.cpu().numpy()


def _nd_lstsq(a, b):
    x = _nd().lstsq(a if not isinstance(a, np.ndarray) else _gpu(a), b if not isinstance(b, np.ndarray) else _gpu(b))
    return x.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _exact(m, n):
    a, r0 = F.exact_family(m, n)
    q, r = np.linalg.qr(a)
    for x in (a, r0, q, r):
        x.setflags(write=False)
    return a, r0, q, r


@functools.lru_cache(maxsize=None)
def _emulated(family, m, n):
    a = getattr(F, family)(m, n)
    a.setflags(write=False)
    return a, F.metrics(a, *F.qr_emulated(a))


# ---- exact ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", F.EXACT_SHAPES)
def test_exact_family_through_every_layer(hip, m, n):
    a, r0, want_q, want_r = _exact(m, n)
    q, r, after = _qr(hip, a)
    assert _same(after, a)
    assert np.array_equal(q, want_q) and np.array_equal(r, want_r)
    assert set(np.unique(q)) <= {-1.0, 0.0, 1.0}
    q64 = q.astype(np.float64)
    assert np.array_equal(q64.T @ q64, np.eye(n)) and np.array_equal(q64 @ r.astype(np.float64), a.astype(np.float64))
    assert np.array_equal(np.abs(r), np.abs(r0))
    assert not _bits(r)[np.tril_indices(n, -1)].any()           # +0.0f by bit pattern
    packed, tau = _geqrf(hip, a)
    upper = np.triu_indices(n)
    assert np.array_equal(_bits(packed[:n])[upper], _bits(r)[upper])
    assert set(np.unique(tau)) <= {0.0, 1.0}
    qf, rf = _nd_qr(a)
    assert _same(qf, q) and _same(rf, r)


def test_qr_bodies_gpu_operands_never_reach_the_reference_code(hip):
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "qr_bodies"
    proc = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "qr_bodies gpu: 0 calls reached the reference's own code, 0 failures" in proc.stdout


@pytest.mark.parametrize("m,n", [(129, 65), (200, 130)])
def test_scaling_by_a_power_of_two_scales_r_and_leaves_q(hip, m, n):
    """fails with the squares of the column norm in fp32: (2^62)^2 overflows, (2^-62)^2 flushes"""
    a = F.gaussian(m, n)
    q, r, _ = _qr(hip, a)
    assert np.isfinite(q).all() and np.isfinite(r).all()
    for e in (62, -62):
        qs, rs, _ = _qr(hip, np.ldexp(a, e))
        assert _same(qs, q) and _same(rs, np.ldexp(r, e))


def test_zero_columns_the_zero_matrix_and_diagonal_matrices(hip):
    m, n, j = 100, 70, 35
    a = F.gaussian(m, n).copy()
    a[:, j] = 0.0
    packed, tau = _geqrf(hip, a)
    assert tau[j] == 0.0 and packed[j, j] == 0.0 and not packed[:, j].any()
    assert np.all(tau[:j] != 0) and np.all(tau[j + 1:] != 0)
    q, r, _ = _qr(hip, a)
    ref = F.metrics(a, *F.qr_emulated(a))
    got = F.metrics(a, q, r)
    assert r[j, j] == 0.0 and got["orth"] <= 4 * ref["orth"] and got["res"] <= 4 * ref["res"]
    for mm, nn in ((5, 3), (130, 65)):
        q, r, _ = _qr(hip, np.zeros((mm, nn), np.float32))
        assert not _bits(r).any() and _same(q, np.eye(mm, nn, dtype=np.float32))
        assert not _geqrf(hip, np.zeros((mm, nn), np.float32))[1].any()
        d = np.zeros((mm, nn), np.float32)
        d[np.arange(nn), np.arange(nn)] = np.where(np.arange(nn) % 3 == 0, -1.0, 1.0) * (1.0 + np.arange(nn))
        for mat in (np.eye(mm, nn, dtype=np.float32), d):
            q, r, _ = _qr(hip, mat)
            packed, tau = _geqrf(hip, mat)
            assert not tau.any() and _same(packed, mat)
            assert _same(r, mat[:nn]) and _same(q, np.eye(mm, nn, dtype=np.float32))


# ---- least squares ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", F.EXACT_SHAPES)
def test_lstsq_returns_x0_bit_for_bit(hip, m, n):
    a, _ = F.exact_family(m, n, pow2_diag=True)
    for nrhs in (1, 3, 65, 257):
        b, x0 = F.exact_rhs(a, nrhs)
        x, info, a_after, b_after = _lstsq(hip, a, b)
        assert info == 0 and _same(a_after, a) and _same(b_after, b)
        assert np.array_equal(x, x0), nrhs
    b, x0 = F.exact_rhs(a, 3)
    assert np.array_equal(_nd_lstsq(a, b), x0)


def test_lstsq_info_and_errors(hip):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    nd = _nd()
    m, n = 70, 66
    a, _ = F.exact_family(m, n, pow2_diag=True)
    b, _ = F.exact_rhs(a, 2)
    live = lib.np_live_allocs()
    for j in (0, 63, 64, n - 1):
        low = a.copy()
        low[:, j] = 0.0
        x, info, _, _ = _lstsq(hip, low, b)
        assert info == j + 1 and np.all(x == -77.0)
        with pytest.raises(Error) as e:
            nd.lstsq(_gpu(low), _gpu(b))
        assert str(e.value) == "The diagonal element %d of the triangular factor of $a is zero, so that $a does not have full rank." % (j + 1)
        del e                # its traceback holds the frame of NDArray.lstsq, and with it the two operands of the refused call
    gc.collect()
    assert lib.np_live_allocs() == live
    shape = "Invalid dimensions to calculate lstsq, both arrays must have 2 dimensions and $b must contain the same amount of rows as $a"
    ones = lambda *s: _gpu(np.ones(s, np.float32))
    for x, y, msg in ((ones(3), ones(3, 1), shape), (ones(3, 2), ones(3), shape), (ones(3, 2), ones(4, 1), shape),
                      (ones(2, 3), ones(2, 1), "m >= n"), (ones(3, 2), nd.array(np.ones((3, 1), np.float32)), "same device")):
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            nd.lstsq(x, y)
        assert (str(e.value) == msg) if msg is shape else (msg in str(e.value))
        assert nd.live_device_allocations() == before
    for x, msg in ((ones(3), "two-dimensional"), (ones(2, 2, 2), "two-dimensional"), (ones(2, 3), "m >= n")):
        before = nd.live_device_allocations()
        with pytest.raises(Error, match=msg):
            nd.qr(x)
        assert nd.live_device_allocations() == before


# ---- accuracy ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", BOUND_SHAPES)
@pytest.mark.parametrize("family,keys", [("gaussian", ("res", "colres", "orth")), ("graded", ("colres", "orth")),
                                         ("rank_deficient", ("res", "orth"))])
def test_accuracy_against_the_emulator(hip, family, keys, m, n):
    a, ref = _emulated(family, m, n)
    q, r, _ = _qr(hip, a)
    got = F.metrics(a, q, r)
    print("\n%s %d x %d: " % (family, m, n) + "  ".join("%s %.3g (emulator %.3g)" % (k, got[k], ref[k]) for k in keys), flush=True)
    assert not np.tril(r, -1).any()
    for k in keys:
        assert got[k] <= 4 * ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("m,n", LARGE_SHAPES)
def test_accuracy_at_the_large_sizes(hip, m, n):
    a = F.gaussian(m, n)
    q, r, _ = _qr(hip, a)
    got = F.growth(a, q, r)
    print("\ngaussian %d x %d: res %.3f orth %.3f sqrt(n) eps (bound %.2f, %.2f)"
          % (m, n, got["res"], got["orth"], 4 * F.RECORDED_GROWTH["res"], 4 * F.RECORDED_GROWTH["orth"]), flush=True)
    for k in ("res", "orth"):
        assert got[k] <= 4 * F.RECORDED_GROWTH[k], (k, got[k])


@pytest.mark.parametrize("m,n,nrhs", [(128, 64, 1), (200, 100, 3), (513, 130, 65), (1024, 257, 2)])
def test_lstsq_accuracy_against_the_emulator(hip, m, n, nrhs):
    a, b = F.gaussian(m, n), F.gaussian(m, nrhs, 9)
    x, info, _, _ = _lstsq(hip, a, b)
    xe, _ = F.lstsq_emulated(a, b)
    got, ref = F.xerr(a, b, x), F.xerr(a, b, xe)
    print("\nlstsq %d x %d, nrhs %d: xerr %.3g (emulator %.3g)" % (m, n, nrhs, got, ref), flush=True)
    assert info == 0 and got <= 4 * ref


# ---- the remaining cases ----------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_identical(hip):
    a, b = F.gaussian(513, 257), F.gaussian(513, 5, 9)
    first, again = _qr(hip, a), _qr(hip, a)
    assert _same(first[0], again[0]) and _same(first[1], again[1])
    assert _same(_lstsq(hip, a, b)[0], _lstsq(hip, a, b)[0])
    p1, p2 = _geqrf(hip, a), _geqrf(hip, a)
    assert _same(p1[0], p2[0]) and _same(p1[1], p2[1])


def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    m, n = 90, 70
    a, b = F.gaussian(m, n), F.gaussian(m, 3, 9)
    q, r, _ = _qr(hip, a)
    x = _lstsq(hip, a, b)[0]
    qt, rt = _nd_qr(nd.transpose(_gpu(np.ascontiguousarray(a.T))))           # a strided view
    assert _same(qt, q) and _same(rt, r)
    big = np.full((m + 3, n + 5), 9.0, np.float32)
    big[1:1 + m, 2:2 + n] = a
    sliced = _gpu(big).slice([1, 1 + m], [2, 2 + n])                         # a strided slice
    qs, rs = _nd_qr(sliced)
    assert _same(qs, q) and _same(rs, r)
    assert _same(_nd_lstsq(sliced, nd.transpose(_gpu(np.ascontiguousarray(b.T)))), x)
    nd.set_lazy_binding(True)
    try:
        chain = (_gpu(a) * 2.0) * 0.5                                         # pending until a consumer needs it
        ql, rl = _nd_qr(chain)
        assert _same(ql, q) and _same(rl, r)
        assert _same(_nd_lstsq((_gpu(a) * 2.0) * 0.5, (_gpu(b) * 4.0) * 0.25), x)
    finally:
        nd.set_lazy_binding(False)


def test_non_finite_input_returns(hip):
    a = F.gaussian(130, 70).copy()
    b = F.gaussian(130, 2, 9)
    for bad in (np.nan, np.inf, -np.inf):
        c = a.copy()
        c[40, 20] = bad
        q, r, _ = _qr(hip, c)
        assert not np.isfinite(r).all() or not np.isfinite(q).all()
        assert not _bits(r)[np.tril_indices(70, -1)].any()
        x, info, _, _ = _lstsq(hip, c, b)
        assert info == 0 and not np.isfinite(x).all()


def test_refusals_leave_the_outputs_untouched_and_nothing_leaks(hip):
    _l, lib = _lib()
    nd = _nd()
    d = hip.DeviceArray.from_host(np.full(64, 5.0, np.float32))
    info = C.c_int(-3)
    live = lib.np_live_allocs()
    assert lib.np_qr(d.ptr, 3, 4, d.ptr, d.ptr) == -1 and b"smaller than n" in lib.np_last_error()
    assert lib.np_geqrf(d.ptr, 3, 4, d.ptr) == -1
    assert lib.np_lstsq(d.ptr, d.ptr, 3, 4, 1, d.ptr, C.byref(info)) == -1 and info.value == -3
    assert np.all(d.to_host() == 5.0)
    assert lib.np_qr(None, 4, 3, d.ptr, d.ptr) == -1 and lib.np_qr(d.ptr, 4, 3, None, d.ptr) == -1 and lib.np_qr(d.ptr, 4, 3, d.ptr, None) == -1
    assert lib.np_geqrf(None, 4, 3, d.ptr) == -1 and lib.np_geqrf(d.ptr, 4, 3, None) == -1
    assert lib.np_lstsq(d.ptr, d.ptr, 4, 3, 1, d.ptr, None) == -1 and lib.np_lstsq(d.ptr, None, 4, 3, 1, d.ptr, C.byref(info)) == -1
    assert lib.np_qr(d.ptr, 65537, 65537, d.ptr, d.ptr) == -1 and b"65536" in lib.np_last_error()
    assert lib.np_geqrf(d.ptr, (1 << 24) + 1, 2, d.ptr) == -1 and b"16777216" in lib.np_last_error()
    _l.check(lib.np_qr(d.ptr, 0, 0, d.ptr, d.ptr))
    _l.check(lib.np_lstsq(d.ptr, d.ptr, 4, 3, 0, d.ptr, C.byref(info)))
    assert info.value == 0 and np.all(d.to_host() == 5.0)
    assert lib.np_live_allocs() == live
    a, b = F.gaussian(150, 70), F.gaussian(150, 3, 9)
    _qr(hip, a)
    _geqrf(hip, a)
    _lstsq(hip, a, b)
    assert lib.np_live_allocs() == live
    before = nd.live_device_allocations()
    ga, gb = _gpu(a), _gpu(b)
    r = nd.qr(ga)
    assert tuple(r[0].shape()) == (150, 70) and tuple(r[1].shape()) == (70, 70)
    x = nd.lstsq(ga, gb)
    assert tuple(x.shape()) == (70, 3)
    del r, x, ga, gb
    assert nd.live_device_allocations() == before
    d.free()
