"""The device symmetric eigensolver (np_jacobi.hip: np_eigh / np_eigvalsh / np_symmetry_mismatch; NDArray.eig).

Exact tests.  diag(d) with distinct +-j 2^e at permuted positions, one +0.0 and one -0.0 (tests/eig_family.py): nothing rotates,
so w is the stably sorted d bit for bit, v a permutation matrix of 0 / +1, info = 0 and a untouched — through np_eigh,
np_eigvalsh, NDArray_Eig and NDArray.eig.

Closed forms.  Tridiagonal Toeplitz, H diag(d) H^T / n, the exchange matrix, 3 I + u u^T: w against the formula within the bound
below; Toeplitz eigenvectors (n <= 129: the gaps shrink like 1 / n^2) against the sines within eps ||a|| / gap.

Bound tests.  res, orth, werr (eig_family.metrics; float64 arithmetic on the fp32 results, eps = 2^-23):
  n <= 512   metric <= max(2 eps, 4 x the same metric of the CPU emulator on the same input) — the emulator
             (eig_family.jacobi_eigh_emulated: fp32 storage, fp64 rotations, unblocked, the same activity rule) is the calibration
             because neither LAPACK nor cuSOLVER says what an fp32 Jacobi iteration reaches; the factor 4 is room for another
             blocking and summation order, a dropped rotation or a wrong pairing gives O(1)
  larger     metric <= c n eps with c = 4 x the emulator's largest growth, metric / (n eps), over the three families at n = 512
             and n = 1024, measured on the CPU (profiles/linalg/eigh_sweep.log has the table):
                         res     orth    werr
               n = 512   0.106   0.177   0.087     (the graded family on res and orth, the plain symmetric one on werr)
               n = 1024  0.115   0.186   0.106     (the graded family on all three)
               c         0.46    0.74    0.42      (4 x the larger row, rounded down)
The closed-form inputs follow the same rule: the emulator on the same input up to n = 512 (run on the spot up to 257, recorded in
tests/golden/eig_emulator_recorded.json for the Toeplitz matrix of 500), c n eps above (Toeplitz 1000, Hadamard 1024).
Each case prints its figures, numpy's fp32 eigh beside them (not a gate), before it asserts."""
import ctypes as C
import gc
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import eig_family as F

pytestmark = pytest.mark.gpu
EPS = F.EPS
GROWTH = {"res": 0.46, "orth": 0.74, "werr": 0.42}             # c of the docstring


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


def _eigh(hip, a):
    """np_eigh: (w, v, info, the input buffer afterwards)"""
    _l, lib = _lib()
    n = a.shape[0]
    da = hip.DeviceArray.from_host(a)
    dw, dv = hip.DeviceArray((n,)), hip.DeviceArray((n, n))
    info = C.c_int(-1)
    _l.check(lib.np_eigh(da.ptr, n, dw.ptr, dv.ptr, C.byref(info)))
    out = dw.to_host().reshape(n), dv.to_host().reshape(n, n), info.value, da.to_host().reshape(n, n)
    for d in (da, dw, dv):
        d.free()
    return out


def _eigvalsh(hip, a):
    _l, lib = _lib()
    n = a.shape[0]
    da, dw = hip.DeviceArray.from_host(a), hip.DeviceArray((n,))
    info = C.c_int(-1)
    _l.check(lib.np_eigvalsh(da.ptr, n, dw.ptr, C.byref(info)))
    out = dw.to_host().reshape(n), info.value
    da.free()
    dw.free()
    return out


def _nd_eig(a):
    w, v = _nd().eig(a if not isinstance(a, np.ndarray) else _gpu(a))
    return w.cpu().numpy(), v.cpu().numpy()


def _sweeps(lib):
    s = C.c_int(-1)
    assert lib.np_debug_eigh_last_sweeps(C.byref(s)) == 0
    return s.value


def _launches(lib):
    c = C.c_ulonglong()
    assert lib.np_debug_launch_count(C.byref(c)) == 0
    return c.value


def _follows_the_sign_rule(v):
    """exactly, on the returned values: the first component of largest magnitude in every column is positive"""
    at = np.argmax(np.abs(v), axis=0)
    return bool(np.all(v[at, np.arange(v.shape[1])] > 0))


# ---- exact ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", F.EXACT_SIZES)
def test_exact_family_through_every_layer(hip, n):
    a, d = F.exact_diagonal(n)
    want, order = F.sorted_stable(d)
    perm = np.zeros((n, n), np.float32)
    perm[order, np.arange(n)] = 1.0                              # column j = the unit vector of the position w[j] came from
    w, v, info, after = _eigh(hip, a)
    assert info == 0
    assert _same(w, want)                                        # -0.0 and +0.0 included, in their diagonal order
    assert _same(v, perm)                                        # exactly 0 or +1: no -0.0 either
    assert _same(after, a)
    w2, info2 = _eigvalsh(hip, a)
    assert info2 == 0 and _same(w2, want)
    wf, vf = _nd_eig(a)
    assert _same(wf, want) and _same(vf, perm)


@pytest.mark.parametrize("n", [1, 5, 64, 65, 200])
def test_a_multiple_of_the_identity_keeps_its_order_and_the_zero_matrix_too(hip, n):
    for c in (2.5, -3.0, 0.0):
        a = (c * np.eye(n)).astype(np.float32)
        w, v, info, _ = _eigh(hip, a)
        assert info == 0 and _same(w, np.full(n, c, np.float32)) and _same(v, np.eye(n, dtype=np.float32))
    w, v, info, _ = _eigh(hip, np.zeros((n, n), np.float32))
    assert info == 0 and not w.any() and not np.signbit(w).any() and _same(v, np.eye(n, dtype=np.float32))


def test_one_by_one(hip):
    for x in (-3.5, 0.0, 7.0):
        w, v, info, _ = _eigh(hip, np.array([[x]], np.float32))
        assert info == 0 and _same(w, np.array([x], np.float32)) and _same(v, np.ones((1, 1), np.float32))


def test_two_by_two_signs_against_the_closed_form(hip):
    h = np.float32(np.sqrt(0.5))
    w, v, info, _ = _eigh(hip, np.array([[2, 1], [1, 2]], np.float32))
    assert info == 0 and _same(w, np.array([1, 3], np.float32))
    # (1, -1) / sqrt 2 for 1: equal magnitudes, the first is the positive one; (1, 1) / sqrt 2 for 3
    assert np.abs(v - np.array([[h, h], [-h, h]])).max() <= EPS


# ---- the lower triangle -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 64, 65, 200])
def test_only_the_lower_triangle_is_read(hip, n):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    a = F.random_symmetric(n)
    w, v, info, _ = _eigh(hip, a)
    assert info == 0
    held = []
    for junk in (np.nan, np.inf, 1e30):
        b = a.copy()
        b[np.triu_indices(n, 1)] = junk
        w2, v2, info2, after = _eigh(hip, b)
        assert info2 == 0 and _same(w2, w) and _same(v2, v) and _same(after, b)
        w3, info3 = _eigvalsh(hip, b)
        assert info3 == 0 and _same(w3, w)
        held.append(_gpu(b))                                       # kept to the end: nothing is freed between the two counts
        gc.collect()                                               # nor by a collector run that garbage of earlier tests has made due
        live = lib.np_live_allocs()
        with pytest.raises(Error) as e:                            # the NDArray layer does not answer from one triangle
            _nd().eig(held[-1])
        assert "symmetric eigensolver" in str(e.value) and "->cpu()" in str(e.value)
        assert lib.np_live_allocs() == live


# ---- closed forms and bounds --------------------------------------------------------------------------------------------------

def _limits(n, family=None, a=None, name=None, lam=None):
    """-> (limit per metric, the emulator's metrics or None); family: a bound family, else the closed-form input `name`"""
    if n > 512:
        return {k: GROWTH[k] * n * EPS for k in F.METRICS}, None
    ref = F.emulator_metrics(family, n) if family is not None else F.closed_form_emulator_metrics(name, a, lam)
    return {k: max(2 * EPS, 4 * ref[k]) for k in F.METRICS}, ref


def _check_bounds(hip, name, a, lam=None, family=None):
    n = a.shape[0]
    lam64 = F.w64(a) if lam is None else lam
    w, v, info, _ = _eigh(hip, a)
    _l, lib = _lib()
    sweeps = _sweeps(lib)
    got = F.metrics(a, w, v, lam64)
    lim, ref = _limits(n, family, a, name, lam64)
    wn, vn = np.linalg.eigh(a)
    host = F.metrics(a, wn, vn, lam64)
    fmt = lambda d: {key: round(d[key] / EPS, 2) for key in F.METRICS}
    print("eigh %s n %d info %d sweeps %d device(eps) %s limit(eps) %s emulator(eps) %s numpy-fp32(eps) %s" %
          (name, n, info, sweeps, fmt(got), fmt(lim), fmt(ref) if ref else "-", fmt(host)), flush=True)
    assert info == 0
    assert np.all(w[:-1] <= w[1:]) and _follows_the_sign_rule(v)
    for key in F.METRICS:
        assert got[key] <= lim[key], (key, got[key] / EPS, lim[key] / EPS)
    return w, v


@pytest.mark.parametrize("n", F.TOEPLITZ_SIZES)
def test_toeplitz_against_the_closed_form(hip, n):
    a, lam, vec = F.toeplitz(n)
    w, v = _check_bounds(hip, "toeplitz", a, lam)                # werr is measured against the formula
    if n <= 129:
        # Davis-Kahan: a unit vector with residual r lies within about ||r|| / gap of the eigenvector (res bounds ||r|| / ||a||,
        # werr moves the gap's ends), plus the loss of normalisation orth allows
        lim, _ = _limits(n, None, a, "toeplitz", lam)
        gap = np.minimum(np.diff(lam, prepend=-np.inf), np.diff(lam, append=np.inf))
        tol = 2.0 * max(lim["res"], lim["werr"]) * lam[-1] / gap + lim["orth"]
        # The sign rule against the formula.  Column k is symmetric about the middle for odd k and antisymmetric for even k, and
        # |sin(i k pi / (n + 1))| takes every value exactly twice, at i and n + 1 - i, when gcd(k, n + 1) = 1.  For odd k those
        # two components have the same sign, so the rule fixes the column's sign whichever of them rounds larger: these columns
        # are compared with the rule applied to the formula, no alignment.  For even k the two have opposite signs, and with a
        # common factor the maximum recurs with alternating signs: there rounding decides, and the formula is aligned with the
        # column (the rule itself is checked exactly on the returned values in _check_bounds).
        k = np.arange(1, n + 1)
        decided = (k % 2 == 1) & (np.gcd(k, n + 1) == 1)
        ruled = F.apply_sign_rule(vec)
        aligned = vec * np.where((vec * v).sum(axis=0) < 0, -1.0, 1.0)
        want = np.where(decided, ruled, aligned)
        err = np.abs(v - want).max(axis=0)
        print("toeplitz n %d: %d columns held to the sign rule, worst eigenvector error %.1f eps, at %.2f of its limit" %
              (n, int(decided.sum()), err.max() / EPS, (err / tol).max()))
        assert decided.any() and np.all(err <= tol)


@pytest.mark.parametrize("n", F.HADAMARD_SIZES)
def test_hadamard_known_spectrum(hip, n):
    a, d = F.hadamard_case(n)
    _check_bounds(hip, "hadamard", a, d)


@pytest.mark.parametrize("n", F.EXCHANGE_SIZES)
def test_exchange_matrix_converges_in_two_sweeps(hip, n):
    _l, lib = _lib()
    a, lam = F.exchange(n)
    w, v = _check_bounds(hip, "exchange", a, lam)
    assert _sweeps(lib) <= 3
    assert _same(w, lam.astype(np.float32))                       # a 45 degree rotation in fp64: -1 and +1 exactly


@pytest.mark.parametrize("n", [5, 64, 130])
def test_rank_one_update_of_a_multiple_of_the_identity(hip, n):
    a, lam = F.rank_one_shift(n)
    _check_bounds(hip, "3I+uu^T", a, lam)


@pytest.mark.parametrize("family", sorted(F.BOUND_FAMILIES))
@pytest.mark.parametrize("n", F.BOUND_SIZES)
def test_bounds(hip, n, family):
    _check_bounds(hip, family, F.BOUND_FAMILIES[family](n), family=family)


# ---- the one-launch path and the blocked path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 64])
def test_both_paths_meet_the_bounds_where_the_small_path_runs(hip, n):
    _l, lib = _lib()
    a = F.random_symmetric(n)
    _check_bounds(hip, "symmetric-small", a, family="symmetric")
    try:
        _l.check(lib.np_debug_eigh_small_path(0))
        _check_bounds(hip, "symmetric-blocked", a, family="symmetric")
        e, d = F.exact_diagonal(n)
        w, v, info, _ = _eigh(hip, e)
        assert info == 0 and _same(w, F.sorted_stable(d)[0])
    finally:
        _l.check(lib.np_debug_eigh_small_path(1))


def test_the_small_path_is_one_launch_and_the_blocked_path_several(hip):
    _l, lib = _lib()
    a = F.random_symmetric(64)
    l0 = _launches(lib)
    w, v, info, _ = _eigh(hip, a)
    l1 = _launches(lib)
    wv, infov = _eigvalsh(hip, a)
    l2 = _launches(lib)
    assert l1 - l0 == 1 and l2 - l1 == 1 and info == 0 and infov == 0 and _same(wv, w)
    try:
        _l.check(lib.np_debug_eigh_small_path(0))
        l0 = _launches(lib)
        _eigh(hip, a)
        assert _launches(lib) - l0 > 3
    finally:
        _l.check(lib.np_debug_eigh_small_path(1))
    l0 = _launches(lib)
    _eigh(hip, F.random_symmetric(65))
    assert _launches(lib) - l0 > 3


# ---- behaviour -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 257, 1000])
def test_two_calls_give_the_same_bits_and_eigvalsh_the_same_w(hip, n):
    a = F.random_symmetric(n)
    w1, v1, i1, after = _eigh(hip, a)
    w2, v2, i2, _ = _eigh(hip, a)
    assert i1 == i2 == 0 and _same(w1, w2) and _same(v1, v2) and _same(after, a)
    w3, i3 = _eigvalsh(hip, a)
    assert i3 == 0 and _same(w3, w1)


def test_the_sweep_cap_reports_info_and_the_ndarray_layer_raises(hip):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    for n in (40, 300):                                            # both paths
        a = F.random_symmetric(n)
        x = _gpu(a)
        try:
            _l.check(lib.np_debug_eigh_max_sweeps(1))
            w, v, info, _ = _eigh(hip, a)
            wv, infov = _eigvalsh(hip, a)
            assert _sweeps(lib) == 1
            live = lib.np_live_allocs()
            with pytest.raises(Error, match="sweep cap"):
                _nd().eig(x)
            assert lib.np_live_allocs() == live
        finally:
            _l.check(lib.np_debug_eigh_max_sweeps(0))
        assert 0 < info <= n * (n - 1) // 2 and infov == info and _same(wv, w)
        assert np.isfinite(w).all() and np.isfinite(v).all()      # the results are returned anyway
        w, v, info, _ = _eigh(hip, a)                              # the knob is back: a clean call
        assert info == 0


@pytest.mark.parametrize("n", [20, 130])
def test_non_finite_input_returns_with_a_nan_and_the_next_call_is_clean(hip, n):
    a = F.random_symmetric(n)
    good = _eigh(hip, a)
    for junk in (np.nan, np.inf):
        b = a.copy()
        b[n // 2, 3] = junk                                        # in the lower triangle
        w, v, info, _ = _eigh(hip, b)
        assert np.isnan(w).any()
        wv, _ = _eigvalsh(hip, b)
        assert np.isnan(wv).any()
    again = _eigh(hip, a)
    assert again[2] == 0 and _same(again[0], good[0]) and _same(again[1], good[1])


def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    n = 70
    a = F.random_symmetric(n)
    w, v, _, _ = _eigh(hip, a)
    wt, vt = _nd_eig(nd.transpose(_gpu(a)))                       # a strided view; a^T = a element for element
    assert _same(wt, w) and _same(vt, v)
    big = np.full((n + 3, n + 5), 9.0, np.float32)
    big[1:1 + n, 2:2 + n] = a
    ws, vs = _nd_eig(_gpu(big).slice([1, 1 + n], [2, 2 + n]))    # a strided slice
    assert _same(ws, w) and _same(vs, v)
    nd.set_lazy_binding(True)
    try:
        chain = (_gpu(a) * 2.0) * 0.5                              # pending until a consumer needs it
        wl, vl = _nd_eig(chain)
        assert _same(wl, w) and _same(vl, v)
    finally:
        nd.set_lazy_binding(False)


def test_errors_and_live_allocations(hip):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    nd = _nd()
    d = hip.DeviceArray((16,))
    info = C.c_int(-1)
    live = lib.np_live_allocs()
    _l.check(lib.np_eigh(d.ptr, 0, d.ptr, d.ptr, C.byref(info)))
    assert info.value == 0
    info = C.c_int(-1)
    _l.check(lib.np_eigvalsh(d.ptr, 0, d.ptr, C.byref(info)))
    assert info.value == 0
    assert lib.np_eigh(None, 4, d.ptr, d.ptr, C.byref(info)) == -1 and lib.np_eigh(d.ptr, 4, d.ptr, None, C.byref(info)) == -1
    assert lib.np_eigh(d.ptr, 4, d.ptr, d.ptr, None) == -1 and lib.np_eigvalsh(d.ptr, 4, None, C.byref(info)) == -1
    assert lib.np_eigh(d.ptr, 65537, d.ptr, d.ptr, C.byref(info)) == -1 and b"65536" in lib.np_last_error()
    assert lib.np_symmetry_mismatch(None, 4, C.byref(info)) == -1
    assert lib.np_live_allocs() == live
    _eigh(hip, F.random_symmetric(40))
    _eigvalsh(hip, F.random_symmetric(90))
    assert lib.np_live_allocs() == live
    a = _gpu(F.random_symmetric(30))
    r = nd.eig(a)
    assert tuple(r[0].shape()) == (30,) and tuple(r[1].shape()) == (30, 30)
    del r
    skew = F.random_symmetric(30)
    skew[7, 2] += 1.0
    nan_pair = F.random_symmetric(30)
    nan_pair[7, 2] = nan_pair[2, 7] = np.nan                       # two NaNs count as equal: symmetric, and w is NaN
    assert np.isnan(_nd_eig(nan_pair)[0]).all()
    for arg, msg in ((_gpu(np.ones(5, np.float32)), "Error: Input matrix is not square.\n"),
                     (_gpu(np.ones((2, 3), np.float32)), "Error: Input matrix is not square.\n"),
                     (_gpu(np.ones((2, 2, 2), np.float32)), "Error: Input matrix is not square.\n"),
                     (_gpu(skew), "the device solver is a symmetric eigensolver")):
        before = lib.np_live_allocs()
        with pytest.raises(Error) as e:
            nd.eig(arg)
        assert msg in str(e.value) and (msg.endswith("eigensolver") or str(e.value) == msg)
        assert lib.np_live_allocs() == before
    d.free()


def test_symmetry_check(hip):
    _l, lib = _lib()
    for n in (1, 2, 65, 300):
        a = F.random_symmetric(n)
        cases = [(a, 0)]
        if n > 1:
            b, c, e = a.copy(), a.copy(), a.copy()
            b[n - 1, 0] = np.nextafter(b[n - 1, 0], np.float32(np.inf))
            c[0, n - 1] = c[n - 1, 0] = np.nan
            e[0, n - 1] = np.nan
            cases += [(b, 1), (c, 0), (e, 1)]
        for m, want in cases:
            dm = hip.DeviceArray.from_host(m)
            any_ = C.c_int(-1)
            _l.check(lib.np_symmetry_mismatch(dm.ptr, n, C.byref(any_)))
            dm.free()
            assert any_.value == want


def test_eig_bodies_gpu_operands_never_reach_the_reference_code(hip):
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "eig_bodies"
    proc = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "eig_bodies gpu: 0 calls reached the reference's own code, 0 failures" in proc.stdout
