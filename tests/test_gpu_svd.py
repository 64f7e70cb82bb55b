"""The device SVD (np_jacobi.hip: np_svd / np_svdvals; NDArray.svd, matrix_rank, norm, cond).

Exact tests.  a = P diag(d) Q with signed permutations and distinct d = j 2^e (tests/svd_family.py): the columns are already
orthogonal, every dot product has one non-zero term and every norm is the root of an exactly represented perfect square, so
S is sort(d) descending bit for bit, every entry of U and Vt is 0 or +-1, U diag(S) Vt == a element for element, info = 0 —
through np_svd, np_svdvals, NDArray_SVD and NDArray.svd.

Known spectrum.  Hadamard products with singular values n .. 1: serr against the closed form.

Bound tests.  rec, orthA, orthN, serr (svd_family.metrics; float64 arithmetic on the fp32 results, eps = 2^-23):
  max(m, n) <= 512   metric <= max(2 eps, 4 x the same metric of the CPU emulator on the same input) — the emulator
                     (svd_family.jacobi_svd_emulated: fp32 storage, fp64 rotations, unblocked) is the calibration because
                     neither LAPACK (Householder) nor the reference (cuSOLVER) says what an fp32 Jacobi iteration reaches;
                     the factor 4 is room for another blocking and summation order, a dropped rotation gives O(1)
  larger             metric <= max(m, n) eps / 2: four times the emulator's growth (about n / 9 eps on the shifted squares)
Every test asserts from numpy's float64 spectrum of its own input that no vector can drop out of the "live" filter
(s_min / s_0 >= 16 x the threshold; the two Hadamard cases with n = 1024 have s_min / s_0 = 1 / 1024 in closed form, which is
8 x and 2 x their thresholds, and are held to those margins, 8 and 2, and to "no vector excluded"), on the rank-r inputs that exactly
min(m, n) - r do.  Each case prints its figures
before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import svd_family as F

pytestmark = pytest.mark.gpu
EPS = F.EPS


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


def _svd(hip, a):
    """np_svd: (u, s, vt, info, the input buffer afterwards)"""
    _l, lib = _lib()
    m, n = a.shape
    k = min(m, n)
    da = hip.DeviceArray.from_host(a)
    du, ds, dv = hip.DeviceArray((m, k)), hip.DeviceArray((k,)), hip.DeviceArray((k, n))
    info = C.c_int(-1)
    _l.check(lib.np_svd(da.ptr, m, n, du.ptr, ds.ptr, dv.ptr, C.byref(info)))
    out = du.to_host().reshape(m, k), ds.to_host().reshape(k), dv.to_host().reshape(k, n), info.value, da.to_host().reshape(m, n)
    for d in (da, du, ds, dv):
        d.free()
    return out


def _svdvals(hip, a):
    _l, lib = _lib()
    m, n = a.shape
    da, ds = hip.DeviceArray.from_host(a), hip.DeviceArray((min(m, n),))
    info = C.c_int(-1)
    _l.check(lib.np_svdvals(da.ptr, m, n, ds.ptr, C.byref(info)))
    out = ds.to_host().reshape(-1), info.value
    da.free()
    ds.free()
    return out


def _nd_svd(a):
    U, S, V = _nd().svd(_gpu(a))
    return U.cpu().numpy(), S.cpu().numpy(), V.cpu().numpy()


def _is_signed_selection(Q):
    """entries 0 / +-1, at most one non-zero per row and per column"""
    A = np.abs(Q)
    return bool(np.isin(A, (0.0, 1.0)).all() and (A.sum(axis=0) <= 1).all() and (A.sum(axis=1) <= 1).all())


def _check_padded(a, U, S, V):
    """the NDArray layer's shapes: U (m, m), S (k), V (n, n), the thin factors in front, +0.0f behind"""
    m, n = a.shape
    k = min(m, n)
    assert U.shape == (m, m) and S.shape == (k,) and V.shape == (n, n)
    assert not U[:, k:].any() and not np.signbit(U[:, k:]).any()
    assert not V[k:, :].any() and not np.signbit(V[k:, :]).any()
    return U[:, :k], S, V[:k, :]


# ---- exact ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", F.EXACT_SHAPES)
def test_exact_family_through_every_layer(hip, shape):
    m, n = shape
    k = min(m, n)
    a, d, _, _ = F.exact_case(m, n)
    want = np.sort(d)[::-1]
    U, S, Vt, info, after = _svd(hip, a)
    assert info == 0
    assert np.array_equal(_bits(S), _bits(want))
    assert _is_signed_selection(U) and _is_signed_selection(Vt)
    assert np.abs(U).sum() == k and np.abs(Vt).sum() == k
    assert np.array_equal((U * S) @ Vt, a)
    assert np.array_equal(_bits(after), _bits(a))
    S2, info2 = _svdvals(hip, a)
    assert info2 == 0 and np.array_equal(_bits(S2), _bits(want))
    Uf, Sf, Vf = _nd_svd(a)
    Ut, St, Vtt = _check_padded(a, Uf, Sf, Vf)
    assert np.array_equal(_bits(St), _bits(want)) and np.array_equal(_bits(Ut), _bits(U)) and np.array_equal(_bits(Vtt), _bits(Vt))
    assert np.array_equal((Uf[:, :k] * Sf) @ Vf[:k, :], a)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", [(33, 97), (97, 33), (128, 128), (129, 257)])
def test_exact_family_more_seeds(hip, shape, seed):
    a, d, _, _ = F.exact_case(*shape, seed=seed)
    U, S, Vt, info, _ = _svd(hip, a)
    assert info == 0 and np.array_equal(_bits(S), _bits(np.sort(d)[::-1])) and np.array_equal((U * S) @ Vt, a)


@pytest.mark.parametrize("shape", [(7, 7), (70, 40), (40, 70)])
def test_zero_matrix(hip, shape):
    m, n = shape
    k = min(m, n)
    a = np.zeros(shape, np.float32)
    U, S, Vt, info, _ = _svd(hip, a)
    assert info == 0 and not S.any() and not np.signbit(S).any()
    nrm, acc = (U, Vt) if m >= n else (Vt, U.T)                # acc: k x k
    assert not nrm.any() and not np.signbit(nrm).any()          # +0.0f
    assert acc.shape == (k, k) and _is_signed_selection(acc) and np.abs(acc).sum() == k   # a permutation of I


def test_one_by_one_negative_entry(hip):
    a = np.array([[-3.5]], np.float32)
    U, S, Vt, info, _ = _svd(hip, a)
    assert info == 0 and S[0] == np.float32(3.5) and U[0, 0] * S[0] * Vt[0, 0] == a[0, 0]


def test_cond_of_a_diagonal_of_powers_of_two_is_exact(hip):
    d = np.ldexp(np.ones(9, np.float32), np.array([3, -2, 0, 5, -4, 1, 2, -1, 4]))
    assert _nd().cond(_gpu(np.diag(d))) == float(d.max() / d.min()) == 512.0


@pytest.mark.parametrize("shape", [(64, 64), (200, 96), (96, 200)])
def test_norm_is_the_first_singular_value_bit_for_bit(hip, shape):
    a = F.gaussian(*shape)
    _, S, _, _, _ = _svd(hip, a)
    v = _nd().norm(_gpu(a))
    assert np.float32(v).view(np.uint32) == S[:1].view(np.uint32)[0]
    assert _nd().norm(_gpu(a), 2) == v


@pytest.mark.parametrize("case", F.RANK_CASES)
def test_matrix_rank(hip, case):
    m, n, r = case
    a = F.rank_case(m, n, r)
    nd = _nd()
    assert int(nd.matrix_rank(_gpu(a))) == r
    S, _ = _svdvals(hip, a)
    mid = float((S[4] + S[5]) / 2)
    assert int(nd.matrix_rank(_gpu(a), mid)) == 5                # an explicit tolerance is followed
    assert int(nd.matrix_rank(_gpu(a), float(S[0]))) == 0        # strict >
    assert int(nd.matrix_rank(_gpu(a), 0.0)) == int(np.count_nonzero(S > 0))


# ---- known spectrum and bounds ------------------------------------------------------------------------------------------------

def _limits(a, sigma):
    m, n = a.shape
    if max(m, n) > 512:
        return {k: max(m, n) * EPS / 2 for k in ("rec", "orthA", "orthN", "serr")}, None
    Ue, Se, Vte, sweeps, ok = F.jacobi_svd_emulated(a)
    assert ok
    ref = F.metrics(a, Ue, Se, Vte, sigma)
    return {k: max(2 * EPS, 4 * ref[k]) for k in ("rec", "orthA", "orthN", "serr")}, ref


def _check_bounds(hip, name, a, sigma=None, excluded=0):
    m, n = a.shape
    k = min(m, n)
    s64 = F.sigma64(a)
    thr = max(m, n) * EPS
    if excluded == 0:
        # no vector can drop out of the live filter.  The Hadamard family's spectrum is n .. 1 in closed form, s_min / s_0 = 1 / n
        # exactly: 8 x the threshold at 1024 x 1024 and 2 x at 4096 x 1024, so the margin of 16 cannot hold for these two
        # cases whatever the code does; they keep their closed-form margins of 8 and 2 and, like every case, `live == k` below.
        margin = 16 if sigma is None or max(m, n) <= 512 else (8 if m == n else 2)
        spec = s64 if sigma is None else sigma                  # the closed form where there is one (1 / 1024 = 2 x 4096 eps exactly)
        assert spec[-1] / spec[0] >= margin * thr
    else:
        r = k - excluded
        assert s64[r - 1] / s64[0] >= 16 * thr and s64[r] / s64[0] <= thr / 16
    U, S, Vt, info, _ = _svd(hip, a)
    got = F.metrics(a, U, S, Vt, sigma if sigma is not None else s64)
    lim, ref = _limits(a, sigma if sigma is not None else s64)
    fmt = lambda d: {key: round(d[key] / EPS, 2) for key in ("rec", "orthA", "orthN", "serr")}
    print("svd %s %dx%d info %d live %d device(eps) %s limit(eps) %s emulator(eps) %s" %
          (name, m, n, info, got["live"], fmt(got), fmt(lim), fmt(ref) if ref else "-"), flush=True)
    assert info == 0
    assert got["live"] == k - excluded
    assert np.all(S >= 0) and np.all(S[:-1] >= S[1:])
    for key in ("rec", "orthA", "orthN", "serr"):
        assert got[key] <= lim[key], (key, got[key] / EPS, lim[key] / EPS)


@pytest.mark.parametrize("shape", F.HADAMARD_SHAPES)
def test_known_spectrum(hip, shape):
    a, sigma = F.hadamard_case(*shape)
    _check_bounds(hip, "hadamard", a, sigma)


@pytest.mark.parametrize("n", F.SQUARE_SIZES)
def test_bounds_shifted_squares(hip, n):
    _check_bounds(hip, "shifted", F.shifted_square(n))


@pytest.mark.parametrize("shape", F.RECT_SHAPES)
def test_bounds_rectangular(hip, shape):
    _check_bounds(hip, "gaussian", F.gaussian(*shape))


@pytest.mark.parametrize("shape", F.SCALED_SHAPES)
def test_bounds_scaled_columns(hip, shape):
    _check_bounds(hip, "scaled", F.scaled_case(*shape))


@pytest.mark.parametrize("case", F.RANK_CASES)
def test_bounds_rank_deficient(hip, case):
    m, n, r = case
    _check_bounds(hip, "rank%d" % r, F.rank_case(m, n, r), excluded=min(m, n) - r)


# ---- the one-launch path (min(m, n) <= 64 and a row length that fits LDS) and its boundary ------------------------------------

SMALL_EDGE = [(557, 64), (558, 64), (64, 557), (64, 558), (1200, 64), (64, 1200), (3000, 5), (5, 3000), (9000, 4), (64, 64), (33, 64)]


def _launches(lib):
    c = C.c_ulonglong()
    assert lib.np_debug_launch_count(C.byref(c)) == 0
    return c.value


@pytest.mark.parametrize("shape", SMALL_EDGE)
def test_exact_family_on_both_sides_of_the_small_path(hip, shape):
    """k = 64 fits LDS up to a row length of 557: 557 takes the one-launch kernel, 558 and 1200 fall through to the blocked path;
    every shape is also run with the small path switched off.  Both paths return the exact answer, so they agree bit for bit here."""
    _l, lib = _lib()
    m, n = shape
    a, d, _, _ = F.exact_case(m, n)
    want = np.sort(d)[::-1]
    # the library's LDS rule (svd_small_floats, 156 KB) restated on purpose: it pins the documented boundary, 64 rows of 557
    # floats; a change of that constant fails here and has to change include/np_hip.h's fine print with it
    fits = min(m, n) * (max(m, n) | 1) + min(m, n) * (min(m, n) | 1) + 2 * min(m, n) <= 156 * 1024 // 4
    l0 = _launches(lib)
    U, S, Vt, info, _ = _svd(hip, a)
    used = _launches(lib) - l0
    assert (used == 1) == fits, (used, fits)
    S2, info2 = _svdvals(hip, a)
    try:
        _l.check(lib.np_debug_svd_small_path(0))
        Ub, Sb, Vtb, infob, _ = _svd(hip, a)
    finally:
        _l.check(lib.np_debug_svd_small_path(1))
    for u_, s_, v_, i_ in ((U, S, Vt, info), (Ub, Sb, Vtb, infob)):
        assert i_ == 0 and np.array_equal(_bits(s_), _bits(want))
        assert _is_signed_selection(u_) and _is_signed_selection(v_) and np.array_equal((u_ * s_) @ v_, a)
    assert info2 == 0 and np.array_equal(_bits(S2), _bits(want))
    assert np.array_equal(_bits(U), _bits(Ub)) and np.array_equal(_bits(Vt), _bits(Vtb))


@pytest.mark.parametrize("shape", [(64, 64), (40, 300), (300, 40), (7, 3), (1, 9), (557, 64)])
def test_small_path_is_one_launch_and_svdvals_has_the_same_bits(hip, shape):
    _l, lib = _lib()
    a = F.gaussian(*shape)
    l0 = _launches(lib)
    U, S, Vt, info, after = _svd(hip, a)
    l1 = _launches(lib)
    Sv, infov = _svdvals(hip, a)
    l2 = _launches(lib)
    assert l1 - l0 == 1 and l2 - l1 == 1
    assert info == 0 and infov == 0 and np.array_equal(_bits(Sv), _bits(S)) and np.array_equal(_bits(after), _bits(a))
    U2, S2, Vt2, _, _ = _svd(hip, a)
    assert np.array_equal(_bits(U), _bits(U2)) and np.array_equal(_bits(S), _bits(S2)) and np.array_equal(_bits(Vt), _bits(Vt2))


def test_small_path_sweep_cap(hip):
    _l, lib = _lib()
    a = F.gaussian(64, 64)
    try:
        _l.check(lib.np_debug_svd_max_sweeps(1))
        U, S, Vt, info, _ = _svd(hip, a)
        Sv, infov = _svdvals(hip, a)
    finally:
        _l.check(lib.np_debug_svd_max_sweeps(0))
    lim, _ = _limits(a, F.sigma64(a))
    got = F.metrics(a, U, S, Vt)
    assert 0 < info <= 64 * 63 // 2 and infov == info and np.array_equal(_bits(Sv), _bits(S))
    assert got["rec"] <= lim["rec"] and got["orthA"] <= lim["orthA"] and got["orthN"] > 16 * F.bound(64, 64)


@pytest.mark.parametrize("shape", [(64, 64), (130, 64), (17, 5), (64, 130)])
def test_blocked_path_keeps_its_bounds_where_the_small_path_now_runs(hip, shape):
    _l, lib = _lib()
    try:
        _l.check(lib.np_debug_svd_small_path(0))
        _check_bounds(hip, "gaussian-blocked", F.gaussian(*shape))
    finally:
        _l.check(lib.np_debug_svd_small_path(1))


# ---- behaviour -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 300, 2048])
def test_two_calls_give_the_same_bits_and_svdvals_the_same_s(hip, n):
    a = F.shifted_square(n)
    U1, S1, V1, i1, after = _svd(hip, a)
    U2, S2, V2, i2, _ = _svd(hip, a)
    assert i1 == i2 == 0
    assert np.array_equal(_bits(U1), _bits(U2)) and np.array_equal(_bits(S1), _bits(S2)) and np.array_equal(_bits(V1), _bits(V2))
    S3, i3 = _svdvals(hip, a)
    assert i3 == 0 and np.array_equal(_bits(S3), _bits(S1))
    assert np.array_equal(_bits(after), _bits(a))


def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    a = F.gaussian(96, 40)
    U, S, Vt, _, _ = _svd(hip, a)
    Uf, Sf, Vf = nd.svd(nd.transpose(_gpu(np.ascontiguousarray(a.T))))          # a strided view of a^T's buffer
    assert np.array_equal(_bits(Sf.cpu().numpy()), _bits(S)) and np.array_equal(_bits(Uf.cpu().numpy()[:, :40]), _bits(U))
    nd.set_lazy_binding(True)
    try:
        x = _gpu(a)
        chain = (x * 2.0) * 0.5                                                   # pending until a consumer needs it
        Ul, Sl, Vl = nd.svd(chain)
        assert np.array_equal(_bits(Sl.cpu().numpy()), _bits(S)) and np.array_equal(_bits(Vl.cpu().numpy()[:40]), _bits(Vt))
        assert nd.norm(chain) == float(S[0])
    finally:
        nd.set_lazy_binding(False)


def test_the_sweep_cap_reports_info_and_still_reconstructs(hip):
    _l, lib = _lib()
    a = F.gaussian(300, 300)
    try:
        _l.check(lib.np_debug_svd_max_sweeps(1))
        U, S, Vt, info, _ = _svd(hip, a)
        Sv, infov = _svdvals(hip, a)
    finally:
        _l.check(lib.np_debug_svd_max_sweeps(0))
    got = F.metrics(a, U, S, Vt)
    print("capped: info %d rec %.2f eps orthN %.3g eps" % (info, got["rec"] / EPS, got["orthN"] / EPS))
    lim, _ = _limits(a, F.sigma64(a))                             # the bound of the converged result: 4 x the emulator
    print("capped: limits(eps) rec %.1f orthA %.1f" % (lim["rec"] / EPS, lim["orthA"] / EPS))
    assert 0 < info <= 300 * 299 // 2 and infov == info          # row pairs above the tolerance, each counted once
    assert np.array_equal(_bits(Sv), _bits(S))
    assert got["rec"] <= lim["rec"]                               # every Jacobi state reconstructs a
    assert got["orthA"] <= lim["orthA"]                           # the accumulated factor is orthogonal at every state
    assert got["orthN"] > 16 * F.bound(300, 300)                 # far outside: one sweep does not make the columns orthogonal
    U, S, Vt, info, _ = _svd(hip, a)                              # the knob is back: a clean call
    assert info == 0 and F.metrics(a, U, S, Vt)["orthN"] <= 4 * F.bound(300, 300)


def test_non_finite_input_returns_with_a_nan(hip):
    a = F.gaussian(130, 70)
    a[17, 3] = np.nan
    U, S, Vt, info, _ = _svd(hip, a)
    assert np.isnan(S).any()
    a[17, 3] = np.inf
    S2, _ = _svdvals(hip, a)
    assert np.isnan(S2).any() or np.isinf(S2).any()


def test_errors_and_live_allocations(hip):
    from numpower_amd.ndarray import Error
    _l, lib = _lib()
    nd = _nd()
    d = hip.DeviceArray((16,))
    info = C.c_int(-1)
    live = lib.np_live_allocs()
    _l.check(lib.np_svd(d.ptr, 0, 4, d.ptr, d.ptr, d.ptr, C.byref(info)))
    assert info.value == 0
    info = C.c_int(-1)
    _l.check(lib.np_svdvals(d.ptr, 4, 0, d.ptr, C.byref(info)))
    assert info.value == 0
    assert lib.np_svd(None, 4, 4, d.ptr, d.ptr, d.ptr, C.byref(info)) == -1 and lib.np_svd(d.ptr, 4, 4, d.ptr, d.ptr, d.ptr, None) == -1
    assert lib.np_svdvals(d.ptr, 4, 4, None, C.byref(info)) == -1
    assert lib.np_svd(d.ptr, 65537, 1, d.ptr, d.ptr, d.ptr, C.byref(info)) == -1 and b"65536" in lib.np_last_error()
    assert lib.np_live_allocs() == live
    a = _gpu(F.gaussian(40, 24))
    live = lib.np_live_allocs()
    _svd(hip, F.gaussian(40, 24))
    _svdvals(hip, F.gaussian(24, 40))
    assert lib.np_live_allocs() == live
    r = nd.svd(a)
    del r
    nd.norm(a), nd.matrix_rank(a), nd.cond(_gpu(F.shifted_square(12)))
    for call, arg, msg in ((nd.svd, _gpu(np.ones(5, np.float32)), "Array must be at least two-dimensional"),
                           (nd.svd, _gpu(np.ones((2, 3, 4), np.float32)), "only two-dimensional"),
                           (lambda x: nd.norm(x, 3), a, "NDArray_Norm: The provided norm `3` is invalid"),
                           (lambda x: nd.norm(x, 1), a, "norm `1` is not available for GPU arrays"),
                           (nd.cond, _gpu(np.zeros((3, 3), np.float32)), "LU factorization failed")):
        before = lib.np_live_allocs()
        with pytest.raises(Error) as e:
            call(arg)
        assert msg in str(e.value)
        assert lib.np_live_allocs() == before
    d.free()


def test_svd_bodies_gpu_operands_never_reach_the_reference_code(hip):
    import subprocess
    from pathlib import Path
    exe = Path(__file__).resolve().parent.parent / "numpower_amd" / "lib" / "svd_bodies"
    proc = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "svd_bodies gpu: 0 calls reached the reference's own code, 0 failures" in proc.stdout
