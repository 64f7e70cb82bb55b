"""GPU tests of layer and group normalization (np_groupnorm.hip: np_groupnorm_forward, np_groupnorm_backward; NDArray.dnn_layer_norm_*
and dnn_group_norm_*) against tests/groupnorm_family.py, which tests/test_groupnorm_reference_cpu.py holds to torch.

The exact family is compared bit for bit everywhere.  Gaussian data is compared bit for bit on every row and parameter that the
guard clears (the CPU tier shows that these are all but 2 % of a case at the most, and all of a case with fewer than 50 rows); on
the rest the saved scalars are within one ulp and y, dx within the bound derived in groupnorm_family (unguarded_*_tolerance).
The exact family needs an even L (devs -1, +1) or a multiple of four (devs -3, 1, 1, 1): it runs at every shape that has one.

Operands sit at float offsets 0 .. 3 inside NaN frames and outputs inside a canary (gemm_family.framed / canary); every call asserts
the whole probe record against the dispatcher restated in groupnorm_family.py, and every case runs unforced and with every form
that can serve it forced."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from tests import groupnorm_family as B
from tests.test_gpu_batchnorm import _Call, same

pytestmark = pytest.mark.gpu
F32 = np.float32


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _bounds():
    _l, lib = _lib()
    b = (C.c_size_t * 7)()
    _l.check(lib.np_debug_groupnorm_bounds(b, 7))
    return tuple(b)


def _probe():
    _l, lib = _lib()
    r, p, n, rs, ps = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
    _l.check(lib.np_debug_groupnorm_last_path(C.byref(r), C.byref(p), C.byref(n), C.byref(rs), C.byref(ps)))
    return r.value, p.value, n.value, rs.value, ps.value


@contextlib.contextmanager
def _forced(row, param=None):
    _l, lib = _lib()
    _l.check(lib.np_debug_groupnorm_force_form(-1 if row is None else row, -1 if param is None else param))
    try:
        yield
    finally:
        _l.check(lib.np_debug_groupnorm_force_form(-1, -1))


def _row_forms(shape):
    """None (the unforced choice) and every row form that can serve the shape"""
    L = shape[2] * shape[3]
    return [None] + [f for f in (B.ROW_SHORT, B.ROW_WAVE, B.ROW_GROUP, B.ROW_SPLIT) if B.row_serves(f, L, _bounds())]


def _param_forms(shape):
    return [None] + [f for f in (B.PARAM_COLUMNS, B.PARAM_PLANES) if B.param_serves(f, shape[3])]


def _expect_probe(shape, row, param, backward, grads):
    bounds = _bounds()
    r = B.pick_row_form(shape[2] * shape[3], bounds) if row is None else row
    p = B.PARAM_NONE if not (backward and grads) else B.pick_param_form(shape[3]) if param is None else param
    return r, p, B.launches(r, p), B.row_slices(r, *shape, bounds), B.param_slices(p, *shape, bounds)


def _fwd(hip, x, gamma, beta, eps, off=0, row=None):
    """np_groupnorm_forward on a (N, G, D, inner) array -> dict; the probe must report what the dispatcher says"""
    _l, lib = _lib()
    N, G, D, inner = x.shape
    c = _Call(hip, off)
    try:
        px, pg, pb = c.operand(x), c.operand(gamma), c.operand(beta)
        pm, om = c.output((N, G))
        pi, oi = c.output((N, G))
        py, oy = c.output(x.shape)
        with _forced(row):
            _l.check(lib.np_groupnorm_forward(px, pg, pb, N, G, D, inner, eps, py, pm, pi))
        assert _probe() == _expect_probe(x.shape, row, None, False, False), (_probe(), row, x.shape)
        return {"y": c.take(oy), "save_mean": c.take(om), "save_invstd": c.take(oi)}
    finally:
        c.free()


def _bwd(hip, x, dy, gamma, mean, invstd, off=0, row=None, param=None, grads=(True, True), alias=False):
    _l, lib = _lib()
    N, G, D, inner = x.shape
    c = _Call(hip, off)
    try:
        px, pg, pm, pi = c.operand(x), c.operand(gamma), c.operand(mean), c.operand(invstd)
        if alias:
            pdx, odx = c.output(x.shape, dy)
            pdy = pdx
        else:
            pdy = c.operand(dy)
            pdx, odx = c.output(x.shape)
        pdg, odg = c.output((G * D,)) if grads[0] else (None, None)
        pdb, odb = c.output((G * D,)) if grads[1] else (None, None)
        with _forced(row, param):
            _l.check(lib.np_groupnorm_backward(px, pdy, pg, pm, pi, N, G, D, inner, pdx, pdg, pdb))
        assert _probe() == _expect_probe(x.shape, row, param, True, any(grads)), (_probe(), row, param, x.shape)
        return {"dx": c.take(odx), "dgamma": c.take(odg) if grads[0] else None, "dbeta": c.take(odb) if grads[1] else None}
    finally:
        c.free()


def _through_ndarray(x, dy, gamma, beta, eps, mean, invstd):
    """the same case through NDArray: layer normalization where G = 1 and inner = 1, group normalization otherwise"""
    nd = _nd()
    N, G, D, inner = x.shape
    g, b = (None if a is None else _gpu(a) for a in (gamma, beta))
    if G == 1 and inner == 1:
        y, m, i = nd.dnn_layer_norm_forward(_gpu(x.reshape(N, D)), D, g, b, eps)
        assert y.shape() == [N, D] and m.shape() == [N] and i.shape() == [N]
        dx, dg, db = nd.dnn_layer_norm_backward(_gpu(x.reshape(N, D)), _gpu(dy.reshape(N, D)), (D,), g, _gpu(mean.reshape(N)), _gpu(invstd.reshape(N)))
        assert dx.shape() == [N, D] and dg.shape() == [D] and db.shape() == [D]
    else:
        y, m, i = nd.dnn_group_norm_forward(_gpu(x.reshape(N, G * D, inner)), G, g, b, eps)
        assert y.shape() == [N, G * D, inner] and m.shape() == [N, G] and i.shape() == [N, G]
        dx, dg, db = nd.dnn_group_norm_backward(_gpu(x.reshape(N, G * D, inner)), _gpu(dy.reshape(N, G * D, inner)), G, g, _gpu(mean), _gpu(invstd))
        assert dx.shape() == [N, G * D, inner] and dg.shape() == [G * D]
    host = lambda a, shape: a.cpu().numpy().reshape(shape)
    return ({"y": host(y, x.shape), "save_mean": host(m, (N, G)), "save_invstd": host(i, (N, G))},
            {"dx": host(dx, x.shape), "dgamma": host(dg, (G * D,)), "dbeta": host(db, (G * D,))})


# ---- 1. the exact family ---------------------------------------------------------------------------------------------------------------------------------
def _exact_cases():
    """one pattern per shape: (-3, 1, 1, 1) and (-1, +1) take turns where L is a multiple of four, (-1, +1) where L is even"""
    out = []
    for shape in dict.fromkeys(c[:4] for c in B.GAUSSIAN_CASES):
        L = shape[2] * shape[3]
        if L % 2 == 0:
            out.append(("m3" if L % 4 == 0 and len(out) % 2 else "pm1", shape))
    return out


EXACT = _exact_cases()


@pytest.mark.parametrize("pattern, shape", EXACT, ids=lambda v: str(v).replace(" ", ""))
def test_exact_family_by_bits_in_every_form(hip, pattern, shape):
    M = shape[0] * shape[1]
    constant = (M - 1,) if M >= 2 else ()
    d = B.exact_family(*shape, pattern, seed=7, constant=constant)
    x = d["x"]
    plain = B.apply(x, d["save_mean"], d["save_invstd"])
    for k, row in enumerate(_row_forms(shape)):
        f = _fwd(hip, x, d["gamma"], d["beta"], d["eps"], off=k, row=row)
        for name in ("y", "save_mean", "save_invstd"):
            assert same(f[name], d[name]), (name, row)
        for r in constant:      # eps > 0: y = beta by bits; eps = 0: NaN
            yr, br = f["y"].reshape(M, -1)[r], B._per_row(d["beta"], *shape)[r]
            assert (yr.view(np.uint32) == br.view(np.uint32)).all() if d["eps"] > 0 else np.isnan(yr).all()
        b = _bwd(hip, x, d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], off=k + 1, row=row)
        for name in ("dx", "dgamma", "dbeta"):
            assert same(b[name], d[name]), (name, row)
        assert same(_fwd(hip, x, None, None, d["eps"], off=k + 2, row=row)["y"], plain), row                        # NULL gamma and beta
        assert same(_fwd(hip, x, d["gamma"], None, d["eps"], off=k + 3, row=row)["y"], B.apply(x, d["save_mean"], d["save_invstd"], d["gamma"])), row
        ba = _bwd(hip, x, d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], off=k, row=row, grads=(False, False), alias=True)
        assert same(ba["dx"], d["dx"]), row                                                                            # no parameter reduction, dx aliasing dy
    for k, param in enumerate(_param_forms(shape)[1:]):
        b = _bwd(hip, x, d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], off=k, param=param)
        assert same(b["dgamma"], d["dgamma"]) and same(b["dbeta"], d["dbeta"]) and same(b["dx"], d["dx"]), param
        b = _bwd(hip, x, d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], off=k + 1, param=param, grads=(True, False), alias=True)
        assert same(b["dgamma"], d["dgamma"]) and b["dbeta"] is None and same(b["dx"], d["dx"]), param
        b = _bwd(hip, x, d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], off=k + 2, param=param, grads=(False, True))
        assert same(b["dbeta"], d["dbeta"]) and b["dgamma"] is None, param
    nf, nb = _through_ndarray(x, d["dy"], d["gamma"], d["beta"], d["eps"], d["save_mean"], d["save_invstd"])
    assert all(same(nf[n], d[n]) for n in nf) and all(same(nb[n], d[n]) for n in nb)


# ---- 2. Gaussian data, bit for bit under the guard ----------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.reshape(-1).view(np.int32).astype(np.int64) - b.reshape(-1).view(np.int32).astype(np.int64))


def _check_forward(got, ref, ok, tol, what):
    M = ok.size
    for name in ("save_mean", "save_invstd"):
        u = _ulps(got[name], ref[name])
        assert (u[ok] == 0).all() and (u <= 1).all(), (name, what)
    y, yr = got["y"].reshape(M, -1), ref["y"].reshape(M, -1)
    assert same(y[ok], yr[ok]), ("y", what)
    assert (np.abs(y[~ok].astype(np.float64) - yr[~ok]) <= tol.reshape(M, -1)[~ok]).all(), ("y beyond the guard", what)


def _check_backward(got, ref, ok_rows, ok_params, tol, what):
    M = ok_rows.size
    dx, dxr = got["dx"].reshape(M, -1), ref["dx"].reshape(M, -1)
    assert same(dx[ok_rows], dxr[ok_rows]), ("dx", what)
    assert (np.abs(dx[~ok_rows].astype(np.float64) - dxr[~ok_rows]) <= tol.reshape(M, -1)[~ok_rows]).all(), ("dx beyond the guard", what)
    for name in ("dgamma", "dbeta"):
        if got[name] is not None:
            u = _ulps(got[name], ref[name])
            assert (u[ok_params] == 0).all() and (u <= 1).all(), (name, what)


@pytest.mark.parametrize("case", B.GAUSSIAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_data_by_bits_in_every_form(hip, case):
    shape = case[:4]
    d = B.gaussian_family(*case)
    x, dy, g, b_, eps = d["x"], d["dy"], d["gamma"], d["beta"], d["eps"]
    ref = B.forward(x, g, b_, eps)
    mean, invstd = ref["save_mean"], ref["save_invstd"]
    bref = B.backward(x, dy, g, mean, invstd)
    bplain = B.backward(x, dy, None, mean, invstd)
    ok_f, ok_r, ok_p = B.guarded(ref["wide"], "forward"), B.guarded(bref["wide"], "rows"), B.guarded(bref["wide_param"], "params")
    ok_plain = B.guarded(bplain["wide"], "rows")
    tol_y, tol_dx = B.unguarded_y_tolerance(x, ref, g, b_), B.unguarded_dx_tolerance(x, dy, g, mean, invstd, bref)
    tol_plain_y, tol_plain_dx = B.unguarded_y_tolerance(x, ref, None, None), B.unguarded_dx_tolerance(x, dy, None, mean, invstd, bplain)
    plain = {"y": B.apply(x, mean, invstd), "save_mean": mean, "save_invstd": invstd}
    for k, row in enumerate(_row_forms(shape)):
        _check_forward(_fwd(hip, x, g, b_, eps, off=k, row=row), ref, ok_f, tol_y, row)
        _check_forward(_fwd(hip, x, None, None, eps, off=k + 1, row=row), plain, ok_f, tol_plain_y, row)
        _check_backward(_bwd(hip, x, dy, g, mean, invstd, off=k + 2, row=row), bref, ok_r, ok_p, tol_dx, row)
        _check_backward(_bwd(hip, x, dy, g, mean, invstd, off=k + 3, row=row, grads=(False, False), alias=True), bref, ok_r, ok_p, tol_dx, row)
        _check_backward(_bwd(hip, x, dy, None, mean, invstd, off=k, row=row, grads=(False, True)), bplain, ok_plain, ok_p, tol_plain_dx, row)
    for k, param in enumerate(_param_forms(shape)[1:]):
        _check_backward(_bwd(hip, x, dy, g, mean, invstd, off=k, param=param), bref, ok_r, ok_p, tol_dx, param)
    nf, nb = _through_ndarray(x, dy, g, b_, eps, mean, invstd)
    _check_forward(nf, ref, ok_f, tol_y, "NDArray")
    _check_backward(nb, bref, ok_r, ok_p, tol_dx, "NDArray")


VARIANCE_AT_1E4 = 1e-6 + (2.0 ** -10) ** 2 / 12


@pytest.mark.parametrize("case", B.OTHER_CASES["large_mean"], ids=lambda c: "x".join(map(str, c)))
def test_the_large_mean_rows_give_the_evaluators_invstd(hip, case):
    """mean 1e4, sigma 1e-3: the variance comes out to within five standard deviations of an estimate from L values, 5 sqrt(2 / L),
    not the noise of E[x^2] - mean^2, in every form.  The variance of the fp32 data is sigma^2 = 1e-6 plus that of its rounding to
    the fp32 grid at 1e4, q = 2^-10: q^2 / 12."""
    shape, L = case[:4], case[2] * case[3]
    d = B.gaussian_family(*case)
    rows = [r for r in range(shape[0]) if B.MEANS[r % 2] == 1e4 and B.SIGMAS[(r // 3) % 2] == 1e-3]
    assert len(rows) >= 2
    ref = B.forward(d["x"], eps=d["eps"])
    ok = B.guarded(ref["wide"], "forward")
    for row in _row_forms(shape):
        f = _fwd(hip, d["x"], None, None, d["eps"], row=row)
        _check_forward(f, ref, ok, B.unguarded_y_tolerance(d["x"], ref, None, None), row)
        for r in rows:
            assert abs(1 / float(f["save_invstd"][r, 0]) ** 2 - d["eps"] - VARIANCE_AT_1E4) < 5 * np.sqrt(2 / L) * VARIANCE_AT_1E4


# ---- 3. identities, by bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.OTHER_CASES["identities"], ids=lambda c: "x".join(map(str, c)))
def test_three_runs_a_sample_alone_and_a_batch_permutation(hip, case):
    shape = case[:4]
    N = shape[0]
    d = B.gaussian_family(*case)
    x, dy, g, b_, eps = d["x"], d["dy"], d["gamma"], d["beta"], d["eps"]
    runs = [_fwd(hip, x, g, b_, eps, off=k) for k in range(3)]
    for r in runs[1:]:
        assert all(same(r[n], runs[0][n]) for n in r)
    mean, invstd = runs[0]["save_mean"], runs[0]["save_invstd"]
    back = [_bwd(hip, x, dy, g, mean, invstd, off=k) for k in range(3)]
    for r in back[1:]:
        assert all(same(r[n], back[0][n]) for n in r)
    for n in (0, N - 1):                                      # the rows of one sample alone equal the same rows among N
        for row in _row_forms(shape):
            alone = _fwd(hip, x[n:n + 1], g, b_, eps, row=row)
            assert same(alone["y"], runs[0]["y"][n:n + 1]) and same(alone["save_invstd"], invstd[n:n + 1]) and same(alone["save_mean"], mean[n:n + 1])
            balone = _bwd(hip, x[n:n + 1], dy[n:n + 1], g, mean[n:n + 1], invstd[n:n + 1], row=row)
            assert same(balone["dx"], back[0]["dx"][n:n + 1])
    perm = np.random.default_rng(3).permutation(N)
    fp = _fwd(hip, x[perm], g, b_, eps, off=1)
    assert same(fp["y"], runs[0]["y"][perm]) and same(fp["save_mean"], mean[perm]) and same(fp["save_invstd"], invstd[perm])
    bp = _bwd(hip, x[perm], dy[perm], g, mean[perm], invstd[perm], off=2)
    assert same(bp["dx"], back[0]["dx"][perm])
    ok_p = B.guarded(B.backward(x, dy, g, mean, invstd)["wide_param"], "params")      # the parameters' sums run over the batch: another order
    for name in ("dgamma", "dbeta"):
        assert (_ulps(bp[name], back[0][name])[ok_p] == 0).all() and (_ulps(bp[name], back[0][name]) <= 1).all()


@pytest.mark.parametrize("case", B.OTHER_CASES["one_group"], ids=lambda c: "x".join(map(str, c)))
def test_layer_norm_is_group_norm_with_one_group_and_instance_norm_is_layer_norm(hip, case):
    M, L = case[0], case[2]
    d = B.gaussian_family(*case)
    x, dy, eps = d["x"], d["dy"], d["eps"]
    for scale, shift in ((None, None), (F32(1.5), F32(-0.25))):
        gl, bl = (None, None) if scale is None else (np.full(L, scale, F32), np.full(L, shift, F32))
        gg, bg = (None, None) if scale is None else (np.full(1, scale, F32), np.full(1, shift, F32))
        layer = _fwd(hip, x, gl, bl, eps)
        group = _fwd(hip, x.reshape(M, 1, 1, L), gg, bg, eps, off=1)            # (N, C = 1, inner = L) in one group
        assert same(layer["y"].reshape(-1), group["y"].reshape(-1)) and same(layer["save_mean"], group["save_mean"]) and same(layer["save_invstd"], group["save_invstd"])
        bl_ = _bwd(hip, x, dy, gl, layer["save_mean"], layer["save_invstd"], off=2)
        bg_ = _bwd(hip, x.reshape(M, 1, 1, L), dy.reshape(M, 1, 1, L), gg, layer["save_mean"], layer["save_invstd"], off=3)
        assert same(bl_["dx"].reshape(-1), bg_["dx"].reshape(-1))
    # instance normalization of (N, C, inner) is layer normalization of (N.C, inner), without affine parameters
    for N, Cc in ((1, M),):
        inst = _fwd(hip, x.reshape(N, Cc, 1, L), None, None, eps)
        layer = _fwd(hip, x, None, None, eps, off=1)
        assert same(inst["y"].reshape(-1), layer["y"].reshape(-1)) and same(inst["save_invstd"].reshape(-1), layer["save_invstd"].reshape(-1))
        bi = _bwd(hip, x.reshape(N, Cc, 1, L), dy.reshape(N, Cc, 1, L), None, layer["save_mean"].reshape(N, Cc), layer["save_invstd"].reshape(N, Cc), grads=(False, False))
        bl_ = _bwd(hip, x, dy, None, layer["save_mean"], layer["save_invstd"], off=1, grads=(False, False))
        assert same(bi["dx"].reshape(-1), bl_["dx"].reshape(-1))


# ---- 4. special values --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.OTHER_CASES["special"], ids=lambda c: "x".join(map(str, c)))
def test_a_nan_or_an_inf_poisons_its_row_alone(hip, case):
    shape = case[:4]
    d = B.gaussian_family(*case)
    x, dy, g, b_, eps = d["x"], d["dy"], d["gamma"], d["beta"], d["eps"]
    M, L = shape[0] * shape[1], shape[2] * shape[3]
    others = [r for r in range(M) if r != 1]
    for row in _row_forms(shape):
        clean = _fwd(hip, x, g, b_, eps, row=row)
        bclean = _bwd(hip, x, dy, g, clean["save_mean"], clean["save_invstd"], row=row, grads=(False, False))
        for value in (np.nan, np.inf, -np.inf):
            for at in (0, L // 2, L - 1):
                bad = x.copy()
                bad.reshape(M, L)[1, at] = value
                f = _fwd(hip, bad, g, b_, eps, row=row)
                b = _bwd(hip, bad, dy, g, f["save_mean"], f["save_invstd"], row=row, grads=(False, False))
                assert np.isnan(f["y"].reshape(M, L)[1]).all() and np.isnan(b["dx"].reshape(M, L)[1]).all(), (value, at, row)
                assert same(f["y"].reshape(M, L)[others], clean["y"].reshape(M, L)[others]), (value, at, row)
                assert same(b["dx"].reshape(M, L)[others], bclean["dx"].reshape(M, L)[others]), (value, at, row)
                assert same(f["save_mean"].reshape(M)[others], clean["save_mean"].reshape(M)[others])


def test_rows_of_one_value_and_constant_rows(hip):
    """L = 1 and a constant row: y = beta exactly for eps > 0, NaN for eps = 0"""
    for shape in ((7, 1, 1, 1), (3, 4, 1, 1), (5, 1, 40, 1), (2, 2, 3, 30), (2, 1, 3000, 1), (2, 1, 9000, 1)):
        M, L, P, _ = B.geometry(*shape)
        rng = np.random.default_rng(11)
        x = np.repeat(rng.standard_normal((M, 1)).astype(F32) * 100, L, axis=1).reshape(shape)
        gamma, beta = rng.standard_normal(P).astype(F32), rng.standard_normal(P).astype(F32)
        dy = rng.standard_normal(shape).astype(F32)
        for row in _row_forms(shape):
            f = _fwd(hip, x, gamma, beta, 1e-5, row=row)
            assert (f["y"].reshape(M, L).view(np.uint32) == B._per_row(beta, *shape).view(np.uint32)).all(), (shape, row)
            assert same(f["save_mean"].reshape(-1), x.reshape(M, L)[:, 0]) and same(f["save_invstd"], np.full(shape[:2], F32(1 / np.sqrt(1e-5)), F32))
            if L == 1:      # g - mb = 0 and xh = 0: dx = 0
                assert (_bwd(hip, x, dy, gamma, f["save_mean"], f["save_invstd"], row=row, grads=(False, False))["dx"] == 0).all()
            f0 = _fwd(hip, x, gamma, beta, 0.0, row=row)
            assert np.isnan(f0["y"]).all() and np.isinf(f0["save_invstd"]).all(), (shape, row)
            b0 = _bwd(hip, x, dy, gamma, f0["save_mean"], f0["save_invstd"], row=row)
            assert np.isnan(b0["dx"]).all() and np.isnan(b0["dgamma"]).all() and np.isfinite(b0["dbeta"]).all()


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------------------------------
def test_ndarray_views_and_pending_chains(hip):
    nd = _nd()
    N, G, D, inner, seed, zm = B.OTHER_CASES["surface"][1]                       # group normalization of (4, 6, 3, 5)
    d = B.gaussian_family(N, G, D, inner, seed, zm)
    x4, dy4 = d["x"].reshape(4, 6, 3, 5), d["dy"].reshape(4, 6, 3, 5)
    ref = B.forward(d["x"], d["gamma"], d["beta"], 1e-5)
    bref = B.backward(d["x"], d["dy"], d["gamma"], ref["save_mean"], ref["save_invstd"])
    assert B.guarded(ref["wide"], "forward").all() and B.guarded(bref["wide"], "rows").all() and B.guarded(bref["wide_param"], "params").all()
    y, mean, invstd = nd.dnn_group_norm_forward(_gpu(x4), 3, _gpu(d["gamma"]), _gpu(d["beta"]))
    assert y.shape() == [4, 6, 3, 5] and mean.shape() == [4, 3] and invstd.shape() == [4, 3]
    assert same(y.cpu().numpy().reshape(d["x"].shape), ref["y"]) and same(mean.cpu().numpy(), ref["save_mean"]) and same(invstd.cpu().numpy(), ref["save_invstd"])
    dx, dg, db = nd.dnn_group_norm_backward(_gpu(x4), _gpu(dy4), 3, _gpu(d["gamma"]), mean, invstd)
    assert same(dx.cpu().numpy().reshape(d["x"].shape), bref["dx"]) and same(dg.cpu().numpy(), bref["dgamma"]) and same(db.cpu().numpy(), bref["dbeta"])
    y0 = nd.dnn_group_norm_forward(_gpu(x4), 3)[0]                               # without gamma and beta
    assert same(y0.cpu().numpy().reshape(d["x"].shape), B.apply(d["x"], ref["save_mean"], ref["save_invstd"]))
    inst = nd.dnn_group_norm_forward(_gpu(x4), 6)                                # instance normalization
    assert inst[1].shape() == [4, 6] and same(inst[0].cpu().numpy().reshape(4, 6, 1, 15), B.forward(d["x"].reshape(4, 6, 1, 15))["y"])
    # layer normalization over the last two axes of (6, 5, 7), and over the last axis with an int
    N, G, D, inner, seed, zm = B.OTHER_CASES["surface"][0]
    d2 = B.gaussian_family(N, G, D, inner, seed, zm)
    x3, dy3 = d2["x"].reshape(6, 5, 7), d2["dy"].reshape(6, 5, 7)
    ref2 = B.forward(d2["x"], d2["gamma"], d2["beta"], 1e-5)
    bref2 = B.backward(d2["x"], d2["dy"], d2["gamma"], ref2["save_mean"], ref2["save_invstd"])
    g2, b2 = _gpu(d2["gamma"].reshape(5, 7)), _gpu(d2["beta"].reshape(5, 7))
    y2, m2, i2 = nd.dnn_layer_norm_forward(_gpu(x3), (5, 7), g2, b2)
    assert y2.shape() == [6, 5, 7] and m2.shape() == [6] and same(y2.cpu().numpy().reshape(d2["x"].shape), ref2["y"])
    dx2, dg2, db2 = nd.dnn_layer_norm_backward(_gpu(x3), _gpu(dy3), (5, 7), g2, m2, i2)
    assert dg2.shape() == [5, 7] and same(dx2.cpu().numpy().reshape(d2["x"].shape), bref2["dx"]) and same(dg2.cpu().numpy().reshape(-1), bref2["dgamma"])
    assert same(db2.cpu().numpy().reshape(-1), bref2["dbeta"])
    last = nd.dnn_layer_norm_forward(_gpu(x3), 7)
    assert last[1].shape() == [6, 5] and same(last[0].cpu().numpy().reshape(30, 1, 7, 1), B.forward(d2["x"].reshape(30, 1, 7, 1))["y"])
    whole = nd.dnn_layer_norm_forward(_gpu(x3), (6, 5, 7))                       # the whole array: one row, statistics of shape (1)
    assert whole[1].shape() == [1] and same(whole[0].cpu().numpy().reshape(1, 1, 210, 1), B.forward(d2["x"].reshape(1, 1, 210, 1))["y"])
    # strided views: x given as the transpose of its transposed copy
    x2 = d2["x"].reshape(6, 35)
    xt = nd.transpose(_gpu(np.ascontiguousarray(x2.T)))
    yv = nd.dnn_layer_norm_forward(xt, 35, _gpu(d2["gamma"]), _gpu(d2["beta"]))[0]
    assert same(yv.cpu().numpy().reshape(d2["x"].shape), ref2["y"])
    nd.set_lazy_binding(True)
    try:                                                                         # pending chains
        yp, mp, ip = nd.dnn_layer_norm_forward((_gpu(x2) * 2.0) * 0.5, 35, (_gpu(d2["gamma"]) * 2.0) * 0.5, _gpu(d2["beta"]))
        assert same(yp.cpu().numpy().reshape(d2["x"].shape), ref2["y"])
        dxp = nd.dnn_layer_norm_backward((_gpu(x2) * 2.0) * 0.5, (_gpu(dy3.reshape(6, 35)) * 4.0) * 0.25, 35, _gpu(d2["gamma"]), mp, ip)[0]
        assert same(dxp.cpu().numpy().reshape(d2["x"].shape), bref2["dx"])
        yg = nd.dnn_group_norm_forward((_gpu(x4) * 2.0) * 0.5, 3, _gpu(d["gamma"]), _gpu(d["beta"]))[0]
        assert same(yg.cpu().numpy().reshape(d["x"].shape), ref["y"])
    finally:
        nd.set_lazy_binding(False)


def test_messages_and_nothing_leaks(hip):
    from tests.test_groupnorm_glue_cpu import MESSAGES
    from numpower_amd.ndarray import Error
    nd = _nd()
    ones = lambda *sh: _gpu(np.ones(sh, np.float32))
    cpu = lambda *sh: nd.array(np.ones(sh, np.float32))
    x = ones(2, 6, 4)
    lf, lb, gf, gb = nd.dnn_layer_norm_forward, nd.dnn_layer_norm_backward, nd.dnn_group_norm_forward, nd.dnn_group_norm_backward
    cases = [(lambda: lf(x, (2, 6, 4, 1)), "LN_MSG_NDIM"), (lambda: lf(x, ()), "LN_MSG_NDIM"), (lambda: lf(x, 5), "LN_MSG_SHAPE"),
             (lambda: lf(x, (4, 6)), "LN_MSG_SHAPE"), (lambda: lf(x, 4, ones(5)), "LN_MSG_GAMMA"), (lambda: lf(x, (6, 4), ones(4)), "LN_MSG_GAMMA"),
             (lambda: lf(x, 4, ones(4), ones(4, 1)), "LN_MSG_BETA"), (lambda: lb(x, x, 4, None, ones(2), ones(2, 6)), "LN_MSG_SAVED"),
             (lambda: lb(x, ones(2, 6, 5), 4, None, ones(2, 6), ones(2, 6)), "LN_MSG_GRADIENT"), (lambda: lf(x, 4, eps=-1e-5), "LN_MSG_EPS"),
             (lambda: lf(x, 4, eps=float("nan")), "LN_MSG_EPS"), (lambda: lf(x, 4, cpu(4)), "LN_MSG_DEVICE"),
             (lambda: lb(x, cpu(2, 6, 4), 4, None, ones(2, 6), ones(2, 6)), "LN_MSG_DEVICE"), (lambda: lf(cpu(2, 6, 4), 4), "LN_MSG_CPU"),
             (lambda: gf(ones(6), 1), "GN_MSG_NDIM"), (lambda: gf(x, 0), "GN_MSG_GROUPS"), (lambda: gf(x, -2), "GN_MSG_GROUPS"),
             (lambda: gf(x, 4), "GN_MSG_DIVISIBLE"), (lambda: gf(x, 3, ones(3)), "GN_MSG_GAMMA"), (lambda: gf(x, 3, ones(6), ones(6, 1)), "GN_MSG_BETA"),
             (lambda: gb(x, x, 3, None, ones(2, 6), ones(2, 3)), "GN_MSG_SAVED"), (lambda: gb(x, x, 3, None, ones(6), ones(6)), "GN_MSG_SAVED"),
             (lambda: gb(x, ones(2, 6, 5), 3, None, ones(2, 3), ones(2, 3)), "GN_MSG_GRADIENT"), (lambda: gf(x, 3, eps=-1.0), "GN_MSG_EPS"),
             (lambda: gf(x, 3, cpu(6)), "GN_MSG_DEVICE"), (lambda: gb(x, cpu(2, 6, 4), 3, None, ones(2, 3), ones(2, 3)), "GN_MSG_DEVICE"),
             (lambda: gf(cpu(2, 6, 4), 3), "GN_MSG_CPU")]
    for call, name in cases:
        gc.collect()
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == MESSAGES["NPH_" + name], name
        del e
        gc.collect()
        assert nd.live_device_allocations() == before, name
    _l, lib = _lib()
    gc.collect()
    before, pool = nd.live_device_allocations(), lib.np_live_allocs()
    big = ones(3, 2, 5000)                                                       # the split form and the planes form: scratch for the partials
    results = [lf(x, 4), gf(x, 2), lf(big, (2, 5000)), lb(big, big, (2, 5000), None, ones(3), ones(3)), gb(big, big, 1, None, ones(3, 1), ones(3, 1))]
    assert _probe()[:2] == (B.ROW_SPLIT, B.PARAM_PLANES)
    gc.collect()
    assert nd.live_device_allocations() == before + 1 + 3 * 5                    # big, three results five times
    del results, big
    gc.collect()
    assert nd.live_device_allocations() == before and lib.np_live_allocs() == pool


def test_the_example_trains_a_classifier_with_group_norm(hip):
    """examples/conv_gn_classifier.py: conv -> group norm -> relu -> pool -> conv -> pool -> cross-entropy at a batch size of 2"""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("conv_gn_classifier", Path(__file__).resolve().parent.parent / "examples" / "conv_gn_classifier.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, labels = ex.make_problem(64)
    params, losses = ex.train_gpu(X, labels, 3, 0.05)
    assert np.isfinite(losses).all() and np.mean(losses[-8:]) < 0.5 * np.mean(losses[:8])
    assert [a.shape() for a in params] == [[8, 1, 3, 3], [8], [8], [4, 8, 3, 3], [4]]
    logit = ex.predict(X, params)
    assert logit.shape == (64, 4) and np.isfinite(logit).all()
