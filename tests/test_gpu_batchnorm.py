"""GPU tests of batch normalization (np_batchnorm.hip: np_batchnorm_forward, np_batchnorm_backward; NDArray.dnn_batch_norm_forward /
dnn_batch_norm_backward) against tests/batchnorm_family.py, which tests/test_batchnorm_reference_cpu.py holds to torch.

EVERYTHING is compared bit for bit with the evaluator, Gaussian data included: the statistics are fp64 sums rounded once, and for
every Gaussian case below the CPU tier has shown that no summation order the kernels use can move a rounded scalar (the guard).
No tolerance appears in this file except the example's loss.

Operands sit at float offsets 0 .. 3 inside NaN frames and outputs inside a canary (gemm_family.framed / canary); every case asserts
the kernel form, the launch count and the slice count by the probe, against the dispatcher restated in batchnorm_family.py."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from tests import batchnorm_family as B
from tests import gemm_family as G

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
    b = (C.c_size_t * 5)()
    _l.check(lib.np_debug_batchnorm_bounds(b, 5))
    return tuple(b)


def _probe():
    _l, lib = _lib()
    f, n, s = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    _l.check(lib.np_debug_batchnorm_last_path(C.byref(f), C.byref(n), C.byref(s)))
    return f.value, n.value, s.value


@contextlib.contextmanager
def _forced(form):
    _l, lib = _lib()
    _l.check(lib.np_debug_batchnorm_force_form(-1 if form is None else form))
    try:
        yield
    finally:
        _l.check(lib.np_debug_batchnorm_force_form(-1))


def _forms(N, C_, inner):
    """None (the unforced choice) and every form that can serve the shape"""
    return [None] + [f for f in (B.FORM_ONE, B.FORM_SPLIT, B.FORM_ROWS) if B.serves(f, N, C_, inner, _bounds())]


def _expect_probe(form, N, C_, inner, inference=False):
    """(form, launches, slices) the probe must report for a call forced to `form` (None: unforced)"""
    bounds = _bounds()
    f = B.pick_form(N, C_, inner, bounds) if form is None else form
    if inference:
        f = B.FORM_SPLIT if f == B.FORM_ONE else f
        return B.FORM_APPLY, 1, B.slices(f, N, C_, inner, bounds)
    return f, B.launches(f), B.slices(f, N, C_, inner, bounds)


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())


# ---- the C ABI on host arrays: operands in NaN frames at `off` floats, outputs in a canary ----
class _Call:
    def __init__(self, hip, off=0):
        self.hip, self.off, self.held, self.k = hip, off, [], 0

    def operand(self, a):
        if a is None:
            return None
        self.k += 1
        image, start = G.framed(a, (self.off + self.k) % 4)
        d = self.hip.DeviceArray.from_host(image)
        self.held.append(d)
        return d.ptr + 4 * start

    def output(self, shape, initial=None):
        size = int(np.prod(shape))
        self.k += 1
        image, start = G.canary(size, (self.off + self.k) % 4)
        if initial is not None:
            image[start:start + size] = np.asarray(initial, F32).reshape(-1)
        d = self.hip.DeviceArray.from_host(image)
        self.held.append(d)
        return d.ptr + 4 * start, (d, start, size, shape)

    def take(self, out):
        d, start, size, shape = out
        image = d.to_host()
        assert G.frame_intact(image, start, size), "the output's frame was written"
        return image[start:start + size].reshape(shape)

    def free(self):
        for d in self.held:
            d.free()


def _fwd(hip, x, gamma, beta, eps, training=True, momentum=0.1, rm=None, rv=None, off=0, form=None):
    """np_batchnorm_forward -> dict; the probe must report what the dispatcher says"""
    _l, lib = _lib()
    N, C_, inner = x.shape
    c = _Call(hip, off)
    try:
        px, pg, pb = c.operand(x), c.operand(gamma), c.operand(beta)
        if training:
            prm, orm = c.output((C_,), rm) if rm is not None else (None, None)
            prv, orv = c.output((C_,), rv) if rv is not None else (None, None)
            pm, om = c.output((C_,))
            pi, oi = c.output((C_,))
        else:
            prm, prv, orm, orv, pm, pi = c.operand(rm), c.operand(rv), None, None, None, None
        py, oy = c.output(x.shape)
        with _forced(form):
            _l.check(lib.np_batchnorm_forward(px, pg, pb, N, C_, inner, 1 if training else 0, momentum, eps, prm, prv, py, pm, pi))
        assert _probe() == _expect_probe(form, N, C_, inner, not training), (_probe(), form, x.shape)
        out = {"y": c.take(oy)}
        if training:
            out.update(save_mean=c.take(om), save_invstd=c.take(oi), running_mean=c.take(orm) if orm else None,
                       running_var=c.take(orv) if orv else None)
        return out
    finally:
        c.free()


def _bwd(hip, x, dy, gamma, mean, invstd, off=0, form=None, grads=True, alias=False):
    _l, lib = _lib()
    N, C_, inner = x.shape
    c = _Call(hip, off)
    try:
        px, pg, pm, pi = c.operand(x), c.operand(gamma), c.operand(mean), c.operand(invstd)
        if alias:
            pdx, odx = c.output(x.shape, dy)
            pdy = pdx
        else:
            pdy = c.operand(dy)
            pdx, odx = c.output(x.shape)
        pdg, odg = c.output((C_,)) if grads else (None, None)
        pdb, odb = c.output((C_,)) if grads else (None, None)
        with _forced(form):
            _l.check(lib.np_batchnorm_backward(px, pdy, pg, pm, pi, N, C_, inner, pdx, pdg, pdb))
        assert _probe() == _expect_probe(form, N, C_, inner), (_probe(), form, x.shape)
        return {"dx": c.take(odx), "dgamma": c.take(odg) if grads else None, "dbeta": c.take(odb) if grads else None}
    finally:
        c.free()


# ---- 1. the exact family ---------------------------------------------------------------------------------------------------------------------------------
EXACT = [("pm1", (2, 3, 5), ()), ("pm1", (64, 2, 65), (1,)), ("m3", (4, 3, 7), (0,)), ("m3", (8, 65, 1), (3, 64)), ("pm1", (2, 1, 1), ()),
         ("m3", (64, 3, 16), ()), ("pm1", (1, 2, 4098), ()), ("m3", (4, 2, 2049), (1,)), ("pm1", (5, 3, 4098), ()), ("pm1", (3, 2, 30000), ()),
         ("m3", (1, 1, 200000), ()), ("m3", (200000, 1, 1), ()), ("pm1", (1026, 65, 1), (7,)), ("m3", (36, 65, 1), ())]


@pytest.mark.parametrize("pattern, shape, constant", EXACT, ids=lambda v: str(v).replace(" ", ""))
def test_exact_family_by_bits_in_every_form(hip, pattern, shape, constant):
    d = B.exact_family(*shape, pattern, seed=7, constant=constant)
    x, C_ = d["x"], shape[1]
    rm0, rv0 = np.arange(C_, dtype=F32) - 2, np.arange(C_, dtype=F32) * 0.5 + 1
    ref = B.forward(x, d["gamma"], d["beta"], d["eps"], True, 0.1, rm0, rv0)
    assert same(ref["y"], d["y"]) and same(ref["save_invstd"], d["save_invstd"])      # the closed form, as on the CPU tier
    for k, form in enumerate(_forms(*shape)):
        f = _fwd(hip, x, d["gamma"], d["beta"], d["eps"], True, 0.1, rm0, rv0, off=k, form=form)
        for name in ("y", "save_mean", "save_invstd"):
            assert same(f[name], d[name]), (name, form)
        assert same(f["running_mean"], ref["running_mean"]) and same(f["running_var"], ref["running_var"]), form
        for c in constant:      # eps > 0: y = beta by bits; eps = 0: NaN
            yc = f["y"][:, c, :]
            assert (yc.view(np.uint32) == d["beta"][c:c + 1].view(np.uint32)).all() if d["eps"] > 0 else np.isnan(yc).all()
        b = _bwd(hip, x, d["dy"], d["gamma"], f["save_mean"], f["save_invstd"], off=k + 1, form=form)
        for name in ("dx", "dgamma", "dbeta"):
            assert same(b[name], d[name]), (name, form)
        # inference on the saved statistics: running_var = the biased variance, which the family represents exactly
        finite = np.isfinite(d["save_invstd"])
        var = np.where(finite, d["var"], 1.0).astype(F32)
        inf = _fwd(hip, x, d["gamma"], d["beta"], d["eps"], False, 0.1, f["save_mean"], var, off=k + 2, form=form)
        assert same(inf["y"][:, finite, :], f["y"][:, finite, :]), form
        # the variants of the Gaussian test, here with every value exact
        for m in (0.0, 1.0):
            fm, rmref = _fwd(hip, x, d["gamma"], d["beta"], d["eps"], True, m, rm0, rv0, off=k + 3, form=form), B.forward(x, None, None, d["eps"], True, m, rm0, rv0)
            assert same(fm["y"], d["y"]) and same(fm["running_mean"], rmref["running_mean"]) and same(fm["running_var"], rmref["running_var"]), (m, form)
        fn = _fwd(hip, x, d["gamma"], d["beta"], d["eps"], off=k, form=form)                 # NULL running pointers
        assert same(fn["y"], d["y"]) and same(fn["save_mean"], d["save_mean"]) and same(fn["save_invstd"], d["save_invstd"]), form
        fp = _fwd(hip, x, None, None, d["eps"], off=k + 1, form=form)                        # NULL gamma / beta
        assert same(fp["y"], B.apply(x, d["save_mean"], d["save_invstd"])), form
        fg = _fwd(hip, x, d["gamma"], None, d["eps"], off=k + 2, form=form)
        assert same(fg["y"], B.apply(x, d["save_mean"], d["save_invstd"], d["gamma"])), form
        ba = _bwd(hip, x, d["dy"], d["gamma"], f["save_mean"], f["save_invstd"], off=k + 3, form=form, grads=False, alias=True)
        assert same(ba["dx"], d["dx"]), form                                                   # NULL dgamma / dbeta, dx aliasing dy
        bp, bpref = _bwd(hip, x, d["dy"], None, f["save_mean"], f["save_invstd"], off=k, form=form), B.backward(x, d["dy"], None, d["save_mean"], d["save_invstd"])
        assert same(bp["dx"], bpref["dx"]) and same(bp["dgamma"], d["dgamma"]) and same(bp["dbeta"], d["dbeta"]), form


def test_exact_family_batch_permutation_and_a_channel_alone(hip):
    d = B.exact_family(64, 5, 80, "m3", seed=9)
    x = d["x"]
    f = _fwd(hip, x, d["gamma"], d["beta"], d["eps"])
    perm = np.random.default_rng(3).permutation(64)
    fp = _fwd(hip, x[perm], d["gamma"], d["beta"], d["eps"], off=1)
    assert same(fp["y"], f["y"][perm]) and same(fp["save_mean"], f["save_mean"]) and same(fp["save_invstd"], f["save_invstd"])
    bp = _bwd(hip, x[perm], d["dy"][perm], d["gamma"], f["save_mean"], f["save_invstd"], off=2)
    b = _bwd(hip, x, d["dy"], d["gamma"], f["save_mean"], f["save_invstd"], off=3)
    assert same(bp["dx"], b["dx"][perm]) and same(bp["dgamma"], b["dgamma"]) and same(bp["dbeta"], b["dbeta"])


# ---- 2. Gaussian data, bit for bit under the guard ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.GAUSSIAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_data_by_bits_in_every_form(hip, case):
    N, C_, inner, seed = case
    d = B.gaussian_family(N, C_, inner, seed)
    x, g, b_, eps, rm0, rv0 = d["x"], d["gamma"], d["beta"], d["eps"], d["running_mean"], d["running_var"]
    refs = {m: B.forward(x, g, b_, eps, True, m, rm0, rv0) for m in (0.0, 0.1, 1.0)}
    ref = refs[0.1]
    bref = B.backward(x, d["dy"], g, ref["save_mean"], ref["save_invstd"])
    plain = B.forward(x, None, None, eps)
    bplain = B.backward(x, d["dy"], None, ref["save_mean"], ref["save_invstd"])
    iref = B.forward(x, g, b_, eps, False, 0.1, rm0, rv0)
    for k, form in enumerate(_forms(N, C_, inner)):
        for m in (0.0, 0.1, 1.0):
            f = _fwd(hip, x, g, b_, eps, True, m, rm0, rv0, off=k, form=form)
            for name in ("y", "save_mean", "save_invstd", "running_mean", "running_var"):
                assert same(f[name], refs[m][name]), (name, m, form)
        f = _fwd(hip, x, g, b_, eps, off=k + 1, form=form)                                  # NULL running pointers
        assert same(f["y"], ref["y"]) and same(f["save_mean"], ref["save_mean"]) and same(f["save_invstd"], ref["save_invstd"]), form
        f = _fwd(hip, x, None, None, eps, off=k + 2, form=form)                             # NULL gamma / beta
        assert same(f["y"], plain["y"]), form
        f = _fwd(hip, x, g, None, eps, off=k + 3, form=form)
        assert same(f["y"], B.apply(x, ref["save_mean"], ref["save_invstd"], g, None)), form
        assert same(_fwd(hip, x, g, b_, eps, False, 0.1, rm0, rv0, off=k, form=form)["y"], iref["y"]), form      # inference
        b = _bwd(hip, x, d["dy"], g, ref["save_mean"], ref["save_invstd"], off=k, form=form)
        for name in ("dx", "dgamma", "dbeta"):
            assert same(b[name], bref[name]), (name, form)
        b = _bwd(hip, x, d["dy"], g, ref["save_mean"], ref["save_invstd"], off=k + 1, form=form, grads=False, alias=True)
        assert same(b["dx"], bref["dx"]), form
        b = _bwd(hip, x, d["dy"], None, ref["save_mean"], ref["save_invstd"], off=k + 2, form=form)
        assert same(b["dx"], bplain["dx"]) and same(b["dgamma"], bref["dgamma"]), form


def test_the_large_mean_channel_gives_the_evaluators_invstd(hip):
    """mean 1e4, sigma 1e-3: channel 5 of the (5, 6, 63) case"""
    N, C_, inner, seed = [c for c in B.GAUSSIAN_CASES if c[:3] == (5, 6, 63)][0]
    d = B.gaussian_family(N, C_, inner, seed)
    assert B.MEANS[5 % 3] == 1e4 and B.SIGMAS[(5 // 3) % 2] == 1e-3
    x = np.ascontiguousarray(d["x"][:, 5:6, :])
    ref = B.forward(x, eps=d["eps"])
    for form in _forms(N, 1, inner):
        f = _fwd(hip, x, None, None, d["eps"], form=form)
        assert same(f["save_invstd"], ref["save_invstd"]) and same(f["save_mean"], ref["save_mean"])
        assert abs(1 / float(f["save_invstd"][0]) ** 2 - d["eps"] - 1e-6) < 0.5e-6      # sigma^2 = 1e-6, not the noise of E[x^2] - mean^2


# ---- 3. identities, by bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.OTHER_CASES["identities"], ids=lambda c: "x".join(map(str, c)))
def test_three_runs_and_a_channel_alone(hip, case):
    shape = case[:3]
    d = B.gaussian_family(*case)
    x, g, b_, eps = d["x"], d["gamma"], d["beta"], d["eps"]
    runs = [_fwd(hip, x, g, b_, eps, True, 0.1, d["running_mean"], d["running_var"], off=k) for k in range(3)]
    for r in runs[1:]:
        assert all(same(r[n], runs[0][n]) for n in r)
    back = [_bwd(hip, x, d["dy"], g, runs[0]["save_mean"], runs[0]["save_invstd"], off=k) for k in range(3)]
    for r in back[1:]:
        assert all(same(r[n], back[0][n]) for n in r)
    for c in (0, 4):
        xa, dya = np.ascontiguousarray(x[:, c:c + 1, :]), np.ascontiguousarray(d["dy"][:, c:c + 1, :])
        for form in _forms(shape[0], 1, shape[2]):
            alone = _fwd(hip, xa, g[c:c + 1], b_[c:c + 1], eps, form=form)
            assert same(alone["y"], runs[0]["y"][:, c:c + 1, :]) and same(alone["save_invstd"], runs[0]["save_invstd"][c:c + 1])
            balone = _bwd(hip, xa, dya, g[c:c + 1], alone["save_mean"], alone["save_invstd"], form=form)
            assert same(balone["dx"], back[0]["dx"][:, c:c + 1, :]) and same(balone["dgamma"], back[0]["dgamma"][c:c + 1])


# ---- 4. special values --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.OTHER_CASES["special"], ids=lambda c: "x".join(map(str, c)))
def test_a_nan_or_an_inf_poisons_its_channel_alone(hip, case):
    shape = case[:3]
    d = B.gaussian_family(*case)
    x, g, b_, eps = d["x"], d["gamma"], d["beta"], d["eps"]
    N, C_, inner = shape
    n = N * inner
    for form in _forms(*shape):
        clean = _fwd(hip, x, g, b_, eps, form=form)
        bclean = _bwd(hip, x, d["dy"], g, clean["save_mean"], clean["save_invstd"], form=form)
        for value in (np.nan, np.inf, -np.inf):
            for at in (0, n // 2, n - 1):
                bad = x.copy()
                bad[at // inner, 1, at % inner] = value
                f = _fwd(hip, bad, g, b_, eps, form=form)
                b = _bwd(hip, bad, d["dy"], g, f["save_mean"], f["save_invstd"], form=form)
                assert np.isnan(f["y"][:, 1, :]).all() and np.isnan(b["dx"][:, 1, :]).all(), (value, at, form)
                for c in (0, 2):
                    assert same(f["y"][:, c, :], clean["y"][:, c, :]) and same(b["dx"][:, c, :], bclean["dx"][:, c, :]), (value, at, form)
                    assert same(f["save_mean"][c], clean["save_mean"][c]) and same(b["dgamma"][c], bclean["dgamma"][c])


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------------------------------
def test_ndarray_views_and_pending_chains(hip):
    nd = _nd()
    d = B.gaussian_family(*B.OTHER_CASES["surface"][0])
    x4, dy4 = d["x"].reshape(6, 3, 5, 7), d["dy"].reshape(6, 3, 5, 7)
    ref = B.forward(d["x"], d["gamma"], d["beta"], 1e-5, True, 0.1, d["running_mean"], d["running_var"])
    bref = B.backward(d["x"], d["dy"], d["gamma"], ref["save_mean"], ref["save_invstd"])
    rm, rv = _gpu(d["running_mean"]), _gpu(d["running_var"])
    y, mean, invstd = nd.dnn_batch_norm_forward(_gpu(x4), _gpu(d["gamma"]), _gpu(d["beta"]), rm, rv)
    assert y.shape() == [6, 3, 5, 7] and mean.shape() == [3]
    assert same(y.cpu().numpy().reshape(6, 3, 35), ref["y"]) and same(mean.cpu().numpy(), ref["save_mean"]) and same(invstd.cpu().numpy(), ref["save_invstd"])
    assert same(rm.cpu().numpy(), ref["running_mean"]) and same(rv.cpu().numpy(), ref["running_var"])      # updated in place
    dx, dg, db = nd.dnn_batch_norm_backward(_gpu(x4), _gpu(dy4), _gpu(d["gamma"]), mean, invstd)
    assert same(dx.cpu().numpy().reshape(6, 3, 35), bref["dx"]) and same(dg.cpu().numpy(), bref["dgamma"]) and same(db.cpu().numpy(), bref["dbeta"])
    # inference on the updated running statistics, and without gamma / beta
    iref = B.forward(d["x"], d["gamma"], d["beta"], 1e-5, False, 0.1, ref["running_mean"], ref["running_var"])
    yi = nd.dnn_batch_norm_forward(_gpu(x4), _gpu(d["gamma"]), _gpu(d["beta"]), rm, rv, training=False)
    assert same(yi.cpu().numpy().reshape(6, 3, 35), iref["y"])
    y0 = nd.dnn_batch_norm_forward(_gpu(x4))[0]
    assert same(y0.cpu().numpy().reshape(6, 3, 35), B.forward(d["x"], eps=1e-5)["y"])
    # (N, C): a dense layer's output
    d2 = B.gaussian_family(*B.OTHER_CASES["surface"][1])
    y2, m2, i2 = nd.dnn_batch_norm_forward(_gpu(d2["x"][:, :, 0]), _gpu(d2["gamma"]), _gpu(d2["beta"]))
    assert y2.shape() == [33, 5] and same(y2.cpu().numpy(), B.forward(d2["x"], d2["gamma"], d2["beta"], 1e-5)["y"][:, :, 0])
    # strided views: x given as the transpose of its transposed copy
    xt = nd.transpose(_gpu(np.ascontiguousarray(d2["x"][:, :, 0].T)))
    yv = nd.dnn_batch_norm_forward(xt, _gpu(d2["gamma"]), _gpu(d2["beta"]))[0]
    assert same(yv.cpu().numpy(), y2.cpu().numpy())
    nd.set_lazy_binding(True)
    try:                                                                                     # pending chains
        yp, mp, ip = nd.dnn_batch_norm_forward((_gpu(x4) * 2.0) * 0.5, (_gpu(d["gamma"]) * 2.0) * 0.5, _gpu(d["beta"]))
        assert same(yp.cpu().numpy().reshape(6, 3, 35), ref["y"])
        dxp = nd.dnn_batch_norm_backward((_gpu(x4) * 2.0) * 0.5, (_gpu(dy4) * 4.0) * 0.25, _gpu(d["gamma"]), mp, ip)[0]
        assert same(dxp.cpu().numpy().reshape(6, 3, 35), bref["dx"])
    finally:
        nd.set_lazy_binding(False)


def test_messages_and_nothing_leaks(hip):
    from tests.test_batchnorm_glue_cpu import MESSAGES
    from numpower_amd.ndarray import Error
    nd = _nd()
    ones = lambda *sh: _gpu(np.ones(sh, np.float32))
    cpu = lambda *sh: nd.array(np.ones(sh, np.float32))
    x = ones(2, 3, 4)
    fwd, bwd = nd.dnn_batch_norm_forward, nd.dnn_batch_norm_backward
    cases = [(lambda: fwd(ones(6)), "NDIM"), (lambda: fwd(x, ones(4)), "GAMMA"), (lambda: fwd(x, ones(3), ones(3, 1)), "BETA"),
             (lambda: fwd(x, None, None, ones(4), ones(3)), "RUNNING"), (lambda: fwd(x, None, None, ones(3), ones(2)), "RUNNING"),
             (lambda: fwd(x, training=False), "INFERENCE"), (lambda: fwd(x, None, None, ones(3), None, training=False), "INFERENCE"),
             (lambda: bwd(x, x, None, ones(4), ones(3)), "SAVED"), (lambda: bwd(x, ones(2, 3, 5), None, ones(3), ones(3)), "GRADIENT"),
             (lambda: fwd(x, eps=-1e-5), "EPS"), (lambda: fwd(x, momentum=1.5), "MOMENTUM"), (lambda: fwd(x, momentum=-0.1), "MOMENTUM"),
             (lambda: fwd(x, cpu(3)), "DEVICE"), (lambda: bwd(x, cpu(2, 3, 4), None, ones(3), ones(3)), "DEVICE"),
             (lambda: fwd(cpu(2, 3, 4)), "CPU"), (lambda: fwd(ones(1, 3)), "ONE_VALUE"), (lambda: fwd(ones(1, 3, 1, 1)), "ONE_VALUE"),
             (lambda: fwd(x, eps=float("nan")), "EPS")]
    # NPH_BN_MSG_RUNNING_VIEW has no case: NDArray cannot build a non-contiguous 1-dimensional array (slice copies, $a[i] lays out a
    # fresh header, the transpose of a (C) array is itself), so only a C host that fills the struct itself can reach it
    for call, name in cases:
        gc.collect()
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == MESSAGES["NPH_BN_MSG_" + name], name
        del e
        gc.collect()
        assert nd.live_device_allocations() == before, name
    assert nd.dnn_batch_norm_forward(ones(1, 3), None, None, ones(3), ones(3), training=False).shape() == [1, 3]      # inference with n = 1 is fine
    _l, lib = _lib()
    gc.collect()
    before, pool = nd.live_device_allocations(), lib.np_live_allocs()
    big = ones(3, 2, 5000)                                                                    # the split form: scratch for the partials
    results = [fwd(x), fwd(big), bwd(big, big, None, ones(2), ones(2)), fwd(big, None, None, ones(2), ones(2), training=False)]
    assert _probe()[0] == B.FORM_APPLY
    gc.collect()
    assert nd.live_device_allocations() == before + 1 + 3 + 3 + 3 + 1      # big, three results three times, y
    del results, big
    gc.collect()
    assert nd.live_device_allocations() == before and lib.np_live_allocs() == pool


def test_the_example_trains_a_classifier_with_batch_norm(hip):
    """examples/conv_bn_classifier.py: conv -> batch norm -> relu -> pool -> conv -> pool -> cross-entropy, all on the device"""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("conv_bn_classifier", Path(__file__).resolve().parent.parent / "examples" / "conv_bn_classifier.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, labels = ex.make_problem(128)
    params, running, losses = ex.train_gpu(X, labels, 25, 0.1)
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
    assert [a.shape() for a in params] == [[8, 1, 3, 3], [8], [8], [4, 8, 3, 3], [4]] and [a.shape() for a in running] == [[8], [8]]
    rm, rv = (a.cpu().numpy() for a in running)
    assert np.isfinite(rm).all() and (rv > 0).all() and not (rm == 0).all()                    # the running statistics moved
    logit = ex.predict(X, params, running)
    assert logit.shape == (128, 4) and np.isfinite(logit).all()
