"""GPU tests of softmax, log-softmax and cross-entropy (np_softmax.hip: np_softmax_forward, np_softmax_backward, np_cross_entropy;
NDArray.softmax / log_softmax / softmax_backward / dnn_cross_entropy) against tests/softmax_family.py, which
tests/test_softmax_reference_cpu.py holds to torch: the exact family bit for bit, Gaussian and wide-range data inside the derived
per-element bounds in every form that can serve a shape, the identities of the header bit for bit, the special-value class map,
saturated logits, one case beyond 2^31 elements, and the surface (views, pending chains, messages, no leak, the example).

Operands sit at float offsets 0 .. 3 inside NaN frames and outputs inside a canary (gemm_family.framed / canary); every case asserts
the kernel form by the probe."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from tests import gemm_family as G
from tests import softmax_family as S

pytestmark = pytest.mark.gpu
SHORT, WAVE, BLOCK, STREAM, STRIDED = S.FORM_SHORT, S.FORM_WAVE, S.FORM_BLOCK, S.FORM_STREAM, S.FORM_STRIDED


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
    _l.check(lib.np_debug_softmax_bounds(b, 5))
    return list(b)


def _form():
    _l, lib = _lib()
    f = C.c_int(-1)
    _l.check(lib.np_debug_softmax_last_path(C.byref(f)))
    return f.value


@contextlib.contextmanager
def _forced(form):
    _l, lib = _lib()
    _l.check(lib.np_debug_softmax_force_form(form))
    try:
        yield
    finally:
        _l.check(lib.np_debug_softmax_force_form(-1))


def _natural(cols, inner):
    short, wave, block = _bounds()[:3]
    return STRIDED if inner > 1 else SHORT if cols <= short else WAVE if cols <= wave else BLOCK if cols <= block else STREAM


def _serving(cols, inner, xent=False):
    short, wave, block = _bounds()[:3]
    forms = [f for f, ok in ((SHORT, inner == 1 and cols <= short), (WAVE, inner == 1 and cols <= wave), (BLOCK, inner == 1 and cols <= block),
                             (STREAM, inner == 1), (STRIDED, not xent)) if ok]
    return forms


def _slab_rows(cols):
    _s, _w, _b, slab, most = _bounds()
    return min(most, slab // (cols | 1))


# ---- the C ABI on host arrays: operands in NaN frames at `off` floats, outputs in a canary ----
class _Call:
    def __init__(self, hip, off=0):
        self.hip, self.off, self.held = hip, off, []

    def operand(self, a):
        image, start = G.framed(a, self.off % 4)
        d = self.hip.DeviceArray.from_host(image)
        self.held.append(d)
        return d.ptr + 4 * start

    def output(self, shape):
        size = int(np.prod(shape))
        image, start = G.canary(size, (self.off + 1) % 4)
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


def _fwd(hip, x, mode, off=0, form=None):
    """np_softmax_forward of x (outer, cols, inner) -> y; the probe must report `form`"""
    _l, lib = _lib()
    c = _Call(hip, off)
    try:
        py, out = c.output(x.shape)
        _l.check(lib.np_softmax_forward(c.operand(x), *x.shape, mode, py))
        assert form is None or _form() == form, (_form(), form, x.shape)
        return c.take(out)
    finally:
        c.free()


def _bwd(hip, y, dy, mode, off=0, form=None, alias=False):
    _l, lib = _lib()
    c = _Call(hip, off)
    try:
        if alias:           # dx == dy: the gradient is overwritten in place, inside its NaN frame
            image, start = G.framed(dy, off % 4)
            d = hip.DeviceArray.from_host(image)
            c.held.append(d)
            _l.check(lib.np_softmax_backward(c.operand(y), d.ptr + 4 * start, *y.shape, mode, d.ptr + 4 * start))
            got = d.to_host()
            assert np.isnan(got[:start]).all() and np.isnan(got[start + dy.size:]).all()
            return got[start:start + dy.size].reshape(y.shape)
        px, out = c.output(y.shape)
        _l.check(lib.np_softmax_backward(c.operand(y), c.operand(dy), *y.shape, mode, px))
        assert form is None or _form() == form, (_form(), form, y.shape)
        return c.take(out)
    finally:
        c.free()


def _xent(hip, logits, target, kind, scale=1.0, with_grad=True, off=0, form=None):
    _l, lib = _lib()
    c = _Call(hip, off)
    try:
        rows, cols = logits.shape
        pl, lout = c.output((rows,))
        pg, gout = c.output(logits.shape) if with_grad else (None, None)
        _l.check(lib.np_cross_entropy(c.operand(logits), c.operand(target), rows, cols, kind, scale, pl, pg))
        assert form is None or _form() == form, (_form(), form, logits.shape)
        return c.take(lout), c.take(gout) if with_grad else None
    finally:
        c.free()


def _to3(a, outer, inner):
    """rows (outer . inner, cols) -> (outer, cols, inner)"""
    return np.ascontiguousarray(a.reshape(outer, inner, a.shape[1]).transpose(0, 2, 1))


# ---- 1. the exact family, bit for bit ---------------------------------------------------------------------------------------------------

def _exact_case(hip, outer, cols, inner, seed):
    rng = np.random.default_rng(seed)
    rows, off, form = outer * inner, seed, _natural(cols, inner)
    tag = (outer, cols, inner)
    for filler in ("-inf", "m-200"):
        x, ks, at = S.exact_rows(rng, rows, cols, filler)
        assert S.same(_fwd(hip, _to3(x, outer, inner), S.SOFTMAX, off, form), _to3(S.exact_softmax(ks, at), outer, inner)), ("softmax", filler, tag)
        x, ks, at = S.exact_rows(rng, rows, cols, filler, k_cycle=(1,))
        ly = S.exact_log_softmax(x, ks, at)
        assert S.same(_fwd(hip, _to3(x, outer, inner), S.LOG_SOFTMAX, off + 1, form), _to3(ly, outer, inner)), ("log_softmax", filler, tag)
        dy, dx = S.exact_backward_log_softmax(rng, ly)
        assert S.same(_bwd(hip, _to3(ly, outer, inner), _to3(dy, outer, inner), S.LOG_SOFTMAX, off + 2, form), _to3(dx, outer, inner)), ("log bwd", filler, tag)
        x, ks, at = S.exact_rows(rng, rows, cols, filler, k_cycle=S.EXACT_K_POW2)
        y = S.exact_softmax(ks, at)
        dy, dx = S.exact_backward_softmax(rng, y)
        assert S.same(_bwd(hip, _to3(y, outer, inner), _to3(dy, outer, inner), S.SOFTMAX, off + 3, form), _to3(dx, outer, inner)), ("softmax bwd", filler, tag)
        assert S.same(_bwd(hip, _to3(y, outer, inner), _to3(dy, outer, inner), S.SOFTMAX, off, alias=True), _to3(dx, outer, inner)), ("dx == dy", filler, tag)
        if inner > 1:
            continue
        labels = np.where(np.arange(rows) % 2 == 0, at.argmax(axis=1), (~at).argmax(axis=1))
        for scale in (1.0, 0.125):
            loss, grad = S.exact_cross_entropy(x, ks, at, labels, scale)
            one = ks == 1
            gl, gg = _xent(hip, x, labels.astype(np.float32), S.XENT_INDEX, scale, True, off + 1, form)
            assert S.same(gl[one], loss[one]) and S.same(gg, grad), ("xent index", filler, scale, tag)
            onehot = np.zeros((rows, cols), np.float32)
            onehot[np.arange(rows), labels] = 1.0
            pl, pg = _xent(hip, x, onehot, S.XENT_PROB, scale, True, off + 2, form)
            assert S.same(pl, gl) and S.same(pg, grad), ("xent prob", filler, scale, tag)
            nl, _ = _xent(hip, x, labels.astype(np.float32), S.XENT_INDEX, scale, False, off + 3, form)
            assert S.same(nl, gl), ("xent without a gradient", tag)


def _cols_list():
    short, wave, block = _bounds()[:3]
    cols = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257}
    for b in (short, wave, block):
        cols |= {b - 1, b, b + 1}
    return sorted(cols)


COLS_IDS = list(range(17))       # as many as _cols_list() returns; the list itself needs the library


@pytest.mark.parametrize("which", COLS_IDS)
def test_exact_family_rows_by_bits(hip, which):
    cols_all = _cols_list()
    assert len(cols_all) == len(COLS_IDS)
    cols = cols_all[which]
    R = _slab_rows(cols)
    outers = sorted({1, 2, 255, 256, 257, R - 1, R, R + 1} - {0}) if cols <= 1025 else [1, 2, 5]
    for n, outer in enumerate(outers):
        _exact_case(hip, outer, cols, 1, seed=which * 16 + n)


@pytest.mark.parametrize("inner", [2, 3, 64, 65])
def test_exact_family_strided_by_bits(hip, inner):
    for n, (outer, cols) in enumerate([(1, 1), (2, 2), (3, 3), (1, 5), (2, 64), (33, 4), (2, 65), (1, 257), (3, 1025)]):
        _exact_case(hip, outer, cols, inner, seed=inner * 16 + n)


def test_exact_family_through_ndarray(hip):
    nd = _nd()
    rng = np.random.default_rng(77)
    for shape, axis in (((6, 10), -1), ((6, 10), 0), ((40,), 0), ((3, 7, 5), 1), ((2, 3, 4, 70), -1), ((2, 3, 4, 5), -3)):
        cols = shape[axis]
        outer, inner = int(np.prod(shape[:axis % len(shape)], dtype=np.int64)), int(np.prod(shape[axis % len(shape) + 1:], dtype=np.int64))
        x, ks, at = S.exact_rows(rng, outer * inner, cols, "m-200", k_cycle=S.EXACT_K_POW2)
        shaped = lambda a: _to3(a, outer, inner).reshape(shape)
        y = S.exact_softmax(ks, at)
        assert S.same(nd.softmax(_gpu(shaped(x)), axis).cpu().numpy(), shaped(y)), (shape, axis)
        assert _form() == _natural(cols, inner)
        dy, dx = S.exact_backward_softmax(rng, y)
        assert S.same(nd.softmax_backward(_gpu(shaped(y)), _gpu(shaped(dy)), axis).cpu().numpy(), shaped(dx)), (shape, axis)
        x, ks, at = S.exact_rows(rng, outer * inner, cols, "-inf", k_cycle=(1,))
        ly = S.exact_log_softmax(x, ks, at)
        assert S.same(nd.log_softmax(_gpu(shaped(x)), axis).cpu().numpy(), shaped(ly)), (shape, axis)
        dy, dx = S.exact_backward_log_softmax(rng, ly)
        assert S.same(nd.softmax_backward(_gpu(shaped(ly)), _gpu(shaped(dy)), axis, log=True).cpu().numpy(), shaped(dx)), (shape, axis)
    # cross-entropy: every reduction, with and without the gradient; k == 1 so that the losses are 0 or 200 exactly
    rows, cols = 64, 10
    x, ks, at = S.exact_rows(rng, rows, cols, "m-200", k_cycle=(1,))
    labels = np.where(np.arange(rows) % 4 == 0, (~at).argmax(axis=1), at.argmax(axis=1))      # a quarter of the rows is wrong by 200
    loss, grad = S.exact_cross_entropy(x, ks, at, labels, 1.0)
    gx, gt = _gpu(x), _gpu(labels.astype(np.float32))
    assert S.same(nd.dnn_cross_entropy(gx, gt, "none").cpu().numpy(), loss)
    assert nd.dnn_cross_entropy(gx, gt, "sum") == 200.0 * 16 and nd.dnn_cross_entropy(gx, gt) == 50.0
    for reduction, value, scale in (("none", None, 1.0), ("sum", 3200.0, 1.0), ("mean", 50.0, 1.0 / 64)):
        got, dl = nd.dnn_cross_entropy(gx, gt, reduction, with_grad=True)
        assert (S.same(got.cpu().numpy(), loss) if value is None else got == value) and S.same(dl.cpu().numpy(), grad * np.float32(scale)), reduction
        onehot = np.zeros((rows, cols), np.float32)
        onehot[np.arange(rows), labels] = 1.0
        got, dl = nd.dnn_cross_entropy(gx, _gpu(onehot), reduction, with_grad=True)
        assert (S.same(got.cpu().numpy(), loss) if value is None else got == value) and S.same(dl.cpu().numpy(), grad * np.float32(scale)), reduction


# ---- 2. Gaussian and wide-range data inside the bounds, in every form that serves the shape --------------------------------------------

SHAPES = [(300, 10, 1), (130, 64, 1), (9, 65, 1), (5, 1000, 1), (3, 1025, 1), (2, 9000, 1), (2, 20000, 1), (2, 40000, 1), (3, 21, 70), (2, 300, 5)]


@pytest.mark.parametrize("sigma", [1.0, 30.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_data_is_inside_the_bounds_in_every_form(hip, shape, sigma, capsys):
    outer, cols, inner = shape
    rng = np.random.default_rng(cols + int(sigma))
    x, dy = S.gaussian(rng, shape, sigma), S.gaussian(rng, shape, 1.0)
    labels = rng.integers(0, cols, outer).astype(np.float32)
    prob = rng.random((outer, cols)).astype(np.float32)
    prob = (prob / prob.sum(axis=1, keepdims=True)).astype(np.float32)
    forms = _serving(cols, inner)
    assert forms and _natural(cols, inner) in forms
    worst = {}
    for n, form in enumerate(forms):
        with _forced(form):
            for mode, name in ((S.SOFTMAX, "softmax"), (S.LOG_SOFTMAX, "log_softmax")):
                y = _fwd(hip, x, mode, n, form)
                worst[name, form] = S.worst(y, S.forward(x, mode), S.bound_forward(x, mode, form))
                dx = _bwd(hip, y, dy, mode, n + 1, form)      # from the fp32 output, an exact input of the backward pass
                worst[name + "_bwd", form] = S.worst(dx, S.backward(y, dy, mode), S.bound_backward(y, dy, mode))
            if inner == 1 and form != STRIDED:
                for kind, target, name in ((S.XENT_INDEX, labels, "index"), (S.XENT_PROB, prob, "prob")):
                    loss, grad = _xent(hip, x[:, :, 0], target, kind, 0.5, True, n + 2, form)
                    wl, wg = S.cross_entropy(x[:, :, 0], target, kind, 0.5)
                    bl, bg = S.bound_cross_entropy(x[:, :, 0], target, kind, 0.5, form)
                    worst["loss_" + name, form], worst["grad_" + name, form] = S.worst(loss, wl, bl), S.worst(grad, wg, bg)
    with capsys.disabled():
        print("\n[softmax gpu] %s sigma %g: worst fraction of the bound by form: " % (shape, sigma)
              + ", ".join("%s/%d %.3f" % (k[0], k[1], v) for k, v in sorted(worst.items())))
    for key, w in worst.items():
        assert w <= 1.0, (key, w)


# ---- 3. identities, bit for bit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(37, 10), (6, 300), (3, 3000), (2, 40000)])
def test_identities_by_bits(hip, rows, cols):
    rng = np.random.default_rng(rows * cols)
    x = S.gaussian(rng, (rows, cols), 3.0)
    labels = rng.integers(0, cols, rows)
    form = _natural(cols, 1)
    ls = _fwd(hip, x[:, :, None], S.LOG_SOFTMAX, 1, form)[:, :, 0]
    p = _fwd(hip, x[:, :, None], S.SOFTMAX, 2, form)[:, :, 0]
    loss, grad = _xent(hip, x, labels.astype(np.float32), S.XENT_INDEX, 1.0, True, 3, form)
    assert S.same(loss, (-ls[np.arange(rows), labels]) + np.float32(0.0))      # a zero loss is +0.0
    onehot = np.zeros((rows, cols), np.float32)
    onehot[np.arange(rows), labels] = 1.0
    assert S.same(grad, p - onehot)
    pl, pg = _xent(hip, x, onehot, S.XENT_PROB, 1.0, True, 0, form)
    assert S.same(pl, loss) and S.same(pg, grad)
    for _ in range(2):                                          # three runs are bit-identical
        again = _xent(hip, x, labels.astype(np.float32), S.XENT_INDEX, 1.0, True, 3, form)
        assert S.same(again[0], loss) and S.same(again[1], grad)
        assert S.same(_fwd(hip, x[:, :, None], S.SOFTMAX, 2, form)[:, :, 0], p)
    dy = S.gaussian(rng, (rows, cols), 1.0)
    dx = {m: _bwd(hip, y[:, :, None], dy[:, :, None], m, 1, form)[:, :, 0] for m, y in ((S.SOFTMAX, p), (S.LOG_SOFTMAX, ls))}
    # a row alone equals the same row in a batch of 5, wherever it sits and however it is aligned
    r = rows // 2
    batch = np.concatenate([S.gaussian(rng, (3, cols), 3.0), x[r:r + 1], S.gaussian(rng, (1, cols), 3.0)])
    for off in range(4):
        assert S.same(_fwd(hip, x[r:r + 1, :, None], S.SOFTMAX, off, form)[0, :, 0], p[r])
        assert S.same(_fwd(hip, batch[:, :, None], S.LOG_SOFTMAX, off, form)[3, :, 0], ls[r])
        assert S.same(_bwd(hip, p[r:r + 1, :, None], dy[r:r + 1, :, None], S.SOFTMAX, off, form)[0, :, 0], dx[S.SOFTMAX][r])
        assert S.same(_bwd(hip, ls[r:r + 1, :, None], dy[r:r + 1, :, None], S.LOG_SOFTMAX, off, form)[0, :, 0], dx[S.LOG_SOFTMAX][r])
        one = _xent(hip, x[r:r + 1], labels[r:r + 1].astype(np.float32), S.XENT_INDEX, 1.0, True, off, form)
        assert S.same(one[0], loss[r:r + 1]) and S.same(one[1][0], grad[r])


@pytest.mark.parametrize("outer,cols,inner", [(3, 10, 7), (2, 300, 5), (2, 21, 70)])
def test_the_strided_call_is_the_row_call_on_the_transposed_array(hip, outer, cols, inner):
    rng = np.random.default_rng(cols)
    x = S.gaussian(rng, (outer, cols, inner), 5.0)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(outer * inner, cols, 1)
    for mode in (S.SOFTMAX, S.LOG_SOFTMAX):
        a = _fwd(hip, x, mode, 1, STRIDED)
        b = _fwd(hip, rows, mode, 2, _natural(cols, 1)).reshape(outer, inner, cols).transpose(0, 2, 1)
        bound = S.bound_forward(x, mode, STRIDED) + S.bound_forward(x, mode, _natural(cols, 1))      # each within its own bound of the exact value
        assert np.all(np.abs(a.astype(np.float64) - b) <= bound)


# ---- 4. special values -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols,inner", [(7, 1), (100, 1), (1500, 1), (40000, 1), (7, 3), (100, 2)])
def test_special_values_follow_the_class_map_and_poison_no_other_row(hip, cols, inner):
    x2 = S.special_matrix(cols, reps=inner)                     # (rows, cols): every special row `inner` times
    rows = x2.shape[0]
    outer = rows // inner
    x = _to3(x2, outer, inner)
    clean = [r for r in range(rows) if S.row_class(x2[r]) == "ok"]
    for form in _serving(cols, inner):
        with _forced(form):
            for mode in (S.SOFTMAX, S.LOG_SOFTMAX):
                y = _fwd(hip, x, mode, form, form)
                y2 = np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(rows, cols)
                for r in range(rows):
                    assert S.classes_hold(y2[r], x2[r], mode), (form, mode, r, y2[r][:8])
                if inner == 1:
                    alone = _fwd(hip, x2[clean][:, :, None], mode, 0, form)[:, :, 0]
                    assert S.same(y2[clean], alone), (form, mode)       # the clean rows do not see the poisoned ones
                # backward: a NaN in dy poisons its own row alone
                ok = y2[clean]
                dy = np.ones_like(ok)
                dy[0, cols // 2] = np.nan
                dx = _bwd(hip, ok[:, :, None], dy[:, :, None], mode, 1, form)[:, :, 0]
                assert np.isnan(dx[0]).all() and np.isfinite(dx[1:]).all(), (form, mode)


@pytest.mark.parametrize("cols", [6, 100, 1500, 40000])
def test_an_invalid_label_gives_nan_for_its_row_alone(hip, cols):
    bad = S.INVALID_LABELS + [float(cols), float(cols + 7)]
    rows = 2 * len(bad) + 1
    rng = np.random.default_rng(cols)
    x = S.gaussian(rng, (rows, cols), 2.0)
    good = rng.integers(0, cols, rows).astype(np.float32)
    labels = good.copy()
    labels[1::2] = bad
    form = _natural(cols, 1)
    want_loss, want_grad = _xent(hip, x, good, S.XENT_INDEX, 0.25, True, 1, form)
    loss, grad = _xent(hip, x, labels, S.XENT_INDEX, 0.25, True, 2, form)
    assert np.isnan(loss[1::2]).all() and np.isnan(grad[1::2]).all()
    assert S.same(loss[0::2], want_loss[0::2]) and S.same(grad[0::2], want_grad[0::2]) and np.isfinite(loss[0::2]).all()
    only, _ = _xent(hip, x, labels, S.XENT_INDEX, 0.25, False, 3, form)
    assert S.same(only, loss)
    _l, lib = _lib()
    _l.check(lib.np_sync())                                     # no sticky device error
    # a NaN probability poisons its own row's loss and its own element of the gradient
    prob = np.zeros((rows, cols), np.float32)
    prob[np.arange(rows), good.astype(np.int64)] = 1.0
    prob[3, cols // 2] = np.nan
    pl, pg = _xent(hip, x, prob, S.XENT_PROB, 0.25, True, 0, form)
    assert np.isnan(pl[3]) and np.isnan(pg[3, cols // 2]) and np.isfinite(np.delete(pl, 3)).all() and np.isfinite(np.delete(pg, 3, axis=0)).all()


# ---- 5. saturated logits --------------------------------------------------------------------------------------------------------------------------

def test_saturated_logits_have_a_finite_loss_where_the_composition_has_none(hip):
    nd = _nd()
    rows, cols = 8, 10
    x = np.zeros((rows, cols), np.float32)
    x[:, 0] = 200.0                                             # confident, and wrong for the odd rows
    labels = np.where(np.arange(rows) % 2 == 0, 0, 3)
    onehot = np.zeros((rows, cols), np.float32)
    onehot[np.arange(rows), labels] = 1.0
    want, want_grad = S.cross_entropy(x, labels.astype(np.float32), S.XENT_INDEX)
    assert np.array_equal(want, np.where(labels == 0, 0.0, 200.0))
    gx = _gpu(x)
    loss, grad = nd.dnn_cross_entropy(gx, _gpu(labels.astype(np.float32)), "none", with_grad=True)
    bl, bg = S.bound_cross_entropy(x, labels.astype(np.float32), S.XENT_INDEX)
    assert S.worst(loss.cpu().numpy(), want, bl) <= 1.0 and S.worst(grad.cpu().numpy(), want_grad, bg) <= 1.0
    assert nd.dnn_cross_entropy(gx, _gpu(onehot), "mean") == 100.0
    # the composition examples/softmax_regression.py uses: max, two chains, the loss chain
    from numpower_amd.lazy import Lazy  # noqa: F401  (installs NDArray.lazy)
    row_max = nd.reshape(nd.max(gx, 1), [rows, 1])
    row_sum = nd.reshape((gx.lazy() - row_max).exp().sum(axis=1), [rows, 1])
    P = ((gx.lazy() - row_max).exp() / row_sum).eval()
    by_hand = -(P.lazy().log() * _gpu(onehot)).sum()
    assert not np.isfinite(by_hand)


# ---- 6. large sizes ----------------------------------------------------------------------------------------------------------------------------------

def test_beyond_2_31_elements_and_the_refusal_of_2_31_columns(hip):
    _l, lib = _lib()
    cols = 2048
    rows = (1 << 31) // cols + 3                                # 2^31 + 6144 elements; more rows than the grid's cap, so the row loop turns
    n = rows * cols
    x, y, want = (hip.DeviceArray((n,)) for _ in range(3))
    try:
        _l.check(lib.np_fill(x.ptr, 0.5, n))
        _l.check(lib.np_fill(y.ptr, -1.0, n))
        _l.check(lib.np_fill(want.ptr, 1.0 / cols, n))
        _l.check(lib.np_softmax_forward(x.ptr, rows, cols, 1, S.SOFTMAX, y.ptr))
        assert _form() == BLOCK
        differs = C.c_int(-1)
        _l.check(lib.np_count_mismatch(0, y.ptr, want.ptr, n, 0.0, 0.0, C.byref(differs)))
        assert differs.value == 0
        assert (y.view(n - 16, (16,)).to_host() == np.float32(1.0 / cols)).all()
        for big in (1 << 31, (1 << 31) + 1, 1 << 33):
            assert lib.np_softmax_forward(x.ptr, 1, big, 1, S.SOFTMAX, y.ptr) == -1 and b"2^31 or more" in lib.np_last_error()
            assert lib.np_cross_entropy(x.ptr, want.ptr, 1, big, 0, 1.0, y.ptr, None) == -1 and b"2^31 or more" in lib.np_last_error()
    finally:
        for d in (x, y, want):
            d.free()


# ---- 7. the surface -------------------------------------------------------------------------------------------------------------------------------------

def test_views_and_pending_chains_as_operands(hip):
    nd = _nd()
    rng = np.random.default_rng(21)
    x, dy = S.gaussian(rng, (6, 33), 2.0), S.gaussian(rng, (6, 33), 1.0)
    labels = rng.integers(0, 33, 6).astype(np.float32)
    y = nd.softmax(_gpu(x)).cpu().numpy()
    dx = nd.softmax_backward(_gpu(y), _gpu(dy)).cpu().numpy()
    loss, grad = nd.dnn_cross_entropy(_gpu(x), _gpu(labels), "none", with_grad=True)
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    xt, dyt, yt = (nd.transpose(_gpu(np.ascontiguousarray(a.T))) for a in (x, dy, y))      # strided views
    assert S.same(nd.softmax(xt).cpu().numpy(), y) and S.same(nd.softmax(xt, -1).cpu().numpy(), y)
    assert S.same(nd.softmax_backward(yt, dyt).cpu().numpy(), dx)
    vl, vg = nd.dnn_cross_entropy(xt, _gpu(labels), "none", with_grad=True)
    assert S.same(vl.cpu().numpy(), loss) and S.same(vg.cpu().numpy(), grad)
    along0 = nd.softmax(nd.transpose(_gpu(x)), 0).cpu().numpy()                              # the view's own axis 0: the strided form
    assert _form() == STRIDED and S.worst(along0.T, S.forward(x[:, :, None], S.SOFTMAX)[:, :, 0], S.bound_forward(x[:, :, None], S.SOFTMAX, STRIDED)[:, :, 0]) <= 1.0
    nd.set_lazy_binding(True)
    try:
        assert S.same(nd.softmax((_gpu(x) * 2.0) * 0.5).cpu().numpy(), y)                    # pending chains
        assert S.same(nd.softmax_backward((_gpu(y) * 2.0) * 0.5, (_gpu(dy) * 4.0) * 0.25).cpu().numpy(), dx)
        pl, pg = nd.dnn_cross_entropy((_gpu(x) * 2.0) * 0.5, (_gpu(labels) * 2.0) * 0.5, "none", with_grad=True)
        assert S.same(pl.cpu().numpy(), loss) and S.same(pg.cpu().numpy(), grad)
    finally:
        nd.set_lazy_binding(False)
    # the reductions: the library's own sum of the rows' losses; the mean divides it once
    total = nd.dnn_cross_entropy(_gpu(x), _gpu(labels), "sum")
    assert np.float32(total) == np.float32(nd.sum(_gpu(loss)))
    mean, mg = nd.dnn_cross_entropy(_gpu(x), _gpu(labels), with_grad=True)
    assert np.float32(mean) == np.float32(total) / np.float32(6)
    onehot = np.zeros_like(x)
    onehot[np.arange(6), labels.astype(np.int64)] = 1.0
    assert S.same(mg.cpu().numpy(), (y - onehot) * (np.float32(1.0) / np.float32(6)))


def test_messages_and_nothing_leaks(hip):
    from tests.test_softmax_glue_cpu import MESSAGES
    from numpower_amd.ndarray import Error
    nd = _nd()
    ones = lambda *sh: _gpu(np.ones(sh, np.float32))
    cpu = lambda *sh: nd.array(np.ones(sh, np.float32))
    x, logits = ones(2, 3, 4), ones(4, 6)
    cases = [(lambda: nd.softmax(x, 3), "SOFTMAX_MSG_AXIS"), (lambda: nd.log_softmax(x, -4), "SOFTMAX_MSG_AXIS"),
             (lambda: nd.softmax_backward(x, ones(2, 3, 5)), "SOFTMAX_MSG_GRADIENT"), (lambda: nd.softmax_backward(x, ones(24), log=True), "SOFTMAX_MSG_GRADIENT"),
             (lambda: nd.softmax_backward(x, cpu(2, 3, 4)), "SOFTMAX_MSG_DEVICE"), (lambda: nd.softmax_backward(cpu(2, 3, 4), x), "SOFTMAX_MSG_DEVICE"),
             (lambda: nd.softmax(cpu(2, 3, 4)), "SOFTMAX_MSG_CPU"), (lambda: nd.softmax_backward(cpu(2, 3, 4), cpu(2, 3, 4)), "SOFTMAX_MSG_CPU"),
             (lambda: nd.dnn_cross_entropy(ones(24), ones(4)), "XENT_MSG_LOGITS"), (lambda: nd.dnn_cross_entropy(logits, ones(5)), "XENT_MSG_TARGET"),
             (lambda: nd.dnn_cross_entropy(logits, ones(4, 5), with_grad=True), "XENT_MSG_TARGET"),
             (lambda: nd.dnn_cross_entropy(logits, cpu(4)), "XENT_MSG_DEVICE"), (lambda: nd.dnn_cross_entropy(cpu(4, 6), ones(4, 6), with_grad=True), "XENT_MSG_DEVICE"),
             (lambda: nd.dnn_cross_entropy(cpu(4, 6), cpu(4), "sum", with_grad=True), "XENT_MSG_CPU")]
    for call, name in cases:
        gc.collect()
        before = nd.live_device_allocations()
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == MESSAGES["NPH_" + name]
        del e
        gc.collect()
        assert nd.live_device_allocations() == before, name
    _l, lib = _lib()
    gc.collect()
    before, pool = nd.live_device_allocations(), lib.np_live_allocs()
    t = ones(4)
    results = [nd.softmax(x, 1), nd.log_softmax(x), nd.softmax_backward(x, x), nd.dnn_cross_entropy(logits, t, "none"),
               nd.dnn_cross_entropy(logits, t, "mean"), nd.dnn_cross_entropy(logits, t, "sum", with_grad=True)]
    gc.collect()
    assert nd.live_device_allocations() == before + 1 + 4 + 1      # t, four arrays, one gradient; the rows' losses of a sum or a mean are gone
    assert results[0].shape() == [2, 3, 4] and results[3].shape() == [4] and isinstance(results[4], float) and results[5][1].shape() == [4, 6]
    assert np.array_equal(results[0].cpu().numpy(), np.full((2, 3, 4), np.float32(1) / np.float32(3)))
    del results, t
    gc.collect()
    assert nd.live_device_allocations() == before and lib.np_live_allocs() == pool


def test_the_example_trains_a_classifier_with_the_cross_entropy(hip):
    """examples/conv_softmax_classifier.py: the network of conv_pool_classifier.py under dnn_cross_entropy(..., with_grad=True)"""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("conv_softmax_classifier", Path(__file__).resolve().parent.parent / "examples" / "conv_softmax_classifier.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    X, labels = ex.make_problem(128)
    params, losses, logit = ex.train_gpu(X, labels, 25, 0.1)
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
    assert [a.shape() for a in params] == [[8, 1, 3, 3], [8], [4, 8, 3, 3], [4]]
    assert logit.shape == (128, 4) and np.mean(np.argmax(logit, axis=1) == labels) > 0.9
