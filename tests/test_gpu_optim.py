"""GPU tests of the optimizer steps (np_optim.hip: np_sgd_step, np_adam_step, np_grad_norm; NDArray.dnn_sgd_step / dnn_adam_step /
dnn_grad_norm; numpower_amd/optim.py) against tests/optim_family.py, which tests/test_optim_reference_cpu.py holds to torch.

EVERYTHING is compared bit for bit with the evaluator: the element is a chain of separately rounded fp32 operations, and for every
norm case the CPU tier has shown that no summation order can move the rounded norm (the guard).  No tolerance appears in this file
except the example's loss.

A call's tensors sit in ONE allocation, each behind and before at least four NaNs and at a chosen residue (float offset 0 .. 3 from
a 16-byte boundary); the whole allocation is compared with its expected image, so one float written outside a tensor fails.  Every
call asserts launches, chunks and the tensors by access form by the probe, against the dispatcher restated in optim_family.py."""
import contextlib
import ctypes as C
import gc
import itertools
import math

import numpy as np
import pytest

from tests import optim_family as fam

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK, MOST = fam.CHUNK, fam.MAX_TENSORS
SGD_FORMS = (dict(), dict(weight_decay=0.05), dict(momentum=0.9), dict(momentum=0.9, dampening=0.25, weight_decay=0.05),
             dict(momentum=0.8, nesterov=True, weight_decay=0.01))
ADAM_FORMS = (dict(), dict(weight_decay=0.05), dict(decoupled=True, weight_decay=0.05), dict(betas=(0.5, 0.75), eps=1e-3))


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _probe():
    _l, lib = _lib()
    n, c, v, s = C.c_int(-1), C.c_size_t(0), C.c_int(-1), C.c_int(-1)
    _l.check(lib.np_debug_optim_last_path(C.byref(n), C.byref(c), C.byref(v), C.byref(s)))
    return n.value, c.value, v.value, s.value


@contextlib.contextmanager
def _scalar(on=True):
    _l, lib = _lib()
    _l.check(lib.np_debug_optim_force_scalar(1 if on else 0))
    try:
        yield
    finally:
        _l.check(lib.np_debug_optim_force_scalar(0))


@contextlib.contextmanager
def _cus(n):
    _l, lib = _lib()
    _l.check(lib.np_debug_set_cus(n))
    try:
        yield
    finally:
        _l.check(lib.np_debug_set_cus(0))


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())


def test_the_library_reports_the_familys_constants(hip):
    _l, lib = _lib()
    b = (C.c_size_t * 5)()
    _l.check(lib.np_debug_optim_bounds(b, 5))
    assert tuple(b) == fam.BOUNDS


# ---- the C ABI: every tensor of a call inside one NaN-framed allocation ----
class Arena:
    def __init__(self, hip):
        self.hip, self.items, self.size = hip, [], 8

    def place(self, data, residue=0):
        """-> the index of the tensor; it starts `residue` floats after a 16-byte boundary, at least four NaNs after the one before"""
        data = np.asarray(data, F32).reshape(-1)
        start = -(-self.size // 4) * 4 + 4 + residue
        self.items.append((start, data))
        self.size = start + data.size + 4
        return len(self.items) - 1

    def upload(self):
        self.image = np.full(-(-self.size // 4) * 4 + 8, np.nan, F32)
        for start, data in self.items:
            self.image[start:start + data.size] = data
        self.dev = self.hip.DeviceArray.from_host(self.image)
        assert self.dev.ptr % 16 == 0
        return self

    def ptr(self, i):
        return self.dev.ptr + 4 * self.items[i][0]

    def expect(self, i, data):
        start, old = self.items[i]
        assert np.asarray(data).size == old.size
        self.image[start:start + old.size] = np.asarray(data, F32).reshape(-1)

    def check(self, what=""):
        got = self.dev.to_host()
        assert same(got, self.image), (what, np.flatnonzero(~((got.view(np.uint32) == self.image.view(np.uint32)) | (np.isnan(got) & np.isnan(self.image))))[:8])


def _vec(values):
    return (C.c_void_p * len(values))(*values)


def _sizes(values):
    return (C.c_size_t * len(values))(*values)


class Problem:
    """T tensors with their states in an arena.  residues[t] = (p, g, s1, s2) float offsets"""

    def __init__(self, hip, counts, states, seed=0, residues=None, data=None, scale=None):
        rng = np.random.default_rng(seed)
        self.counts, self.states, self.arena, self.T = list(counts), states, Arena(hip), len(counts)
        self.p, self.g, self.s = [], [], [[] for _ in range(states)]
        self.ip, self.ig, self.is_ = [], [], [[] for _ in range(states)]
        for t, n in enumerate(counts):
            r = residues[t] if residues is not None else (0, 0, 0, 0)
            d = data[t] if data is not None else None
            self.p.append(fam.gaussian(rng, n) if d is None else np.asarray(d[0], F32))
            self.g.append(fam.gaussian(rng, n) if d is None else np.asarray(d[1], F32))
            self.ip.append(self.arena.place(self.p[t], r[0]))
            self.ig.append(self.arena.place(self.g[t], r[1]))
            for k in range(states):
                init = np.abs(fam.gaussian(rng, n)) * F32(0.01) if d is None else np.asarray(d[2 + k], F32)
                self.s[k].append(init)
                self.is_[k].append(self.arena.place(init, r[2 + k]))
        self.iscale = self.arena.place([scale], 1) if scale is not None else None
        self.scale = None if scale is None else F32(scale)
        self.arena.upload()

    def tensors(self):
        """[(n, addresses)] for the restated dispatcher"""
        a = self.arena
        return [(n, [a.ptr(self.ip[t]), a.ptr(self.ig[t])] + [a.ptr(self.is_[k][t]) for k in range(self.states)])
                for t, n in enumerate(self.counts)]

    def lists(self, order=None):
        order = range(self.T) if order is None else order
        a = self.arena
        return (_vec([a.ptr(self.ip[t]) for t in order]), _vec([a.ptr(self.ig[t]) for t in order]),
                [_vec([a.ptr(self.is_[k][t]) for t in order]) for k in range(self.states)], _sizes([self.counts[t] for t in order]))

    def scale_ptr(self):
        return None if self.iscale is None else self.arena.ptr(self.iscale)

    def sgd(self, order=None, first_step=False, force_scalar=False, **hp):
        _l, lib = _lib()
        p, g, s, n = self.lists(order)
        mu = hp.get("momentum", 0.0)
        _l.check(lib.np_sgd_step(p, g, s[0] if self.states else None, n, self.T, hp.get("lr", 0.1), mu, hp.get("dampening", 0.0),
                                 hp.get("weight_decay", 0.0), 1 if hp.get("nesterov") else 0, 1 if first_step else 0, self.scale_ptr()))
        assert _probe() == fam.plan(self.tensors() if mu != 0.0 else [(n_, a[:2]) for n_, a in self.tensors()], force_scalar)
        for t in range(self.T):
            self.p[t], b = fam.sgd_step(self.p[t], self.g[t], self.s[0][t] if self.states else None, first_step=first_step, scale=self.scale, **hp)
            self.arena.expect(self.ip[t], self.p[t])
            if b is not None:
                self.s[0][t] = b
                self.arena.expect(self.is_[0][t], b)

    def adam(self, step, order=None, force_scalar=False, **hp):
        _l, lib = _lib()
        p, g, s, n = self.lists(order)
        betas = hp.get("betas", (0.9, 0.999))
        _l.check(lib.np_adam_step(p, g, s[0], s[1], n, self.T, step, hp.get("lr", 1e-3), betas[0], betas[1], hp.get("eps", 1e-8),
                                  hp.get("weight_decay", 0.0), 1 if hp.get("decoupled") else 0, self.scale_ptr()))
        assert _probe() == fam.plan(self.tensors(), force_scalar)
        for t in range(self.T):
            self.p[t], self.s[0][t], self.s[1][t] = fam.adam_step(self.p[t], self.g[t], self.s[0][t], self.s[1][t], step, scale=self.scale, **hp)
            for i, v in ((self.ip[t], self.p[t]), (self.is_[0][t], self.s[0][t]), (self.is_[1][t], self.s[1][t])):
                self.arena.expect(i, v)


SEAM_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK + 1)


@pytest.mark.parametrize("scale", (None, 0.37))
@pytest.mark.parametrize("form", range(len(SGD_FORMS)))
def test_sgd_in_its_five_forms_over_the_seam_sizes_first_step_then_four(hip, form, scale):
    hp = SGD_FORMS[form]
    pr = Problem(hip, SEAM_COUNTS, 1 if hp.get("momentum") else 0, seed=form, scale=scale)
    for k in range(5):                                          # first_step followed by four steps equals the evaluator's five
        pr.sgd(first_step=k == 0, lr=0.05, **hp)
        pr.arena.check((form, k))


@pytest.mark.parametrize("scale", (None, 0.37))
@pytest.mark.parametrize("form", range(len(ADAM_FORMS)))
def test_adam_and_adamw_with_and_without_l2_over_the_seam_sizes(hip, form, scale):
    pr = Problem(hip, SEAM_COUNTS, 2, seed=10 + form, scale=scale)
    for step in (1, 2, 3):
        pr.adam(step, lr=0.01, **ADAM_FORMS[form])
        pr.arena.check((form, step))


@pytest.mark.parametrize("T", (1, 2, 3, MOST - 1, MOST, MOST + 1, 2 * MOST + 1))
def test_list_lengths_around_the_launch_capacity_with_one_element_tensors_among_multi_chunk_ones(hip, T):
    counts = [(1, 2 * CHUNK + 3, 5, CHUNK + 1)[t % 4] if t % 16 < 4 else 1 + t % 3 for t in range(T)]
    pr = Problem(hip, counts, 2, seed=T)
    pr.adam(2, lr=0.01, weight_decay=0.05)
    assert _probe()[0] == -(-T // MOST)
    pr.arena.check(T)
    pr = Problem(hip, counts, 1, seed=T, scale=0.5)
    pr.sgd(lr=0.05, momentum=0.9)
    pr.arena.check(T)


def test_a_grid_smaller_than_the_chunk_count(hip):
    counts = [2 * CHUNK + 1, 1, 3 * CHUNK, 7, CHUNK + 5, 5 * CHUNK - 1]
    with _cus(1):
        pr = Problem(hip, counts, 2, seed=3)
        pr.adam(1, lr=0.01)
        chunks = _probe()[1]
        assert chunks == sum(-(-n // CHUNK) for n in counts) and fam.grid(chunks, 1) == 9 < chunks
        pr.arena.check()
        norm = _norm_call(hip, [pr.g[t] for t in range(pr.T)], 1.0)
    assert same(norm, fam.grad_norm(pr.g, 1.0)[0])


RESIDUES = list(itertools.product(range(4), repeat=2))


@pytest.mark.parametrize("which", ("p-g", "m-v"))
def test_every_combination_of_pointer_residues(hip, which):
    """(p, g) at every pair of float offsets with the states aligned, (m, v) at every pair with p and g aligned: 16 tensors each,
    in one list, so the access form is chosen per tensor"""
    res = [(a, b, 0, 0) if which == "p-g" else (0, 0, a, b) for a, b in RESIDUES]
    counts = [(2 * CHUNK - 3, 9, CHUNK, 5)[i % 4] for i in range(16)]
    pr = Problem(hip, counts, 2, seed=21, residues=res)
    pr.adam(1, lr=0.01, weight_decay=0.05)
    assert _probe()[2:] == (1, 15)                              # only (0, 0, 0, 0) has every pointer congruent mod 16
    pr.arena.check(which)
    if which == "p-g":                                          # plain SGD has no states: the four congruent pairs are served wide
        pr = Problem(hip, counts, 0, seed=22, residues=res)
        pr.sgd(lr=0.05, weight_decay=0.05)
        assert _probe()[2:] == (4, 12)
        pr.arena.check("sgd")


@pytest.mark.parametrize("residue", range(4))
def test_congruent_pointers_at_every_residue_and_the_forced_scalar_form_by_bits(hip, residue):
    counts = [1, 2, 3, 4, 5, 7, 8, 9, CHUNK - residue, CHUNK - residue + 1, 2 * CHUNK + 1]
    images = []
    for forced in (False, True):
        pr = Problem(hip, counts, 2, seed=30, residues=[(residue,) * 4] * len(counts), scale=1.5)
        with _scalar(forced):
            pr.adam(3, force_scalar=forced, lr=0.01, decoupled=True, weight_decay=0.1)
        assert _probe()[2:] == ((0, len(counts)) if forced else (len(counts), 0))
        pr.arena.check((residue, forced))
        images.append(pr.arena.dev.to_host())
    assert same(*images)


def test_identities_by_bits(hip):
    counts = [CHUNK + 3, 1, 7, 2 * CHUNK, 33]
    base = Problem(hip, counts, 2, seed=40)
    base.adam(2, lr=0.01, weight_decay=0.05)
    base.arena.check()
    want = [(base.p[t], base.s[0][t], base.s[1][t]) for t in range(5)]
    for t in range(5):                                          # a tensor alone equals the same tensor in a list of 5
        full = Problem(hip, counts, 2, seed=40)
        alone = Problem(hip, [counts[t]], 2, data=[(full.p[t], full.g[t], full.s[0][t], full.s[1][t])])
        alone.adam(2, lr=0.01, weight_decay=0.05)
        alone.arena.check()
        assert all(same(a, b) for a, b in zip((alone.p[0], alone.s[0][0], alone.s[1][0]), want[t]))
    perm = Problem(hip, counts, 2, seed=40)                     # list order permuted
    perm.adam(2, order=[3, 0, 4, 2, 1], lr=0.01, weight_decay=0.05)
    perm.arena.check()
    images = []
    for _ in range(3):                                          # three runs give the same bits
        pr = Problem(hip, counts, 2, seed=40)
        pr.adam(2, lr=0.01, weight_decay=0.05)
        images.append(pr.arena.dev.to_host())
    assert same(images[0], images[1]) and same(images[0], images[2]) and same(images[0], base.arena.dev.to_host()) and same(images[0], perm.arena.dev.to_host())
    a, b = Problem(hip, counts, 1, seed=41, scale=1.0), Problem(hip, counts, 1, seed=41)      # grad_scale = 1.0 equals no grad_scale
    a.sgd(lr=0.05, momentum=0.9, weight_decay=0.01)
    b.sgd(lr=0.05, momentum=0.9, weight_decay=0.01)
    assert all(same(x, y) for x, y in zip(a.p + a.s[0], b.p + b.s[0]))
    a, b = Problem(hip, counts, 2, seed=42), Problem(hip, counts, 2, seed=42)                 # decoupled with wd = 0 equals Adam
    a.adam(1, decoupled=True)
    b.adam(1)
    a.arena.check(), b.arena.check()
    assert same(a.arena.dev.to_host(), b.arena.dev.to_host())


@pytest.mark.parametrize("n", (1, 7, CHUNK + 1))
def test_the_exact_family_equals_its_closed_form(hip, n):
    f = fam.exact_family(n)
    s = f["sgd"]
    pr = Problem(hip, [n], 1, data=[(s["p0"], s["g"], np.zeros(n, F32))])
    for k in range(5):
        pr.sgd(first_step=k == 0, lr=s["lr"], momentum=s["momentum"])
        pr.arena.check(k)
        assert same(pr.p[0], s["closed"][k][0]) and same(pr.s[0][0], s["closed"][k][1])
    a = f["adam"]
    pr = Problem(hip, [n], 2, data=[(a["p0"], a["g"], np.zeros(n, F32), np.zeros(n, F32))])
    pr.adam(1, lr=a["lr"], betas=a["betas"], eps=a["eps"])
    pr.arena.check()
    assert all(same(x, y) for x, y in zip((pr.p[0], pr.s[0][0], pr.s[1][0]), a["closed"]))


def test_special_values(hip):
    n = CHUNK + 9
    rng = np.random.default_rng(50)
    for bad in (np.nan, np.inf, -np.inf):                       # reaches that element alone: the first, a middle and the last
        g = fam.gaussian(rng, n)
        g[[0, n // 2, n - 1]] = bad
        pr = Problem(hip, [n, 5], 2, data=[(fam.gaussian(rng, n), g, np.zeros(n, F32), np.zeros(n, F32)),
                                           (np.ones(5, F32), np.ones(5, F32), np.zeros(5, F32), np.zeros(5, F32))], scale=0.5)
        pr.adam(1, lr=0.01, weight_decay=0.05)
        pr.arena.check(bad)
        assert np.flatnonzero(~np.isfinite(pr.p[0])).tolist() == [0, n // 2, n - 1] and np.isfinite(pr.p[1]).all()
        pr = Problem(hip, [n], 1, data=[(fam.gaussian(rng, n), g, np.zeros(n, F32))])
        pr.sgd(first_step=True, lr=0.05, momentum=0.9, nesterov=True)
        pr.arena.check(bad)
        assert np.flatnonzero(~np.isfinite(pr.p[0])).tolist() == [0, n // 2, n - 1]
    p = np.array([np.inf, -np.inf, 1.0, -0.0, 0.0], F32)         # wd = 0 with p = +-Inf leaves g untouched; -0.0 gradients
    g = np.array([1.0, 2.0, -0.0, -0.0, -0.0], F32)
    pr = Problem(hip, [5], 1, data=[(p, g, np.zeros(5, F32))])
    pr.sgd(first_step=True, lr=0.5, momentum=0.9)
    pr.arena.check()
    assert same(pr.s[0][0], g) and same(pr.p[0], np.array([np.inf, -np.inf, 1.0, 0.0, 0.0], F32))
    g = np.array([0.0, 1.0, -0.0, 2.0], F32)                     # eps = 0 with v = 0 gives NaN for that element alone
    pr = Problem(hip, [4], 2, data=[(np.ones(4, F32), g, np.zeros(4, F32), np.zeros(4, F32))])
    pr.adam(1, eps=0.0)
    pr.arena.check()
    assert np.isnan(pr.p[0]).tolist() == [True, False, True, False]
    # denormal gradients and moments, and a denormal v.  (The square root of an fp32 denormal is a normal number, 2^-74.5 at the
    # least, so "sqrt(v) denormal" cannot occur; what can go wrong is a square root or a division that flushes its denormal INPUT.)
    n = 300
    g = (fam.gaussian(rng, n) * F32(1e-39)).astype(F32)
    v = np.full(n, 1e-44, F32)
    v[::3] = np.float32(2.0 ** -140) * F32(3.0)
    v[1::3] = np.float32(2.0 ** -149)
    assert (np.abs(g[g != 0]) < np.finfo(F32).tiny).all() and (v < np.finfo(F32).tiny).all() and (v > 0).all()
    pr = Problem(hip, [n], 2, data=[(fam.gaussian(rng, n), g, g.copy(), v)])
    pr.adam(4, lr=0.01, eps=0.0, betas=(0.5, 0.75))
    pr.arena.check("denormal")
    assert (np.abs(pr.s[0][0][pr.s[0][0] != 0]) < np.finfo(F32).tiny).all() and (pr.s[1][0] > 0).any()
    pr = Problem(hip, [n], 1, data=[(np.zeros(n, F32), g, g.copy())])
    pr.sgd(lr=0.5, momentum=0.5)
    pr.arena.check("denormal sgd")
    assert (pr.p[0] != 0).any() and (np.abs(pr.p[0]) < np.finfo(F32).tiny).all()


# ---- the norm ----
def _norm_call(hip, grads, max_norm, residues=None):
    _l, lib = _lib()
    arena = Arena(hip)
    idx = [arena.place(g, 0 if residues is None else residues[t]) for t, g in enumerate(grads)]
    out = arena.place([7.0, 7.0], 1)
    arena.upload()
    _l.check(lib.np_grad_norm(_vec([arena.ptr(i) for i in idx]), _sizes([np.asarray(g).size for g in grads]), len(grads), max_norm, arena.ptr(out)))
    assert _probe() == fam.norm_plan([np.asarray(g).size for g in grads]) + (0, 0)
    got = arena.dev.to_host()
    start = arena.items[out][0]
    result = got[start:start + 2].copy()
    arena.expect(out, result)
    arena.check("norm")                                         # nothing but the two floats was written
    return result


@pytest.mark.parametrize("seed,counts", fam.NORM_CASES, ids=lambda v: str(v) if isinstance(v, int) else "T%d" % len(v))
def test_grad_norm_of_gaussian_data_by_bits(hip, seed, counts):
    grads = fam.norm_data(seed, counts)
    for max_norm in (0.5, math.inf):
        want, wide = fam.grad_norm(grads, max_norm)
        assert fam.guard(wide)
        assert same(_norm_call(hip, grads, max_norm), want), (seed, max_norm)
    want = fam.grad_norm(grads, 0.5)[0]                         # the same at every alignment
    assert all(same(_norm_call(hip, grads, 0.5, residues=[(t + r) % 4 for t in range(len(counts))]), want) for r in (1, 2, 3))


def test_grad_norm_closed_forms_and_classes(hip):
    assert _norm_call(hip, [[3.0], [4.0]], 10.0).tolist() == [5.0, 1.0]                       # 3-4-5 across two tensors
    assert _norm_call(hip, [[3.0], [4.0]], 5.0).tolist() == [5.0, F32(5.0 / (5.0 + 1e-6))]
    assert _norm_call(hip, [[3.0], [4.0]], math.inf).tolist() == [5.0, 1.0]
    assert _norm_call(hip, [np.ones(1 << 14, F32)], 2.0).tolist() == [128.0, F32(2.0 / (128.0 + 1e-6))]      # all ones, two partials
    assert _norm_call(hip, [np.ones(9, F32), np.ones(7, F32)], 4.0).tolist() == [4.0, F32(4.0 / (4.0 + 1e-6))]
    assert _norm_call(hip, [np.zeros(5, F32)], 1.0).tolist() == [0.0, 1.0]
    n = fam.NORM_CHUNK + 5
    for where in (0, n // 2, n - 1):
        g = np.ones(n, F32)
        g[where] = np.nan
        assert np.isnan(_norm_call(hip, [np.ones(3, F32), g], 1.0)).all()
        g[where] = -np.inf
        assert same(_norm_call(hip, [g, np.ones(3, F32)], 1.0), np.array([np.inf, 0.0], F32))
        assert same(_norm_call(hip, [g], math.inf), np.array([np.inf, np.nan], F32))
    assert same(_norm_call(hip, [np.full(4, 3e38, F32)], 1.0), np.array([np.inf, 0.0], F32))  # finite in fp64, past fp32: +Inf by the one rounding


# ---- NDArray and optim.py ----
def _transposed_view(a):
    """the 2-dimensional GPU array `a` turned into the transposed view of its own buffer.  NDArray's own methods never hand out a
    view that is not contiguous (transpose and slice copy, $a[i] is a contiguous run), so the test does what a C host can: it swaps
    the extents and the byte strides in the array's header"""
    c = a._p.contents
    assert c.ndim == 2
    c.dimensions[0], c.dimensions[1] = c.dimensions[1], c.dimensions[0]
    c.strides[0], c.strides[1] = c.strides[1], c.strides[0]
    return a


def test_through_ndarray_with_views_and_pending_chains(hip):
    nd = _nd()
    rng = np.random.default_rng(60)
    gc.collect()
    live = nd.live_device_allocations()
    shapes = [(3, 5), (CHUNK + 1,), (1,), (2, 3, 4)]
    P = [fam.gaussian(rng, int(np.prod(s))).reshape(s) for s in shapes]
    Gr = [fam.gaussian(rng, int(np.prod(s))).reshape(s) for s in shapes]
    params, grads = [_gpu(p) for p in P], [_gpu(g) for g in Gr]
    bufs = [_gpu(np.zeros(s, F32)) for s in shapes]
    grads[0] = _transposed_view(_gpu(Gr[0].T.copy()))           # a view that is not contiguous, as a gradient
    assert grads[0].shape() == [3, 5]
    assert nd.dnn_sgd_step(params, grads, 0.05, momentum=0.9, buffers=bufs, first_step=True) is None
    norm = nd.dnn_grad_norm(grads, 0.5)
    assert same(norm.cpu().numpy(), fam.grad_norm(Gr, 0.5)[0])
    nd.dnn_sgd_step(params, grads, 0.05, momentum=0.9, buffers=bufs, grad_scale=(norm, 1))
    coef = norm.cpu().numpy()[1]
    for t in range(4):
        p, b = fam.sgd_step(P[t].reshape(-1), Gr[t].reshape(-1), None, lr=0.05, momentum=0.9, first_step=True)
        p, b = fam.sgd_step(p, Gr[t].reshape(-1), b, lr=0.05, momentum=0.9, scale=coef)
        assert same(params[t].cpu().numpy().reshape(-1), p) and same(bufs[t].cpu().numpy().reshape(-1), b), t
    from numpower_amd import ndarray as module
    was = module._LAZY_BINDING
    try:                                                        # pending chains: a gradient, and a parameter that is flushed first
        nd.set_lazy_binding(True)
        a, b = _gpu(P[1]), _gpu(Gr[1])
        g_chain = b * 2.0 + 1.0
        p_chain = a + 1.0
        m, v = _gpu(np.zeros(shapes[1], F32)), _gpu(np.zeros(shapes[1], F32))
        nd.dnn_adam_step([p_chain], [g_chain], [m], [v], 1, lr=0.01)
        gh = (Gr[1] * F32(2.0) + F32(1.0)).astype(F32)
        want = fam.adam_step((P[1] + F32(1.0)).astype(F32), gh, np.zeros_like(gh), np.zeros_like(gh), 1, lr=0.01)
        assert same(p_chain.cpu().numpy(), want[0]) and same(m.cpu().numpy(), want[1]) and same(v.cpu().numpy(), want[2])
        del a, b, g_chain, p_chain, m, v
    finally:
        nd.set_lazy_binding(was)
    del params, grads, bufs, norm
    gc.collect()
    assert nd.live_device_allocations() == live


def test_optim_py_matches_the_evaluator_over_five_steps(hip):
    from numpower_amd import optim
    nd = _nd()
    rng = np.random.default_rng(61)
    gc.collect()
    live = nd.live_device_allocations()
    shapes = [(7,), (CHUNK + 2,), (4, 4)]
    P = [fam.gaussian(rng, int(np.prod(s))) for s in shapes]
    steps = [[fam.gaussian(rng, p.size) for p in P] for _ in range(5)]
    for make, kind, hp in ((lambda ps: optim.SGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01), "sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01)),
                           (lambda ps: optim.SGD(ps, lr=0.05), "sgd", dict(lr=0.05)),
                           (lambda ps: optim.Adam(ps, lr=0.01, weight_decay=0.05), "adam", dict(lr=0.01, weight_decay=0.05)),
                           (lambda ps: optim.AdamW(ps, lr=0.01), "adam", dict(lr=0.01, weight_decay=1e-2, decoupled=True))):
        params = [_gpu(p.reshape(s)) for p, s in zip(P, shapes)]
        opt = make(params)
        hp_p = [p.copy() for p in P]
        st = [[np.zeros_like(p) for p in P] for _ in range(2)]
        for k, gs in enumerate(steps):
            max_norm = None if k == 1 else 1.0
            opt.step([_gpu(g.reshape(s)) for g, s in zip(gs, shapes)], max_norm=max_norm)
            scale = None
            if max_norm is not None:
                want_norm = fam.grad_norm(gs, max_norm)[0]
                assert same(opt.last_norm.cpu().numpy(), want_norm)
                scale = want_norm[1]
            for t in range(3):
                if kind == "sgd":
                    hp_p[t], b = fam.sgd_step(hp_p[t], gs[t], st[0][t], first_step=k == 0, scale=scale, **hp)
                    st[0][t] = b if b is not None else st[0][t]
                else:
                    hp_p[t], st[0][t], st[1][t] = fam.adam_step(hp_p[t], gs[t], st[0][t], st[1][t], k + 1, scale=scale, **hp)
                assert same(params[t].cpu().numpy().reshape(-1), hp_p[t]), (kind, k, t)
        assert opt.steps == 5
        del opt, params
    gc.collect()
    assert nd.live_device_allocations() == live


def test_every_refusal_and_message_on_the_device_and_no_allocation_is_left(hip):
    from numpower_amd.ndarray import Error
    from tests.test_optim_glue_cpu import MESSAGES
    nd = _nd()
    gc.collect()
    live = nd.live_device_allocations()
    ones = lambda *s: _gpu(np.ones(s, F32))
    M = lambda n: MESSAGES["NPH_OPTIM_MSG_" + n]

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    P, Gr, S1, S2 = ([ones(3), ones(2, 2)] for _ in range(4))
    cpu = [nd.array(np.ones(3, F32)), nd.array(np.ones((2, 2), F32))]
    sgd, adam, norm = nd.dnn_sgd_step, nd.dnn_adam_step, nd.dnn_grad_norm
    assert message(sgd, P, cpu, 0.1) == M("DEVICE") and message(adam, P, Gr, cpu, S2, 1) == M("DEVICE") and message(norm, [Gr[0], cpu[1]]) == M("DEVICE")
    assert message(sgd, P, Gr, 0.1, grad_scale=cpu[0]) == M("DEVICE") and message(sgd, cpu, cpu, 0.1) == M("CPU")
    assert message(sgd, P, Gr[:1], 0.1) == M("LENGTHS") and message(sgd, P, [ones(3), ones(5)], 0.1) == M("COUNT")
    assert message(sgd, P, Gr, 0.1, 0.9) == M("BUFFERS") and message(sgd, P, Gr, -1.0) == M("LR") and message(adam, P, Gr, S1, S2, 0) == M("STEP")
    assert message(adam, P, Gr, S1, S2, 1, betas=(1.0, 0.5)) == M("BETAS") and message(norm, Gr, -1.0) == M("MAX_NORM")
    assert message(sgd, P, Gr, 0.1, grad_scale=(ones(2), 2)) == M("SCALE")
    t = _transposed_view(ones(2, 3))                            # a view that is not contiguous cannot be updated in place
    assert message(sgd, [t], [ones(3, 2)], 0.1) == M("VIEW") and message(adam, [ones(3, 2)], [t], [t], [ones(3, 2)], 1) == M("VIEW")
    assert message(sgd, [ones(3, 2)], [ones(3, 2)], 0.1, 0.5, buffers=[t]) == M("VIEW")
    assert "overlaps" in message(sgd, [P[0], P[0]], [Gr[0], Gr[0]], 0.1) and "overlaps" in message(sgd, P, [P[0], Gr[1]], 0.1)
    assert "overlaps" in message(adam, P, Gr, S1, S1, 1) and "overlaps" in message(sgd, P, Gr, 0.1, grad_scale=P[1])
    before = [p.cpu().numpy().copy() for p in P]
    sgd(P, Gr, 0.0)                                             # lr = 0 is accepted
    shared = ones(3)
    sgd([ones(3), ones(3)], [shared, shared], 0.1)              # two gradients may share memory
    assert all(same(a, b.cpu().numpy()) for a, b in zip(before, P))
    del P, Gr, S1, S2, cpu, t, shared
    gc.collect()
    assert nd.live_device_allocations() == live


def test_a_captured_step_replayed_twice_equals_two_direct_steps(hip):
    _l, lib = _lib()
    counts = [CHUNK + 7, 3, 2 * CHUNK]
    direct, graph = Problem(hip, counts, 1, seed=70, scale=0.75), Problem(hip, counts, 1, seed=70, scale=0.75)
    for _ in range(2):
        direct.sgd(lr=0.05, momentum=0.9, weight_decay=0.01)
    direct.arena.check()
    p, g, s, n = graph.lists()
    handle = C.c_void_p()
    _l.check(lib.np_graph_begin())
    rc = lib.np_sgd_step(p, g, s[0], n, graph.T, 0.05, 0.9, 0.0, 0.01, 0, 0, graph.scale_ptr())
    _l.check(lib.np_graph_end(C.byref(handle)))
    _l.check(rc)
    try:
        _l.check(lib.np_graph_launch(handle))
        _l.check(lib.np_graph_launch(handle))
        hip.sync()
    finally:
        _l.check(lib.np_graph_destroy(handle))
    assert same(graph.arena.dev.to_host(), direct.arena.dev.to_host())


def test_the_example_trains(hip):
    from examples import attention_adam_classifier as ex
    X, labels = ex.make_problem(64)
    params, losses, opt = ex.train_gpu(X, labels, epochs=6)
    per = 64 // ex.BATCH
    assert opt.steps == 6 * per and opt.last_norm.shape() == [2]
    assert np.mean(losses[-per:]) < 0.7 * np.mean(losses[:per]), losses
