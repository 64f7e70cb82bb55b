"""GPU tests of scaled dot-product attention (np_attention.hip: np_attention_forward, np_attention_backward;
NDArray.dnn_attention_forward / _backward) against tests/attention_family.py, which tests/test_attention_reference_cpu.py holds to
torch.

The exact family is compared bit for bit: o, both statistics, dq, dk, dv.  Gaussian data is compared with the float64 evaluator
inside the bounds derived in attention_family.  Operands sit at float offsets 0 .. 3 inside NaN frames and outputs inside a canary
(gemm_family.framed / canary), the whole allocation compared; every call asserts the whole probe record against the dispatcher
restated in attention_family.py, with the tile extents read from np_debug_attention_bounds."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import attention_family as A
from tests.test_gpu_batchnorm import _Call, same

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES_F, NAMES_B = ("o", "save_max", "save_sum"), ("dq", "dk", "dv")


def _nd():
    from numpower_amd.ndarray import NDArray
    return NDArray


def _lib():
    from numpower_amd import _lib
    return _lib, _lib.load()


def _gpu(a):
    return _nd().array(np.asarray(a, np.float32)).gpu()


def _host(a, shape):
    return a.cpu().numpy().reshape(shape)


def _bounds():
    _l, lib = _lib()
    b = (C.c_size_t * 7)()
    _l.check(lib.np_debug_attention_bounds(b, 7))
    return tuple(b)


def _probe():
    _l, lib = _lib()
    d, tq, tk, n, kt, sk = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
    _l.check(lib.np_debug_attention_last_path(*[C.byref(x) for x in (d, tq, tk, n, kt, sk)]))
    return d.value, tq.value, tk.value, n.value, kt.value, sk.value


def _fwd(hip, q, k, v, causal, scale, off=0, stats=(True, True)):
    """np_attention_forward -> dict; the probe must report what the dispatcher says"""
    _l, lib = _lib()
    (BH, Sq, D), Sk = q.shape, k.shape[1]
    c = _Call(hip, off)
    try:
        pq, pk, pv = c.operand(q), c.operand(k), c.operand(v)
        po, oo = c.output(q.shape)
        pm, om = c.output((BH, Sq)) if stats[0] else (None, None)
        ps, os_ = c.output((BH, Sq)) if stats[1] else (None, None)
        _l.check(lib.np_attention_forward(pq, pk, pv, BH, Sq, Sk, D, int(causal), scale, po, pm, ps))
        assert _probe() == A.probe(Sq, Sk, D, causal, bounds=_bounds()), (_probe(), q.shape, Sk, causal)
        return {"o": c.take(oo), "save_max": c.take(om) if stats[0] else None, "save_sum": c.take(os_) if stats[1] else None}
    finally:
        c.free()


def _bwd(hip, q, k, v, o, dout, m, l, causal, scale, off=0, grads=(True, True, True)):
    _l, lib = _lib()
    (BH, Sq, D), Sk = q.shape, k.shape[1]
    c = _Call(hip, off)
    try:
        ins = [c.operand(a) for a in (q, k, v, o, dout, m, l)]
        outs = [c.output(s) if g else (None, None) for s, g in zip((q.shape, k.shape, v.shape), grads)]
        _l.check(lib.np_attention_backward(*ins, BH, Sq, Sk, D, int(causal), scale, *[p for p, _ in outs]))
        assert _probe() == A.probe(Sq, Sk, D, causal, True, grads, _bounds()), (_probe(), q.shape, Sk, causal, grads)
        return {n: c.take(h) if g else None for n, (_, h), g in zip(NAMES_B, outs, grads)}
    finally:
        c.free()


def _both(hip, d, causal, scale, off=0):
    f = _fwd(hip, d["q"], d["k"], d["v"], causal, scale, off)
    b = _bwd(hip, d["q"], d["k"], d["v"], f["o"], d["dout"], f["save_max"], f["save_sum"], causal, scale, off + 1)
    return {**f, **b}


def _through_ndarray(d, causal, scale, lead=None):
    nd = _nd()
    BH, Sq, D = d["q"].shape
    lead = (BH,) if lead is None else lead
    shape = lambda a: lead + a.shape[1:]
    q, k, v, dout = (_gpu(d[n].reshape(shape(d[n]))) for n in ("q", "k", "v", "dout"))
    o, m, l = nd.dnn_attention_forward(q, k, v, causal, scale)
    assert o.shape() == list(shape(d["q"])) and m.shape() == list(lead) + [Sq] and l.shape() == list(lead) + [Sq]
    dq, dk, dv = nd.dnn_attention_backward(q, k, v, o, dout, m, l, causal, scale)
    assert dq.shape() == list(shape(d["q"])) and dk.shape() == list(shape(d["k"])) and dv.shape() == list(shape(d["v"]))
    return {"o": _host(o, d["q"].shape), "save_max": _host(m, (BH, Sq)), "save_sum": _host(l, (BH, Sq)), "dq": _host(dq, d["q"].shape),
            "dk": _host(dk, d["k"].shape), "dv": _host(dv, d["v"].shape)}


def test_the_family_uses_the_constants_the_library_reports():
    assert _bounds() == A.BOUNDS


# ---- 1. the exact family, by bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.EXACT_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]) + ("c" if c[4] else "") + c[6][0])
def test_exact_family_by_bits(hip, case):
    BH, Sq, Sk, D, causal, sizes, layout, scale = case
    d = A.exact_family(BH, Sq, Sk, D, causal, sizes, scale, layout)
    off = (Sq + Sk + D) % 4
    f = _fwd(hip, d["q"], d["k"], d["v"], causal, d["scale"], off)
    for n in NAMES_F:
        assert same(f[n], d[n]), (n, np.abs(f[n] - d[n]).max())
    assert same(_fwd(hip, d["q"], d["k"], d["v"], causal, d["scale"], off + 1, stats=(False, False))["o"], d["o"])      # NULL statistics
    assert same(_fwd(hip, d["q"], d["k"], d["v"], causal, d["scale"], off + 2, stats=(True, False))["save_max"], d["save_max"])
    if d["backward_ok"]:
        b = _bwd(hip, d["q"], d["k"], d["v"], d["o"], d["dout"], d["save_max"], d["save_sum"], causal, d["scale"], off + 1)
        for n in NAMES_B:
            assert same(b[n], d[n]), (n, np.abs(b[n] - d[n]).max())
        if Sq % 2:      # through NDArray too, the default scale where the family took it
            nd = _through_ndarray(d, causal, scale)
            assert all(same(nd[n], d[n]) for n in NAMES_F + NAMES_B)


def test_each_null_subset_of_the_gradients(hip):
    d = A.exact_family(3, 65, 129, 64, False, (1, 2, 4, 8, 16))
    args = (d["q"], d["k"], d["v"], d["o"], d["dout"], d["save_max"], d["save_sum"], False, d["scale"])
    for bits in range(8):
        grads = tuple(bool(bits >> i & 1) for i in range(3))
        b = _bwd(hip, *args, off=bits, grads=grads)      # the probe's launch count is asserted inside: 0 launches with all three absent
        for n, g in zip(NAMES_B, grads):
            assert (same(b[n], d[n]) if g else b[n] is None), (n, grads)


# ---- 2. Gaussian data inside the derived bounds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.GAUSSIAN_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]) + ("c" if c[4] else "") + "s%d" % c[5])
def test_gaussian_inside_the_bounds(hip, case):
    BH, Sq, Sk, D, causal, sigma = case
    d = A.gaussian(BH, Sq, Sk, D, sigma)
    scale = A.default_scale(D)
    ref = A.reference64(d["q"], d["k"], d["v"], d["dout"], causal, scale)
    bound = A.bounds(d["q"], d["k"], d["v"], d["dout"], causal, scale, ref)
    got = _both(hip, d, causal, scale, off=Sq % 4)
    worst = {n: A.worst_fraction(got[n], ref[n], bound[n]) for n in NAMES_F + NAMES_B}
    print("worst fraction of the bound", case, {n: "%.4f" % w for n, w in worst.items()})
    assert all(w <= 1.0 for w in worst.values()), worst
    if Sq in (33, 128):
        nd = _through_ndarray(d, causal, None)
        assert all(same(nd[n], got[n]) for n in NAMES_F + NAMES_B)


# ---- 3. determinism and independence, by bits ------------------------------------------------------------------------------------------------------
def test_three_runs_and_a_slice_alone_equal_the_slice_in_a_batch_of_five(hip):
    for causal in (False, True):
        d = A.gaussian(5, 129, 161, 64, 6.0, seed=3)
        scale = A.default_scale(64)
        runs = [_both(hip, d, causal, scale, off=r) for r in range(3)]
        for r in runs[1:]:
            assert all(same(r[n], runs[0][n]) for n in NAMES_F + NAMES_B)
        for b in (0, 3, 4):
            one = _both(hip, {n: d[n][b:b + 1] for n in ("q", "k", "v", "dout")}, causal, scale, off=b)
            assert all(same(one[n][0], runs[0][n][b]) for n in NAMES_F + NAMES_B), (b, causal)


def test_the_row_prefix_identities(hip):
    """Without causal the first n rows of a call equal the call on q[:, :n].  With causal, on finite operands, row i equals row i of
    the call on q[:, :n], k[:, :c], v[:, :c] for every n > i and every c with min(c, i + 1) = min(Sk, i + 1) (np_hip.h)."""
    TK = _bounds()[1]
    d = A.gaussian(2, 161, 145, 32, 1.0, seed=5)
    scale = A.default_scale(32)
    full = _fwd(hip, d["q"], d["k"], d["v"], False, scale)
    for n in (1, 31, 33, 128, 129):
        part = _fwd(hip, d["q"][:, :n], d["k"], d["v"], False, scale, off=n)
        assert all(same(part[x], full[x][:, :n]) for x in NAMES_F), n
    full = _fwd(hip, d["q"], d["k"], d["v"], True, scale)
    for i in (0, 30, 32, 63, 127, 128, 144, 160):
        cuts = {(i + 1, min(145, i + 1)), (i + 1, min(145, -(-(i + 1) // TK) * TK)), (min(161, i + 40), 145)}      # both cut to i + 1, rounded up to the key tile, Sq alone
        for n, c in sorted(cuts):
            assert min(c, i + 1) == min(145, i + 1)
            part = _fwd(hip, d["q"][:, :n], d["k"][:, :c], d["v"][:, :c], True, scale, off=i)
            assert all(same(part[x][:, i], full[x][:, i]) for x in NAMES_F), (i, n, c)


def test_causal_equals_the_unmasked_call_where_every_masked_score_is_the_low_one(hip):
    """The diagonal layout with one member per class: every key above the diagonal is a filler or a member of another class, so its
    score is the family's m - 200 whether or not it is masked, and fast_exp gives +0.0f either way."""
    for Sq, D in ((129, 64), (65, 16)):
        d = A.exact_family(2, Sq, Sq, D, True, (1,), None, "diagonal")
        a, b = _both(hip, d, True, d["scale"]), _both(hip, d, False, d["scale"], off=2)
        assert all(same(a[n], b[n]) and same(a[n], d[n]) for n in NAMES_F + NAMES_B)


# ---- 4. special values -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", (False, True))
def test_the_footprint_of_a_nan_or_an_inf(hip, causal):
    BH, Sq, Sk, D = 3, 97, 97, 33
    base = A.gaussian(BH, Sq, Sk, D, 1.0, seed=9)
    scale, b, TK = A.default_scale(D), 1, _bounds()[1]
    for row in (0, 40, Sq - 1):
        for col, bad in ((0, np.nan), (D // 2, np.inf), (D - 1, -np.inf)):
            d = {n: a.copy() for n, a in base.items()}
            d["q"][b, row, col] = bad
            g = _both(hip, d, causal, scale)
            hit = np.zeros((BH, Sq), bool)
            hit[b, row] = True
            for n in ("o", "dq"):
                assert np.isnan(g[n][hit]).all() and np.isfinite(g[n][~hit]).all(), (n, row, col)
            assert np.isnan(g["save_sum"][hit]).all() and np.isfinite(g["save_sum"][~hit]).all()
    for name in ("k", "v"):
        for j in (0, 40, Sk - 1):
            for col in (0, D // 2, D - 1):
                d = {n: a.copy() for n, a in base.items()}
                d[name][b, j, col] = np.nan
                g = _fwd(hip, d["q"], d["k"], d["v"], causal, scale, off=col)
                sees = np.arange(Sq) >= j if causal else np.ones(Sq, bool)
                # under causal the rows above j in the key tile of j are not specified: 0 . NaN on the matrix core is NaN
                free = (np.arange(Sq) < j) & (np.arange(Sq) // TK == j // TK) if causal else np.zeros(Sq, bool)
                rows_nan = np.isnan(g["o"][b]).any(-1)
                assert rows_nan[sees].all() and not rows_nan[~sees & ~free].any(), (name, j, col)
                if name == "k":
                    assert np.isnan(g["o"][b][sees]).all()
                others = [x for x in range(BH) if x != b]
                assert np.isfinite(g["o"][others]).all() and np.isfinite(g["save_sum"][others]).all()      # no other slice is reached


def test_a_row_whose_visible_scores_are_all_minus_inf_is_nan(hip):
    d = A.gaussian(1, 40, 50, 8, 1.0, seed=2)
    d["q"][0, 7] = 1.0
    d["k"][0, :, :] = np.abs(d["k"][0])
    d["q"][0, 7, 3] = -np.inf      # every score of row 7 is -Inf
    g = _fwd(hip, d["q"], d["k"], d["v"], False, 1.0)
    assert np.isnan(g["o"][0, 7]).all() and g["save_max"][0, 7] == -np.inf and np.isnan(g["save_sum"][0, 7]) and np.isfinite(np.delete(g["o"][0], 7, 0)).all()


def test_saturated_scores_stay_finite(hip):
    """Scores of +-80 000: exp of the raw score overflows, the fused evaluation subtracts the running maximum first.  The exact
    family scaled up: q = 80 000 . onehot, so every score is 80 000 or 0 and the closed form still holds by bits."""
    d = A.exact_family(2, 65, 129, 16, False, (1, 2, 4, 8), 1.0)
    q = (d["q"] * F32(400.0)).astype(F32)
    q[:, ::2] *= -1                                       # every other row sees -80 000 at its class and 0 elsewhere: the uniform row
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(F32(80000.0)))
    f = _fwd(hip, q, d["k"], d["v"], False, 1.0)
    assert np.isfinite(f["o"]).all() and same(f["o"][:, 1::2], d["o"][:, 1::2])
    assert (f["save_max"][:, 1::2] == 80000.0).all() and (f["save_max"][:, ::2] == 0.0).all()
    ref = A.reference64(q, d["k"], d["v"], d["dout"], False, 1.0)
    assert np.abs(f["o"] - ref["o"]).max() <= 1e-6
    b = _bwd(hip, q, d["k"], d["v"], f["o"], d["dout"], f["save_max"], f["save_sum"], False, 1.0)
    assert all(np.isfinite(b[n]).all() for n in NAMES_B)


# ---- 5. the composition from existing calls ------------------------------------------------------------------------------------------------------
def test_the_composition_lies_inside_the_bound(hip):
    nd = _nd()
    BH, Sq, Sk, D = 3, 65, 129, 64
    d = A.gaussian(BH, Sq, Sk, D, 1.0, seed=4)
    scale = A.default_scale(D)
    q, k, v = (_gpu(d[n]) for n in ("q", "k", "v"))
    s = nd.batched_matmul(q, nd.transpose(k, (0, 2, 1))) * scale
    o = _host(nd.batched_matmul(nd.softmax(s, -1), v), (BH, Sq, D))
    ref = A.reference64(d["q"], d["k"], d["v"], d["dout"], False, scale)
    bound = A.bounds(d["q"], d["k"], d["v"], d["dout"], False, scale, ref)
    fused = _host(nd.dnn_attention_forward(q, k, v)[0], (BH, Sq, D))
    print("worst fraction: composition %.4f, fused %.4f" % (A.worst_fraction(o, ref["o"], bound["o"]), A.worst_fraction(fused, ref["o"], bound["o"])))
    assert A.worst_fraction(o, ref["o"], bound["o"]) <= 1.0 and A.worst_fraction(fused, ref["o"], bound["o"]) <= 1.0


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------------------------------
def _pool_block(nbytes):
    """np_malloc's size classes: powers of two below 1 MiB, 2 MiB granules above, and up to 3 KiB of stagger on a large block"""
    if nbytes < 1 << 20:
        s = 256
        while s < nbytes:
            s <<= 1
        return s
    g = 2 << 20
    return -(-nbytes // g) * g + 4096


def test_the_score_matrix_is_never_allocated(hip):
    """BH = 1, Sq = Sk = 8192, D = 64: the scores would be 256 MiB.  Forward plus backward may reserve the eight (S, D) arrays, the two
    statistics and BH.Sq floats of scratch for delta, each rounded to the pool's size class, and nothing else."""
    _l, lib = _lib()
    nd = _nd()
    S, D = 8192, 64
    rng = np.random.default_rng(0)
    host = [rng.standard_normal((1, S, D)).astype(F32) for _ in range(4)]
    gc.collect()
    freed = C.c_size_t()
    _l.check(lib.np_pool_trim(C.byref(freed)))
    before = lib.np_pool_reserved_bytes()
    q, k, v, dout = (_gpu(a) for a in host)
    o, m, l = nd.dnn_attention_forward(q, k, v, True)
    dq, dk, dv = nd.dnn_attention_backward(q, k, v, o, dout, m, l, True)
    hip.sync()
    growth = lib.np_pool_reserved_bytes() - before
    cap = 8 * _pool_block(4 * S * D) + 2 * _pool_block(4 * S) + _pool_block(4 * S)
    assert growth <= cap < 4 * S * S // 8, (growth, cap)
    ref = A.reference64(host[0][:, -1:], host[1], host[2], host[3][:, -1:], False, A.default_scale(D))      # the last row sees every key
    assert np.abs(_host(o, (1, S, D))[:, -1:] - ref["o"]).max() <= 1e-4


# ---- 7. the upper layers -------------------------------------------------------------------------------------------------------------------------------
def test_views_pending_chains_and_leading_axes_as_operands(hip):
    nd = _nd()
    d = A.gaussian(6, 40, 50, 16, 1.0, seed=8)
    scale = A.default_scale(16)
    want = _both(hip, d, True, scale)
    got = _through_ndarray(d, True, None, lead=(2, 3))                      # leading axes (2, 3) are flattened to BH = 6
    assert all(same(got[n], want[n]) for n in NAMES_F + NAMES_B)
    kt = _gpu(np.ascontiguousarray(d["k"].transpose(0, 2, 1)))             # a transposed view as k
    qh = _gpu(d["q"] * F32(0.5))
    o, m, l = nd.dnn_attention_forward(qh + qh, nd.transpose(kt, (0, 2, 1)), _gpu(d["v"]), True)      # a pending chain as q: 0.5 q + 0.5 q = q
    assert same(_host(o, d["q"].shape), want["o"]) and same(_host(m, (6, 40)), want["save_max"])
    dq, dk, dv = nd.dnn_attention_backward(qh + qh, nd.transpose(kt, (0, 2, 1)), _gpu(d["v"]), o, _gpu(d["dout"]), m, l, True)
    assert same(_host(dq, d["q"].shape), want["dq"]) and same(_host(dk, d["k"].shape), want["dk"]) and same(_host(dv, d["v"].shape), want["dv"])
    o2 = nd.dnn_attention_forward(_gpu(d["q"][0]), _gpu(d["k"][0]), _gpu(d["v"][0]), True, scale)[0]      # ndim 2: BH = 1
    assert o2.shape() == [40, 16] and same(_host(o2, (40, 16)), want["o"][0])


def test_every_message_on_device_operands_and_no_leak(hip):
    from numpower_amd.ndarray import Error
    from tests.test_attention_glue_cpu import MESSAGES
    nd = _nd()
    ones = lambda *s: _gpu(np.ones(s, F32))
    gc.collect()
    live = nd.live_device_allocations()
    q, k, v = ones(2, 5, 8), ones(2, 7, 8), ones(2, 7, 8)

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    f, b, M = nd.dnn_attention_forward, nd.dnn_attention_backward, (lambda n: MESSAGES["NPH_ATTN_MSG_" + n])
    assert message(f, ones(8), ones(8), ones(8)) == M("NDIM") and message(f, q, ones(7, 8), v) == M("NDIM")
    assert message(f, q, ones(3, 7, 8), v) == M("LEADING") and message(f, q, k, ones(1, 7, 8)) == M("LEADING")
    assert message(f, q, ones(2, 7, 9), v) == M("D") and message(f, q, k, ones(2, 7, 4)) == M("D")
    assert message(f, q, k, ones(2, 6, 8)) == M("SK")
    assert message(f, ones(2, 5, 129), ones(2, 7, 129), ones(2, 7, 129)) == M("DMAX")
    o, m, l = f(q, k, v)
    assert message(b, q, k, v, ones(2, 5, 7), q, m, l) == M("OUTPUT") and message(b, q, k, v, o, ones(2, 4, 8), m, l) == M("OUTPUT")
    assert message(b, q, k, v, o, q, ones(2, 4), l) == M("SAVED") and message(b, q, k, v, o, q, m, ones(10)) == M("SAVED")
    assert message(f, q, k, v, scale=float("inf")) == M("SCALE")
    cpu = nd.array(np.ones((2, 7, 8), F32))
    assert message(f, q, cpu, v) == M("DEVICE") and message(b, q, k, v, o, q, m, nd.array(np.ones((2, 5), F32))) == M("DEVICE")
    assert message(f, cpu, cpu, cpu) == M("CPU")
    del q, k, v, o, m, l, cpu
    gc.collect()
    assert nd.live_device_allocations() == live


def test_live_device_allocations_are_unchanged(hip):
    nd = _nd()
    gc.collect()
    live = nd.live_device_allocations()
    d = A.gaussian(2, 70, 90, 40, 1.0)
    _through_ndarray(d, True, None)
    _through_ndarray(d, False, 0.25)
    gc.collect()
    assert nd.live_device_allocations() == live


def test_the_example_trains(hip):
    from examples import attention_classifier as ex
    X, labels = ex.make_problem(64)
    params, losses = ex.train_gpu(X, labels, epochs=6, lr=ex.LR)
    per = 64 // ex.BATCH
    assert np.mean(losses[-per:]) < 0.7 * np.mean(losses[:per]), losses
    assert np.isfinite(ex.predict(X, params)).all()
