"""tests/softmax_family.py against torch's CPU softmax, log_softmax and cross_entropy: the fp64 evaluator is torch's float64 result to
a few fp64 ulp (and class by class on the special values); the exact family's expectations are float32(torch's float64 result)
bit for bit; and plain fp32 implementations of the header's formulas (numpy in three summation orders, torch fp32) sit inside
every derived bound, neither far below it nor above."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import softmax_family as S

EPS64 = 2.0 ** -52


def _close64(got, want, cols):
    """a few fp64 ulp: the two sums of `cols` terms may be ordered differently, hence cols . eps of the magnitude"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    scale = np.maximum(np.abs(want[fin]), 1.0)
    assert np.all(np.abs(got[fin] - want[fin]) <= (cols + 8) * EPS64 * scale * 300)      # |d| <= 300 scales exp's argument error


def _torch_all(x, dy, labels, prob, scale):
    """torch float64: softmax, log-softmax, both backwards by autograd, both cross-entropies with their gradients"""
    out = {}
    t = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    g = torch.tensor(np.asarray(dy, np.float64))
    for name, fn in (("softmax", torch.softmax), ("log_softmax", torch.log_softmax)):
        y = fn(t, 1)
        out[name] = y.detach().numpy()
        out[name + "_bwd"] = torch.autograd.grad(y, t, g)[0].numpy()
    if labels is not None:
        l2 = torch.tensor(np.asarray(x, np.float64)[:, :, 0], requires_grad=True)
        loss = F.cross_entropy(l2, torch.tensor(labels, dtype=torch.long), reduction="none")
        out["xent_index"] = loss.detach().numpy()
        out["xent_index_grad"] = torch.autograd.grad(loss.sum() * scale, l2)[0].numpy()
        l3 = torch.tensor(np.asarray(x, np.float64)[:, :, 0], requires_grad=True)
        loss = F.cross_entropy(l3, torch.tensor(np.asarray(prob, np.float64)), reduction="none")
        out["xent_prob"] = loss.detach().numpy()
        out["xent_prob_grad"] = torch.autograd.grad(loss.sum() * scale, l3)[0].numpy()
    return out


@pytest.mark.parametrize("sigma", [1.0, 30.0])
@pytest.mark.parametrize("shape", [(7, 10, 1), (3, 257, 1), (2, 21, 5)])
def test_the_evaluator_is_torch_in_float64(shape, sigma):
    rng = np.random.default_rng(11)
    x, dy = S.gaussian(rng, shape, sigma), S.gaussian(rng, shape, 1.0)
    rows, cols = shape[0], shape[1]
    labels = rng.integers(0, cols, rows) if shape[2] == 1 else None
    prob = rng.random((rows, cols)).astype(np.float32)
    prob = (prob / prob.sum(axis=1, keepdims=True)).astype(np.float32)
    want = _torch_all(x, dy, labels, prob, 0.25)
    _close64(S.forward(x, S.SOFTMAX), want["softmax"], cols)
    _close64(S.forward(x, S.LOG_SOFTMAX), want["log_softmax"], cols)
    _close64(S.backward(want["softmax"], dy, S.SOFTMAX), want["softmax_bwd"], cols)
    _close64(S.backward(want["log_softmax"], dy, S.LOG_SOFTMAX), want["log_softmax_bwd"], cols)
    if labels is not None:
        loss, grad = S.cross_entropy(x[:, :, 0], labels.astype(np.float32), S.XENT_INDEX, 0.25)
        _close64(loss, want["xent_index"], cols)
        _close64(grad, want["xent_index_grad"], cols)
        loss, grad = S.cross_entropy(x[:, :, 0], prob, S.XENT_PROB, 0.25)
        _close64(loss, want["xent_prob"], cols)
        # the rule assumes sum(t) == 1 and writes p - t; torch writes p . sum(t) - t, and an fp32 row sums to 1 only nearly
        excess = prob.astype(np.float64).sum(axis=1, keepdims=True) - 1.0
        _close64(grad + want["softmax"][:, :, 0] * excess * 0.25, want["xent_prob_grad"], cols)


def test_the_class_map_is_torchs_on_the_special_values():
    x = S.special_matrix(7)
    for mode, fn in ((S.SOFTMAX, torch.softmax), (S.LOG_SOFTMAX, torch.log_softmax)):
        for dtype in (torch.float32, torch.float64):
            got = fn(torch.tensor(x).to(dtype), 1).numpy()
            ours = S.forward(x[:, :, None], mode)[:, :, 0]
            for r, name in enumerate(S.SPECIAL_ROWS):
                assert S.classes_hold(got[r], x[r], mode), (name, got[r])
                assert S.classes_hold(ours[r], x[r], mode), (name, ours[r])
    assert [S.row_class(r) for r in S.SPECIAL_ROWS.values()] == ["nan", "nan", "nan", "ok", "nan", "nan", "ok"]
    # invalid labels: the evaluator's row is NaN, in the loss and in every element of the gradient, and no other row's is
    logits = S.gaussian(np.random.default_rng(3), (len(S.INVALID_LABELS) + 2, 6), 1.0)
    labels = np.array([2.0] + S.INVALID_LABELS + [6.0], np.float32)
    assert list(S.valid_labels(labels, 6)) == [True] + [False] * (len(labels) - 1)
    loss, grad = S.cross_entropy(logits, labels, S.XENT_INDEX)
    assert np.isfinite(loss[0]) and np.isfinite(grad[0]).all() and np.isnan(loss[1:]).all() and np.isnan(grad[1:]).all()


@pytest.mark.parametrize("filler", ["-inf", "m-200"])
def test_the_exact_family_is_float32_of_torchs_float64(filler):
    rng = np.random.default_rng(5)
    x, ks, at = S.exact_rows(rng, 5 * len(S.EXACT_K), 33, filler)
    assert set(ks) == set(S.EXACT_K)
    y64 = torch.softmax(torch.tensor(x.astype(np.float64)), 1).numpy()
    want = S.exact_softmax(ks, at)
    assert S.same(want, y64.astype(np.float32))            # the k chosen: float32(1 / k in fp64) == float32(1) / float32(k)
    assert S.same(want, S.forward(x[:, :, None], S.SOFTMAX)[:, :, 0].astype(np.float32))
    one = ks == 1
    ly64 = torch.log_softmax(torch.tensor(x[one].astype(np.float64)), 1).numpy()
    lwant = S.exact_log_softmax(x[one], ks[one], at[one])
    assert S.same(lwant, ly64.astype(np.float32)) and not np.signbit(lwant[at[one]]).any()
    # backward: exact in any order, so fp32 arithmetic in any order gives the expectation's bits
    pow2 = np.isin(ks, (1, 2, 4, 8, 16))
    dy, dx = S.exact_backward_softmax(rng, want[pow2])
    t = torch.tensor(x[pow2].astype(np.float64), requires_grad=True)
    auto = torch.autograd.grad(torch.softmax(t, 1), t, torch.tensor(dy.astype(np.float64)))[0].numpy()
    assert np.array_equal(dx, auto.astype(np.float32))
    t32 = (dy * want[pow2]).sum(axis=1, keepdims=True, dtype=np.float32)
    assert np.array_equal(dx, want[pow2] * (dy - t32))
    dy, dx = S.exact_backward_log_softmax(rng, lwant)
    assert np.array_equal(dx, S.backward(lwant, dy, S.LOG_SOFTMAX).astype(np.float32))
    # cross-entropy: labels at a maximum and (m - 200 fillers) at a filler; power-of-two k and scale for the gradient
    labels = np.where(np.arange(len(ks)) % 2 == 0, at.argmax(axis=1), (~at).argmax(axis=1))
    for scale in (1.0, 0.125):
        loss, grad = S.exact_cross_entropy(x, ks, at, labels, scale)
        l64 = torch.tensor(x.astype(np.float64), requires_grad=True)
        tl = F.cross_entropy(l64, torch.tensor(labels), reduction="none")
        tg = torch.autograd.grad(tl.sum() * scale, l64)[0].numpy()
        # torch negates log_softmax and so returns -0.0 where the rule's logf(s) - d_label is +0.0: the zero's sign is put aside
        assert S.same(loss[one], tl.detach().numpy().astype(np.float32)[one] + np.float32(0.0))
        assert S.same(grad[pow2], tg.astype(np.float32)[pow2])
        assert set(np.unique(loss[one])) <= {0.0, 200.0, np.inf}


def _sum_orders(terms):
    """fp32 sums of the last axis in three orders: forward, reverse, pairwise"""
    fwd = np.zeros(terms.shape[:-1], np.float32)
    rev = np.zeros(terms.shape[:-1], np.float32)
    for j in range(terms.shape[-1]):
        fwd = (fwd + terms[..., j]).astype(np.float32)
        rev = (rev + terms[..., terms.shape[-1] - 1 - j]).astype(np.float32)
    pair = terms.astype(np.float32)
    while pair.shape[-1] > 1:
        if pair.shape[-1] % 2:
            pair = np.concatenate([pair, np.zeros(pair.shape[:-1] + (1,), np.float32)], axis=-1)
        pair = (pair[..., 0::2] + pair[..., 1::2]).astype(np.float32)
    return fwd, rev, pair[..., 0]


@pytest.mark.parametrize("sigma", [1.0, 30.0])
@pytest.mark.parametrize("rows,cols", [(64, 10), (16, 257), (4, 4099)])
def test_fp32_implementations_sit_inside_every_bound(rows, cols, sigma, capsys):
    rng = np.random.default_rng(cols)
    f32 = np.float32
    x = S.gaussian(rng, (rows, cols), sigma)
    dy = S.gaussian(rng, (rows, cols), 1.0)
    labels = rng.integers(0, cols, rows)
    prob = rng.random((rows, cols)).astype(f32)
    prob = (prob / prob.sum(axis=1, keepdims=True)).astype(f32)
    x3 = x[:, :, None]
    want = {m: S.forward(x3, m)[:, :, 0] for m in (S.SOFTMAX, S.LOG_SOFTMAX)}
    bnd = {m: S.bound_forward(x3, m)[:, :, 0] for m in (S.SOFTMAX, S.LOG_SOFTMAX)}
    worst = {}

    def note(name, got, ref, bound):
        worst[name] = max(worst.get(name, 0.0), S.worst(got, ref, bound))

    d = (x - x.max(axis=1, keepdims=True)).astype(f32)
    e = np.exp(d.astype(np.float64)).astype(f32)           # a correctly rounded exp: inside fast_exp's 1.2 ulp
    for s in _sum_orders(e):
        s = s[:, None]
        y, ly = (e / s).astype(f32), (d - np.log(s.astype(np.float64)).astype(f32)).astype(f32)
        note("softmax", y, want[S.SOFTMAX], bnd[S.SOFTMAX])
        note("log_softmax", ly, want[S.LOG_SOFTMAX], bnd[S.LOG_SOFTMAX])
        lw, gw = S.cross_entropy(x, labels.astype(f32), S.XENT_INDEX, 0.5)
        lb, gb = S.bound_cross_entropy(x, labels.astype(f32), S.XENT_INDEX, 0.5)
        note("loss_index", -ly[np.arange(rows), labels], lw, lb)
        onehot = np.zeros((rows, cols), f32)
        onehot[np.arange(rows), labels] = 1
        note("grad_index", ((y - onehot) * f32(0.5)).astype(f32), gw, gb)
        lw, gw = S.cross_entropy(x, prob, S.XENT_PROB, 0.5)
        lb, gb = S.bound_cross_entropy(x, prob, S.XENT_PROB, 0.5)
        for lp in _sum_orders((prob * (-ly)).astype(f32)):
            note("loss_prob", lp, lw, lb)
        note("grad_prob", ((y - prob) * f32(0.5)).astype(f32), gw, gb)
        # the backward passes take fp32 outputs as exact inputs
        for t in _sum_orders((dy * y).astype(f32)):
            note("softmax_bwd", (y * (dy - t[:, None])).astype(f32), S.backward(y, dy, S.SOFTMAX), S.bound_backward(y, dy, S.SOFTMAX))
        ey = np.exp(ly.astype(np.float64)).astype(f32)
        for t in _sum_orders(dy):
            note("log_softmax_bwd", (dy - (ey * t[:, None]).astype(f32)).astype(f32), S.backward(ly, dy, S.LOG_SOFTMAX),
                 S.bound_backward(ly, dy, S.LOG_SOFTMAX))
    tx = torch.tensor(x)
    note("softmax", torch.softmax(tx, 1).numpy(), want[S.SOFTMAX], bnd[S.SOFTMAX])
    note("log_softmax", torch.log_softmax(tx, 1).numpy(), want[S.LOG_SOFTMAX], bnd[S.LOG_SOFTMAX])
    with capsys.disabled():
        print("\n[softmax bounds] %d x %d sigma %g: worst fraction of the bound " % (rows, cols, sigma)
              + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    for name, w in worst.items():
        assert w <= 1.0, (name, w)                 # not unmeetable
    assert max(worst.values()) >= 2.0 ** -12      # and not vacuous: some plain fp32 result uses a visible share of its bound


def test_the_constant_of_the_softmax_bound():
    assert S.softmax_c(10) == pytest.approx(4.8) and S.softmax_c(4099, S.FORM_BLOCK) == pytest.approx(4.8)
    assert S.softmax_c(1 << 20, S.FORM_STREAM) == pytest.approx(4.8)          # the running forms stay inside cols - 1 for long rows
    assert S.softmax_c(21, S.FORM_STRIDED) > 4.8                             # and say what short ones cost
    assert S.depth(21, S.FORM_STRIDED) == S.CHUNK + 3 + 3.4 * 4
