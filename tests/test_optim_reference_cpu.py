"""The optimizer evaluator (tests/optim_family.py) against torch.optim.SGD / Adam / AdamW (foreach=False, fused=False) and
clip_grad_norm_ on the CPU over five steps, the exact family against its closed form, the guard that lets test_gpu_optim.py compare
the norm bit for bit, and the restated dispatcher pinned by hand.

The comparison with torch is not by bits: torch's lerp (m + (g - m) . (1 - beta1)), its addcdiv and its scalars (1 - beta1, lr / bc1
are doubles that each kernel rounds where it uses them) round differently.  The per-element bound is a running error carried
next to a float64 evaluation of the same chain, u = 2^-24 per fp32 operation.  A quantity is a pair (x, e), |fp32 value - x| <= e:
    c . a       c a scalar   (c x,  |c| e + 2 u |c x|)                one rounding for the product, one for the scalar's own
    a + b, a - b             (x_a +- x_b,  e_a + e_b + 2 u (|x_a| + |x_b|))   the magnitudes, not the sum: a route that
                                                                     associates differently (lerp) rounds terms of that size
    a . b                    (x_a x_b,  |x_a| e_b + |x_b| e_a + e_a e_b + u |x_a x_b|)
    sqrt(a)                  (sqrt x,  sqrt x - sqrt(max(x - e, 0)) + u sqrt x)       the larger side of a concave function
    a / b                    (x_a / x_b,  (|x_a| + e_a) / (|x_b| - e_b) - |x_a / x_b| + u |x_a / x_b|), |x_b| > e_b (asserted)
The states are carried from step to step with their errors, so the bound of step five holds the four steps before it.  The float64
evaluation is the exact value for this purpose; two fp32 evaluations (the evaluator's and torch's) differ by at most twice the
bound.  The worst ratio measured is printed (DESIGN.md §3.20 records it)."""
import math

import numpy as np
import pytest
import torch

from tests import optim_family as fam

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
STEPS = 5
N = 257


class Q:
    """a float64 value with a bound on the distance of an fp32 evaluation from it"""

    def __init__(self, x, e=0.0):
        self.x = np.asarray(x, F64)
        self.e = np.zeros_like(self.x) + e

    def scaled(self, c):
        x = c * self.x
        return Q(x, abs(c) * self.e + 2 * U * np.abs(x))

    def plus(self, o, sign=1.0):
        return Q(self.x + sign * o.x, self.e + o.e + 2 * U * (np.abs(self.x) + np.abs(o.x)))

    def times(self, o):
        x = self.x * o.x
        return Q(x, np.abs(self.x) * o.e + np.abs(o.x) * self.e + self.e * o.e + U * np.abs(x))

    def sqrt(self):
        r = np.sqrt(self.x)
        return Q(r, r - np.sqrt(np.maximum(self.x - self.e, 0.0)) + U * r)

    def over(self, o):
        assert (np.abs(o.x) > o.e).all()
        x = self.x / o.x
        return Q(x, (np.abs(self.x) + self.e) / (np.abs(o.x) - o.e) - np.abs(x) + U * np.abs(x))


def _data(seed):
    rng = np.random.default_rng(seed)
    return fam.gaussian(rng, N), [fam.gaussian(rng, N) for _ in range(STEPS)]


SGD_GRID = [dict(momentum=mu, dampening=damp, weight_decay=wd, nesterov=nest)
            for mu, damp, wd, nest in ((0.0, 0.0, 0.0, False), (0.0, 0.0, 0.05, False), (0.9, 0.0, 0.0, False), (0.9, 0.0, 0.05, False),
                                       (0.9, 0.3, 0.05, False), (0.9, 0.0, 0.0, True), (0.8, 0.0, 0.01, True))]
ADAM_GRID = [dict(weight_decay=wd, decoupled=dec, betas=betas, eps=eps)
             for wd, dec in ((0.0, False), (0.05, False), (0.05, True), (0.0, True))
             for betas, eps in (((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-3))]
worst = {"sgd": 0.0, "adam": 0.0}


@pytest.mark.parametrize("scale", (None, 0.37))
@pytest.mark.parametrize("hp", SGD_GRID, ids=lambda h: "mu%g-damp%g-wd%g-%s" % (h["momentum"], h["dampening"], h["weight_decay"], "nesterov" if h["nesterov"] else "plain"))
def test_sgd_evaluator_is_within_the_rounding_bound_of_torch(hp, scale):
    p0, grads = _data(11)
    lr = 0.05
    tp = torch.nn.Parameter(torch.tensor(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lr, foreach=False, **hp)
    p, b = p0.copy(), None
    qp, qb = Q(p0), None
    for k, g in enumerate(grads):
        tp.grad = torch.tensor(g) * (1.0 if scale is None else F32(scale))        # torch's clip multiplies the gradient in fp32
        opt.step()
        p, b = fam.sgd_step(p, g, b, lr=lr, first_step=k == 0, scale=scale, **hp)
        qg = Q(g) if scale is None else Q(g).scaled(float(F32(scale)))
        if hp["weight_decay"] != 0.0:
            qg = qg.plus(qp.scaled(hp["weight_decay"]))
        qd = qg
        if hp["momentum"] != 0.0:
            qb = qg if k == 0 else qb.scaled(hp["momentum"]).plus(qg.scaled(1.0 - hp["dampening"]))
            qd = qg.plus(qb.scaled(hp["momentum"])) if hp["nesterov"] else qb
        qp = qp.plus(qd.scaled(lr), -1.0)
        diff = np.abs(p.astype(F64) - tp.detach().numpy().astype(F64))
        ratio = float((diff / (2 * qp.e)).max())
        worst["sgd"] = max(worst["sgd"], ratio)
        assert ratio <= 1.0, (k, ratio)
        assert np.abs(p.astype(F64) - qp.x).max() <= qp.e.max() and (np.abs(p.astype(F64) - qp.x) <= qp.e).all()
    print("sgd: worst |evaluator - torch| / bound so far %.3f" % worst["sgd"])


@pytest.mark.parametrize("scale", (None, 0.37))
@pytest.mark.parametrize("hp", ADAM_GRID, ids=lambda h: "wd%g-%s-b%g-eps%g" % (h["weight_decay"], "adamw" if h["decoupled"] else "adam", h["betas"][0], h["eps"]))
def test_adam_evaluator_is_within_the_rounding_bound_of_torch(hp, scale):
    p0, grads = _data(12)
    lr = 0.01
    b1, b2 = hp["betas"]
    tp = torch.nn.Parameter(torch.tensor(p0.copy()))
    cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
    opt = cls([tp], lr=lr, betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False, fused=False)
    p, m, v = p0.copy(), np.zeros(N, F32), np.zeros(N, F32)
    qp, qm, qv = Q(p0), Q(np.zeros(N)), Q(np.zeros(N))
    for k, g in enumerate(grads):
        step = k + 1
        tp.grad = torch.tensor(g) * (1.0 if scale is None else F32(scale))
        opt.step()
        p, m, v = fam.adam_step(p, g, m, v, step, lr=lr, scale=scale, **hp)
        qg = Q(g) if scale is None else Q(g).scaled(float(F32(scale)))
        qp1 = qp
        if hp["weight_decay"] != 0.0:
            if hp["decoupled"]:
                qp1 = qp.plus(qp.scaled(lr * hp["weight_decay"]), -1.0)
            else:
                qg = qg.plus(qp.scaled(hp["weight_decay"]))
        qm = qm.scaled(b1).plus(qg.scaled(1.0 - b1))
        qv = qv.scaled(b2).plus(qg.scaled(1.0 - b2).times(qg))
        den = qv.sqrt().scaled(1.0 / math.sqrt(1.0 - b2 ** step)).plus(Q(np.full(N, hp["eps"]), U * hp["eps"]))
        qp = qp1.plus(qm.over(den).scaled(lr / (1.0 - b1 ** step)), -1.0)
        st = opt.state[tp]
        for name, ours, theirs, q in (("p", p, tp.detach().numpy(), qp), ("m", m, st["exp_avg"].numpy(), qm), ("v", v, st["exp_avg_sq"].numpy(), qv)):
            diff = np.abs(ours.astype(F64) - theirs.astype(F64))
            ratio = float((diff / np.maximum(2 * q.e, 1e-300)).max())
            worst["adam"] = max(worst["adam"], ratio)
            assert ratio <= 1.0, (name, k, ratio)
            assert (np.abs(ours.astype(F64) - q.x) <= q.e).all(), (name, k)
    print("adam: worst |evaluator - torch| / bound so far %.3f" % worst["adam"])


def test_skipped_steps_are_skipped_not_multiplied_through():
    """weight_decay == 0 with p = +-Inf leaves g untouched (0 . Inf would be NaN); scale None equals scale 1.0 by bits"""
    p = np.array([np.inf, -np.inf, 1.0], F32)
    g = np.array([1.0, 2.0, 3.0], F32)
    q, b = fam.sgd_step(p, g, None, lr=0.5, momentum=0.9, first_step=True)
    assert np.array_equal(b, g) and np.array_equal(q, np.array([np.inf, -np.inf, -0.5], F32))
    rng = np.random.default_rng(5)
    p, g = fam.gaussian(rng, 64), fam.gaussian(rng, 64)
    assert np.array_equal(fam.sgd_step(p, g, lr=0.1)[0], fam.sgd_step(p, g, lr=0.1, scale=1.0)[0])
    z = np.zeros(64, F32)
    a = fam.adam_step(p, g, z, z, 1, weight_decay=0.0, decoupled=True)
    for x, y in zip(a, fam.adam_step(p, g, z, z, 1, weight_decay=0.0, decoupled=False)):
        assert np.array_equal(x, y)
    with np.errstate(all="ignore"):                       # eps = 0 with v = 0: m / 0 with m = 0 is NaN, for that element alone
        out = fam.adam_step(np.ones(3, F32), np.array([0.0, 1.0, -0.0], F32), np.zeros(3, F32), np.zeros(3, F32), 1, eps=0.0)[0]
    assert np.isnan(out[0]) and np.isfinite(out[1]) and np.isnan(out[2])


@pytest.mark.parametrize("n", (1, 7, 4097))
def test_the_exact_family_equals_its_closed_form_by_bits(n):
    f = fam.exact_family(n)
    s = f["sgd"]
    p, b = s["p0"], None
    for k in range(5):
        p, b = fam.sgd_step(p, s["g"], b, lr=s["lr"], momentum=s["momentum"], first_step=k == 0)
        assert p.tobytes() == s["closed"][k][0].tobytes() and b.tobytes() == s["closed"][k][1].tobytes(), k
    a = f["adam"]
    out = fam.adam_step(a["p0"], a["g"], np.zeros(n, F32), np.zeros(n, F32), 1, lr=a["lr"], betas=a["betas"], eps=a["eps"])
    for got, want in zip(out, a["closed"]):
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("seed,counts", fam.NORM_CASES, ids=lambda v: str(v) if isinstance(v, int) else "T%d" % len(v))
def test_the_guard_clears_in_all_three_orders_for_every_norm_case(seed, counts):
    grads = fam.norm_data(seed, counts)
    results = [fam.grad_norm(grads, 1.0, order) for order in fam.ORDERS]
    for out, wide in results:
        assert fam.guard(wide), (seed, wide)
        assert out.tobytes() == results[0][0].tobytes()


def test_grad_norm_is_torch_clip_grad_norm():
    for seed, counts in fam.NORM_CASES:
        grads = fam.norm_data(seed, counts)
        for max_norm in (0.5, 1e9, math.inf):
            out, _ = fam.grad_norm(grads, max_norm)
            params = [torch.nn.Parameter(torch.zeros(len(g))) for g in grads]
            for q, g in zip(params, grads):
                q.grad = torch.tensor(g.copy())
            total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
            assert abs(float(total) - float(out[0])) <= 4 * U * math.sqrt(sum(counts)) * float(out[0]) + 1e-30      # torch sums squares in fp32
            clipped = np.concatenate([q.grad.numpy() for q in params])
            ours = np.concatenate(grads) * out[1]
            assert np.abs(clipped - ours).max() <= 8 * U * math.sqrt(sum(counts)) * np.abs(ours).max() + 1e-30
            if max_norm >= float(out[0]) + 1e-3:
                assert out[1] == 1.0
    assert fam.grad_norm([np.array([3.0], F32), np.array([4.0], F32)], 2.5)[0].tolist() == [5.0, F32(2.5 / (5.0 + 1e-6))]
    with np.errstate(all="ignore"):
        nan, inf = fam.grad_norm([np.array([1.0, np.nan], F32)], 1.0)[0], fam.grad_norm([np.array([-np.inf, 1.0], F32)], 1.0)[0]
        both = fam.grad_norm([np.array([np.inf], F32)], math.inf)[0]
    assert np.isnan(nan).all() and inf[0] == np.inf and inf[1] == 0.0 and both[0] == np.inf and np.isnan(both[1])


def test_the_restated_dispatcher_pinned_by_hand():
    A = 1 << 20                                              # a 16-byte aligned address
    assert fam.BOUNDS == (4096, 64, 8192, 8, 3152) and fam.ARG_BYTES <= 4096
    assert fam.mode_of([A, A + 16, A + 4096]) == 0 and fam.mode_of([A + 4, A + 20]) == 1 and fam.mode_of([A + 12, A + 12 + 160]) == 3
    assert fam.mode_of([A, A + 4]) is None and fam.mode_of([A, A, A, A + 8]) is None and fam.mode_of([A, A], force_scalar=True) is None
    assert fam.plan([(1, [A, A])]) == (1, 1, 1, 0)
    assert fam.plan([(4096, [A, A])]) == (1, 1, 1, 0) and fam.plan([(4097, [A, A])]) == (1, 2, 1, 0)
    assert fam.plan([(4096, [A + 4, A + 4])]) == (1, 2, 1, 0)          # the view starts one float early: 4097 positions
    assert fam.plan([(4095, [A + 4, A + 4])]) == (1, 1, 1, 0)
    assert fam.plan([(4096, [A + 4, A + 8])]) == (1, 1, 0, 1)          # scalar: the tensor itself is cut
    assert fam.plan([(4096, [A + 4, A + 4])], force_scalar=True) == (1, 1, 0, 1)
    assert fam.plan([(8193, [A, A, A, A])] * 3 + [(1, [A, A + 4, A, A])]) == (1, 10, 3, 1)
    assert fam.plan([(1, [A, A])] * 64)[:2] == (1, 64) and fam.plan([(1, [A, A])] * 65)[:2] == (2, 65) and fam.plan([(1, [A, A])] * 129)[:2] == (3, 129)
    assert fam.norm_plan((1,)) == (2, 1) and fam.norm_plan((8192, 8193)) == (2, 3) and fam.norm_plan((1,) * 65) == (3, 65)
    assert fam.grid(5, 256) == 5 and fam.grid(2048, 256) == 2048 and fam.grid(2049, 256) == 2049 and fam.grid(9, 1) == 9 and fam.grid(8, 1) == 8
    assert fam.grid(100, 1) == 9
