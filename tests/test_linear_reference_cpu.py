"""The reference of the dense layer (tests/linear_family.py) on the CPU.

fma32 is one correctly rounded fused multiply-add (against exact rational arithmetic, double-rounding ties included); on the exact
family the evaluator equals torch.nn.functional.linear and autograd bit for bit, with a bias and relu, and the backward rules of
tanh and sigmoid equal aten's tanh_backward / sigmoid_backward on dyadic outputs; on standard-normal data torch's fp32 layer sits
inside the bound the GPU tests use around torch's float64 layer, and so does the evaluator; the evaluator equals
tests/dnn_family.py's 1 x 1 convolution; the slice orders of dw and db are the ones the header states."""
from fractions import Fraction

import numpy as np
import pytest

from tests import dnn_family as G
from tests import linear_family as fam

torch = pytest.importorskip("torch")
F32, F64 = np.float32, np.float64
SHAPES = [(1, 1, 1), (5, 7, 3), (33, 31, 65), (70, 100, 37), (600, 9, 40)]


def _round_to_f32(q):
    """the fp32 nearest to the rational q, ties to even"""
    c = F32(float(q))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        d = abs(Fraction(float(cand)) - q)
        even = (int(np.asarray(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, cand)
    return best[1]


def test_fma32_is_one_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(1500).astype(F32) for _ in range(3))
    # double-rounding traps: 24929 . 673 = 2^24 + 1, so a . b is EXACTLY the midpoint of 1 and 1 + 2^-23 and c decides; the fp64 sum
    # loses c, lands on the tie and rounds to even
    mid = (F32(24929 * 2.0 ** -12), F32(673 * 2.0 ** -12))
    traps = [(mid[0], mid[1], F32(2.0 ** -60)), (-mid[0], mid[1], F32(-2.0 ** -60)), (mid[0], mid[1], F32(-2.0 ** -60)), (mid[0], -mid[1], F32(2.0 ** -90))]
    a, b, c = (np.concatenate([v, np.array([t[i] for t in traps], F32)]) for i, v in enumerate((a, b, c)))
    got = fam.fma32(a, b, c)
    twice = (c.astype(F64) + a.astype(F64) * b.astype(F64)).astype(F32)
    want = np.array([_round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want[-4:], np.array([1 + 2.0 ** -23, -1 - 2.0 ** -23, 1, -1], F32))
    assert (twice[-4:-2] != want[-4:-2]).all()                                              # the traps do catch the plain fp64 sum
    assert fam.same(fam.fma32(F32(np.inf), F32(0.0), F32(1.0)), F32(np.nan)) and fam.fma32(F32(2.0), F32(3.0), F32(-np.inf)) == -np.inf
    assert np.signbit(fam.fma32(F32(-0.0), F32(1.0), F32(-0.0))) and not np.signbit(fam.fma32(F32(0.0), F32(0.0), F32(-0.0)))


@pytest.mark.parametrize("M,K,N", SHAPES)
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("has_bias", [False, True])
def test_the_evaluator_equals_torch_bit_for_bit_on_the_exact_family(M, K, N, act, has_bias):
    x, w, dy, b = fam.exact(np.random.default_rng(M + K + N), M, K, N)
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    ty = torch.nn.functional.linear(tx, tw, tb if has_bias else None)
    if act == "relu":
        ty = torch.relu(ty)
    ty.backward(torch.tensor(dy))
    y = fam.forward(x, w, b if has_bias else None, act)
    assert y.dtype == F32 and np.array_equal(ty.detach().numpy(), y)
    dz, dx, dw, db = fam.backward(x, w, y, dy, act)
    assert all(a.dtype == F32 for a in (dz, dx, dw, db))
    assert np.array_equal(tx.grad.numpy(), dx) and np.array_equal(tw.grad.numpy(), dw)
    assert not has_bias or np.array_equal(tb.grad.numpy(), db)
    assert np.array_equal(db.astype(F64), dz.astype(F64).sum(axis=0))
    if act == "relu" and y.size > 50:
        assert (y == 0).any() and (y > 0).any() and not np.array_equal(dz, dy)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_the_backward_rules_of_tanh_and_sigmoid_equal_atens_on_dyadic_outputs(act):
    M, K, N = 70, 9, 45
    rng = np.random.default_rng(3)
    y, dy = fam.dyadic_outputs(rng, M, N, act)
    x, w = fam.exact(rng, M, K, N)[:2]
    dz, dx, dw, db = fam.backward(x, w, y, dy, act)
    rule = torch.ops.aten.tanh_backward if act == "tanh" else torch.ops.aten.sigmoid_backward
    tz = rule(torch.tensor(dy), torch.tensor(y))
    assert np.array_equal(tz.numpy(), dz)
    y64 = y.astype(F64)
    assert np.array_equal(dz.astype(F64), dy * (1 - y64 * y64) if act == "tanh" else dy * ((1 - y64) * y64))
    assert np.array_equal((tz @ torch.tensor(w)).numpy(), dx) and np.array_equal((tz.T @ torch.tensor(x)).numpy(), dw)
    assert np.array_equal(tz.sum(dim=0).numpy(), db)


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_tanh_and_sigmoid_forward_are_within_1e5_of_torch(act):
    x, w, _, b = fam.gaussian(np.random.default_rng(4), 40, 30, 20)
    y = fam.forward(x, w, b, act)
    ty = (torch.tanh if act == "tanh" else torch.sigmoid)(torch.nn.functional.linear(torch.tensor(x), torch.tensor(w), torch.tensor(b))).numpy()
    assert np.abs(y - ty).max() <= 1e-5


@pytest.mark.parametrize("M,K,N", SHAPES[1:])
def test_torch_fp32_and_the_evaluator_sit_inside_the_bound_around_float64(M, K, N):
    x, w, dy, b = fam.gaussian(np.random.default_rng(M), M, K, N)
    x64, w64, z64, b64 = (a.astype(F64) for a in (x, w, dy, b))
    limits = {"y": fam.bound(K, np.abs(x64), np.abs(w64.T), 1) + fam.U * np.abs(b64), "dx": fam.bound(N, np.abs(z64), np.abs(w64)),
              "dw": fam.bound(M, np.abs(z64.T), np.abs(x64)), "db": (M + 1) * fam.U * np.abs(z64).sum(axis=0)}
    t64 = [torch.tensor(a, requires_grad=True) for a in (x64, w64, b64)]
    torch.nn.functional.linear(*t64).backward(torch.tensor(z64))
    ref = {"y": x64 @ w64.T + b64, "dx": t64[0].grad.numpy(), "dw": t64[1].grad.numpy(), "db": t64[2].grad.numpy()}
    assert np.allclose(ref["dx"], z64 @ w64, rtol=1e-12, atol=1e-12) and np.allclose(ref["dw"], z64.T @ x64, rtol=1e-12, atol=1e-12)
    t32 = [torch.tensor(a, requires_grad=True) for a in (x, w, b)]
    ty = torch.nn.functional.linear(*t32)
    ty.backward(torch.tensor(dy))
    got = {"y": ty.detach().numpy(), "dx": t32[0].grad.numpy(), "dw": t32[1].grad.numpy(), "db": t32[2].grad.numpy()}
    _, dx, dw, db = fam.backward(x, w, None, dy, None)
    ours = {"y": fam.forward(x, w, b), "dx": dx, "dw": dw, "db": db}
    for name in ref:
        assert fam.worst_ratio(got[name], ref[name], limits[name]) <= 1.0, ("torch", name)
        assert fam.worst_ratio(ours[name], ref[name], limits[name]) <= 1.0, ("evaluator", name)


@pytest.mark.parametrize("M,K,N", SHAPES[:4])
def test_the_evaluator_equals_the_1x1_convolution_evaluator_by_bits(M, K, N):
    x, w, dy, b = fam.exact(np.random.default_rng(M * N), M, K, N)
    x4, w4, dy4 = x.reshape(M, K, 1, 1), w.reshape(N, K, 1, 1), dy.reshape(M, N, 1, 1)
    same = lambda a, b_: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b_, F32).reshape(np.shape(a)).view(np.uint32))
    assert same(fam.forward(x, w), G.forward(G.as_int(x4), G.as_int(w4)))
    assert same(fam.grad_x(dy, w), G.grad_x(G.as_int(dy4), G.as_int(w4), 1, 1))
    assert same(fam.grad_w(dy, x), G.grad_w(G.as_int(x4), G.as_int(dy4), 1, 1))


def test_the_slice_orders_are_the_stated_ones():
    """values whose sum depends on the order: the evaluator follows the stated one and no other"""
    M, N = 520, 3
    assert fam.act_plan(M, N) == (260, 2) and fam.dw_plan(M, 2, N)[1:] == (9, 2)
    rng = np.random.default_rng(6)
    dz = (rng.standard_normal((M, N)) * 10.0 ** rng.integers(-3, 4, (M, N))).astype(F32)
    want = np.zeros(N, F32)
    for s in range(2):
        groups = []
        for g in range(4):
            acc = F32(0.0) * np.ones(N, F32)
            for m in range(260 * s + g, min(M, 260 * (s + 1)), 4):
                acc = (acc + dz[m]).astype(F32)
            groups.append(acc)
        part = (((groups[0] + groups[1]) + groups[2]) + groups[3]).astype(F32)
        want = part if s == 0 else (want + part).astype(F32)
    assert np.array_equal(fam.grad_b(dz).view(np.uint32), want.view(np.uint32))
    x = rng.standard_normal((M, 2)).astype(F32)
    first, second = fam.chain(dz[:288].T, x[:288]), fam.chain(dz[288:].T, x[288:])
    assert np.array_equal(fam.grad_w(dz, x).view(np.uint32), (first + second).astype(F32).view(np.uint32))
    one = fam.chain(dz.T, x)                                                                  # a single chain over all of M: other bits somewhere
    assert one.shape == (N, 2)
    # the chain continues over the zero-filled tail of the last step: a -0.0 becomes +0.0 there, and only there
    tiny = np.array([[F32(-1e-30)]], F32)
    assert np.signbit(fam.chain(np.tile(tiny, (1, 32)), np.full((32, 1), F32(1e-30)))[0, 0])
    assert not np.signbit(fam.chain(np.tile(tiny, (1, 31)), np.full((31, 1), F32(1e-30)))[0, 0])
