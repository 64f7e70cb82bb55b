"""CPU-tier checks of tests/attention_family.py, the reference of tests/test_gpu_attention.py: the evaluator equals the closed form by
bits on the exact family (forward and backward, three key-tile sizes, two key orders); on every Gaussian case of the GPU file torch's
fp32 scaled_dot_product_attention with its autograd and the fp32 evaluator lie inside every bound against torch in float64; and the
bounds are not vacuous: every mutation of the evaluator breaks a bound or a bit comparison on every case it applies to.  The hand-pinned
dispatcher restatement is in tests/test_attention_glue_cpu.py, next to the constants it reads."""
import numpy as np
import pytest

from tests import attention_family as A

F32 = np.float32
NAMES_F, NAMES_B = ("o", "save_max", "save_sum"), ("dq", "dk", "dv")


def same(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and bool((nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all())


def _ids(c):
    return "x".join(str(v) for v in c[:4]) + ("c" if c[4] else "")


@pytest.mark.parametrize("case", A.EXACT_CASES, ids=_ids)
def test_the_evaluator_equals_the_closed_form_by_bits(case):
    BH, Sq, Sk, D, causal, sizes, layout, scale = case
    d = A.exact_family(BH, Sq, Sk, D, causal, sizes, scale, layout)
    assert d["backward_ok"] == (layout == "diagonal" or (not causal and not set(sizes) & {3, 5, 7}))
    assert (np.exp(F32(0)) == 1 and np.exp(F32(-A.M_HIGH)) == 0)      # the two values the family rests on
    for tile, reverse in ((32, False), (32, True), (7, False), (7, True), (64, False), (64, True)):
        o, m, l = A.evaluate(d["q"], d["k"], d["v"], causal, d["scale"], tile=tile, reverse=reverse)
        assert same(o, d["o"]) and same(m, d["save_max"]) and same(l, d["save_sum"]), (tile, reverse)
        if d["backward_ok"]:
            g = A.evaluate_backward(d["q"], d["k"], d["v"], d["o"], d["dout"], d["save_max"], d["save_sum"], causal, d["scale"], tile=tile, reverse=reverse)
            assert all(same(a, d[n]) for a, n in zip(g, NAMES_B)), (tile, reverse)
    if set(sizes) & {3, 5, 7}:      # the correctly rounded quotient: a reciprocal-multiply misses it somewhere
        count = d["support"].sum(1).astype(F32)
        num = (d["support"].astype(np.float64) @ d["v"].astype(np.float64)).astype(F32)
        assert not same((num * (F32(1) / count)[None, :, None]).astype(F32), d["o"])


def _torch_reference(d, causal, scale, dtype):
    import torch
    import torch.nn.functional as F
    t = {n: torch.tensor(d[n], dtype=dtype, requires_grad=n != "dout") for n in ("q", "k", "v", "dout")}
    o = F.scaled_dot_product_attention(t["q"], t["k"], t["v"], is_causal=causal, scale=scale)
    o.backward(t["dout"])
    return {"o": o.detach().numpy(), "dq": t["q"].grad.numpy(), "dk": t["k"].grad.numpy(), "dv": t["v"].grad.numpy()}


@pytest.mark.parametrize("case", A.GAUSSIAN_CASES, ids=_ids)
def test_torch_and_the_evaluator_lie_inside_every_bound_and_every_mutation_breaks_one(case):
    import torch
    BH, Sq, Sk, D, causal, sigma = case
    d = A.gaussian(BH, Sq, Sk, D, sigma)
    scale = A.default_scale(D)
    ref = A.reference64(d["q"], d["k"], d["v"], d["dout"], causal, scale)
    t64 = _torch_reference(d, causal, scale, torch.float64)
    for n in ("o",) + NAMES_B:
        assert np.abs(t64[n] - ref[n]).max() <= 1e-11 * max(1.0, np.abs(ref[n]).max()), n      # the float64 evaluator is torch's float64
    bound = A.bounds(d["q"], d["k"], d["v"], d["dout"], causal, scale, ref)
    t32 = _torch_reference(d, causal, scale, torch.float32)
    worst_t = {n: A.worst_fraction(t32[n], t64[n], bound[n]) for n in ("o",) + NAMES_B}
    o, m, l = A.evaluate(d["q"], d["k"], d["v"], causal, scale)
    g = A.evaluate_backward(d["q"], d["k"], d["v"], o, d["dout"], m, l, causal, scale)
    got = dict(zip(NAMES_F + NAMES_B, (o, m, l) + g))
    worst_e = {n: A.worst_fraction(got[n], ref[n], bound[n]) for n in got}
    print("worst fraction of the bound", case, "torch fp32", {n: "%.4f" % w for n, w in worst_t.items()}, "evaluator fp32", {n: "%.4f" % w for n, w in worst_e.items()})
    assert all(w <= 1.0 for w in worst_t.values()), worst_t
    assert all(w <= 1.0 for w in worst_e.values()), worst_e

    # the mutations, with a key tile of 8 so that the rescaling happens wherever Sk > 8
    tile = 8

    def broken(forward_mut=None, backward_mut=None):
        o, m, l = A.evaluate(d["q"], d["k"], d["v"], causal, scale, tile=tile, mutate=forward_mut)
        g = A.evaluate_backward(d["q"], d["k"], d["v"], got["o"], d["dout"], got["save_max"], got["save_sum"], causal, scale, tile=tile, mutate=backward_mut)
        out = dict(zip(NAMES_F + NAMES_B, (o, m, l) + g))
        return max(A.worst_fraction(out[n], ref[n], bound[n]) for n in out) > 1.0

    assert not broken()                                    # the unmutated evaluator on that tile passes
    assert broken("drop_key")
    assert broken("scale2") and broken(None, "scale2")
    if (min(Sq, Sk) if causal else Sk) > tile:      # some row sees more than one tile
        assert broken("no_rescale")
    if causal:
        assert broken("mask_plus") and broken(None, "mask_plus")
        if Sq >= 2 and Sk >= 2:
            assert broken("mask_minus") and broken(None, "mask_minus")
    assert broken(None, "no_delta")
    assert broken(None, "swap")


def test_the_mutations_break_the_bit_comparison_on_the_exact_family():
    d = A.exact_family(3, 65, 129, 64, False, (1, 2, 4, 8, 16))
    for mut in ("drop_key", "no_rescale", "scale2"):
        o, m, l = A.evaluate(d["q"], d["k"], d["v"], False, d["scale"], mutate=mut)
        assert not (same(o, d["o"]) and same(m, d["save_max"]) and same(l, d["save_sum"])), mut
    c = A.exact_family(1, 257, 257, 64, True, (1, 2, 4, 8, 16))      # the permuted layout: members lie next to the diagonal somewhere
    for mut in ("mask_plus", "mask_minus"):
        o, m, l = A.evaluate(c["q"], c["k"], c["v"], True, c["scale"], mutate=mut)
        assert not (same(o, c["o"]) and same(l, c["save_sum"])), mut
    for mut in ("no_delta", "swap", "scale2"):
        g = A.evaluate_backward(d["q"], d["k"], d["v"], d["o"], d["dout"], d["save_max"], d["save_sum"], False, d["scale"], mutate=mut)
        assert not all(same(a, d[n]) for a, n in zip(g, NAMES_B)), mut
