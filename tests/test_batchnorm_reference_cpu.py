"""The batch-normalization evaluator (tests/batchnorm_family.py) against torch on the CPU, the exact family against its closed
form, and the guard that lets test_gpu_batchnorm.py compare Gaussian data bit for bit.

The per-element bounds, u = 2^-24 per fp32 operation, for any evaluation that rounds the mean and invstd to fp32 once (relative
error u each; 2 u is allowed for invstd so that torch's own route to it is covered) and then takes the three rounded steps:
    e_d  = u |d| + u |mean|                    d = x - mean: one subtract of a mean that is off by u |mean|
    e_h  = e_d . invstd + 3 u |h|              h = d . invstd: invstd's 2 u and the multiply's u
    e_y  = e_h |gamma| + u |h gamma| + u |y|   the multiply by gamma, the add of beta
    dx = k ((dy - mb) - xh mg), k = gamma . invstd (3 u), mb and mg rounded once (u each):
    e_dgamma = sum |dy| e_h + u |dgamma|,   e_dbeta = u |dbeta|;   mg = dgamma / n carries e_dgamma / n
    e_dx = |k| (u |dy - mb| + u |mb| + |mg| e_h + |xh| e_dgamma / n + 2 u |xh mg| + u |(dy - mb) - xh mg|) + 4 u |dx|
A float64 evaluation is the exact value for this purpose; two fp32 evaluations differ by at most twice the bound."""
import numpy as np
import pytest
import torch

from tests import batchnorm_family as fam

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
SHAPES = ((4, 3, 5), (3, 6, 49), (16, 6, 1), (2, 7, 130), (64, 2, 64))


def _bounds(d):
    """the bounds above from float64 values"""
    x, dy = d["x"].astype(F64), d["dy"].astype(F64)
    n = x.shape[0] * x.shape[2]
    mean = x.mean(axis=(0, 2), keepdims=True)
    var = x.var(axis=(0, 2), keepdims=True)
    inv = 1.0 / np.sqrt(var + d["eps"])
    g, b = d["gamma"].astype(F64).reshape(1, -1, 1), d["beta"].astype(F64).reshape(1, -1, 1)
    dd = x - mean
    h = dd * inv
    y = h * g + b
    e_h = (U * np.abs(dd) + U * np.abs(mean)) * inv + 3 * U * np.abs(h)
    e_y = e_h * np.abs(g) + U * np.abs(h * g) + U * np.abs(y)
    mb, mg = dy.mean(axis=(0, 2), keepdims=True), (dy * h).mean(axis=(0, 2), keepdims=True)
    core = (dy - mb) - h * mg
    dx = g * inv * core
    e_dgamma = (np.abs(dy) * e_h).sum(axis=(0, 2)) + U * np.abs(n * mg.reshape(-1))
    e_dx = np.abs(g * inv) * (U * np.abs(dy - mb) + U * np.abs(mb) + np.abs(mg) * e_h + np.abs(h) * e_dgamma.reshape(1, -1, 1) / n
                              + 2 * U * np.abs(h * mg) + U * np.abs(core)) + 4 * U * np.abs(dx)
    e_dbeta = U * np.abs(n * mb.reshape(-1))
    return {"y": e_y, "dx": e_dx, "dgamma": e_dgamma, "dbeta": e_dbeta, "mean": mean.reshape(-1), "var": var.reshape(-1), "inv": inv.reshape(-1), "n": n,
            "abs_dbeta": np.abs(dy).sum(axis=(0, 2)), "abs_dgamma": np.abs(dy * h).sum(axis=(0, 2))}


def _torch(d, dtype, training=True, momentum=0.1):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = t(d["x"]).requires_grad_(True)
    g, b = t(d["gamma"]).requires_grad_(True), t(d["beta"]).requires_grad_(True)
    rm, rv = t(d["running_mean"]), t(d["running_var"])
    y = torch.nn.functional.batch_norm(x, rm, rv, g, b, training, momentum, d["eps"])
    out = {"y": y.detach().numpy(), "running_mean": rm.numpy(), "running_var": rv.numpy()}
    if training:
        y.backward(t(d["dy"]))
        out.update(dx=x.grad.numpy(), dgamma=g.grad.numpy(), dbeta=b.grad.numpy())
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_evaluator_and_torch_fp32_sit_inside_the_bounds_around_torch_float64(shape):
    d = fam.gaussian_family(*shape, seed=sum(shape))
    e = _bounds(d)
    f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], True, 0.1, d["running_mean"], d["running_var"])
    b = fam.backward(d["x"], d["dy"], d["gamma"], f["save_mean"], f["save_invstd"])
    t64, t32 = _torch(d, torch.float64), _torch(d, torch.float32)
    n = e["n"]
    # the saved statistics: one rounding of an accurate fp64 value
    assert (np.abs(f["save_mean"] - e["mean"]) <= U * np.abs(e["mean"]) * 1.001).all()
    assert (np.abs(f["save_invstd"] - e["inv"]) <= U * e["inv"] * 1.001).all()
    assert (np.abs(f["running_mean"] - t64["running_mean"]) <= 2 * U * np.abs(t64["running_mean"]) + 1e-30).all()
    if n > 1:
        assert (np.abs(f["running_var"] - t64["running_var"]) <= 2 * U * np.abs(t64["running_var"])).all()
        assert (np.abs(t32["running_var"] - t64["running_var"]) <= 8 * U * np.abs(t64["running_var"]) * (1 + e["mean"] ** 2 / e["var"])).all()
    for name, mine in (("y", f["y"]), ("dx", b["dx"]), ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
        err = np.abs(mine.astype(F64) - t64[name])
        assert (err <= e[name] * 1.001).all(), (name, float((err / e[name]).max()))
        err32 = np.abs(t32[name].astype(F64) - t64[name])
        slack = n * U * e["abs_" + name] if name in ("dgamma", "dbeta") else 0.0      # torch's fp32 sums: n u sum |t| at most
        assert (err32 <= 2 * e[name] + slack).all(), (name, float((err32 / e[name]).max()))
    # inference: the evaluator on the running statistics against torch float64
    inf = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], False, 0.1, d["running_mean"], d["running_var"])
    i64 = _torch(d, torch.float64, training=False)
    x64, rm, rv = d["x"].astype(F64), d["running_mean"].astype(F64).reshape(1, -1, 1), d["running_var"].astype(F64).reshape(1, -1, 1)
    inv = 1 / np.sqrt(rv + d["eps"])
    h = (x64 - rm) * inv
    g = np.abs(d["gamma"].astype(F64)).reshape(1, -1, 1)
    bound = (U * np.abs(x64 - rm) * inv + 3 * U * np.abs(h)) * g + U * np.abs(h) * g + U * np.abs(i64["y"])
    assert (np.abs(inf["y"].astype(F64) - i64["y"]) <= bound * 1.001).all()
    assert (fam.forward(d["x"], None, None, d["eps"], False, 0.1, f["save_mean"], d["running_var"])["y"]
            == fam.apply(d["x"], f["save_mean"], (1 / np.sqrt(d["running_var"].astype(F64) + d["eps"])).astype(F32))).all()


@pytest.mark.parametrize("pattern, shape, constant", [("pm1", (2, 3, 5), ()), ("pm1", (64, 2, 65), (1,)), ("m3", (4, 3, 7), (0,)),
                                                      ("m3", (8, 65, 1), (3, 64)), ("pm1", (2, 2, 100000), ()), ("m3", (200000, 1, 1), ())])
def test_the_exact_family_reproduces_its_closed_form_by_bits(pattern, shape, constant):
    d = fam.exact_family(*shape, pattern, seed=7, constant=constant)
    for order in fam.ORDERS:
        f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], True, 0.1, order=order)
        b = fam.backward(d["x"], d["dy"], d["gamma"], f["save_mean"], f["save_invstd"], order=order)
        for name, got in (("y", f["y"]), ("save_mean", f["save_mean"]), ("save_invstd", f["save_invstd"]), ("dx", b["dx"]),
                          ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
            assert got.tobytes() == d[name].tobytes() or (np.isnan(got) == np.isnan(d[name])).all() and (got[~np.isnan(got)] == d[name][~np.isnan(got)]).all(), name
    for c in constant:      # eps > 0: y = beta exactly; eps = 0: NaN
        yc = f["y"][:, c, :]
        assert (yc == d["beta"][c]).all() if d["eps"] > 0 else np.isnan(yc).all()
    # a batch permutation permutes the outputs and leaves the statistics alone
    perm = np.random.default_rng(3).permutation(shape[0])
    fp = fam.forward(d["x"][perm], d["gamma"], d["beta"], d["eps"])
    assert fp["y"].tobytes() == f["y"][perm].tobytes() and fp["save_mean"].tobytes() == f["save_mean"].tobytes()


@pytest.mark.parametrize("case", fam.GAUSSIAN_CASES + sum(fam.OTHER_CASES.values(), ()), ids=lambda c: "x".join(map(str, c)))
def test_the_guard_clears_every_gaussian_case_of_the_gpu_file(case):
    """margin >= 2^10 . bound for every rounded scalar, and three summation orders give the same fp32 bits.  A seed that fails is
    replaced in batchnorm_family.GAUSSIAN_CASES."""
    N, C, inner, seed = case
    d = fam.gaussian_family(N, C, inner, seed)
    runs = []
    for momentum in (0.1, 1.0):
        for order in fam.ORDERS:
            f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], True, momentum, d["running_mean"], d["running_var"], order=order)
            b = fam.backward(d["x"], d["dy"], d["gamma"], f["save_mean"], f["save_invstd"], order=order)
            assert fam.guard_ratio(f["wide"]) >= 2.0 ** 10, (momentum, order, fam.guard_ratio(f["wide"]))
            assert fam.guard_ratio(b["wide"], True) >= 2.0 ** 10, (order, fam.guard_ratio(b["wide"], True))
            runs.append(b"".join(a.tobytes() for a in (f["y"], f["save_mean"], f["save_invstd"], f["running_mean"], f["running_var"], b["dx"],
                                                       b["dgamma"], b["dbeta"])))
        assert runs[-1] == runs[-2] == runs[-3]


def test_the_dispatcher_covers_the_forms_and_slice_counts_the_gpu_file_needs():
    forms = {fam.pick_form(N, C, inner) for N, C, inner, _ in fam.GAUSSIAN_CASES}
    assert forms == {fam.FORM_ONE, fam.FORM_SPLIT, fam.FORM_ROWS}
    S = {(fam.pick_form(N, C, inner), fam.slices(fam.pick_form(N, C, inner), N, C, inner)) for N, C, inner, _ in fam.GAUSSIAN_CASES}
    assert (fam.FORM_SPLIT, 2) in S and (fam.FORM_ROWS, 1) in S and (fam.FORM_ROWS, 2) in S, S
    assert fam.slices(fam.FORM_SPLIT, 1, 1, 200000) == 49 and fam.slices(fam.FORM_ROWS, 200000, 1, 1) == 195      # the largest S at 2 . 10^5 elements
    assert fam.slices(fam.FORM_SPLIT, 2, 3, 5) == 1 and fam.slices(fam.FORM_ONE, 2, 3, 5) == 0
    for n in (4095, 4096, 4097, 8191, 8192, 8193):
        assert any(N * inner == n for N, C, inner, _ in fam.GAUSSIAN_CASES if inner > 1), n


def test_the_shifted_sums_are_accurate_where_fp32_one_pass_is_not():
    """Why the definition is what it is: mean 1e4, sigma 1e-3."""
    rng = np.random.default_rng(5)
    x = (1e4 + 1e-3 * rng.standard_normal((64, 1, 64))).astype(F32)
    f = fam.forward(x, eps=0.0)
    x64 = x.astype(F64).reshape(-1)
    two_pass = ((x64 - x64.mean()) ** 2).mean()
    assert abs(f["wide"][0]["var64"] - two_pass) <= 1e-6 * two_pass
    xf = x.reshape(-1)
    m32, q32 = np.cumsum(xf, dtype=F32)[-1] / F32(xf.size), np.cumsum(xf * xf, dtype=F32)[-1] / F32(xf.size)      # fp32 chains
    one_pass = q32 - m32 * m32
    assert abs(F64(one_pass) - two_pass) > 1.0 * two_pass
