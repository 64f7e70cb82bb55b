"""The layer / group normalization evaluator (tests/groupnorm_family.py) against torch on the CPU, the exact family against its
closed form, and the guard that says where test_gpu_groupnorm.py may compare Gaussian data bit for bit.

The per-element bounds come from u = 2^-24 per fp32 operation (groupnorm_family.y_bound and dx_bound carry the derivation): an
evaluation whose mean is within u (|mean| + E|x - mean|) and whose invstd is within 2 u (`_bounds` says why) and which then takes
the rounded steps.  The evaluator's own saved scalars are held to one rounding, u, of the fp64 values.  A float64
evaluation is the exact value for this purpose; an fp32 evaluation by another route must lie inside twice the bounds."""
import numpy as np
import pytest
import torch

from tests import batchnorm_family as B
from tests import groupnorm_family as fam

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
# (N, G, D, inner): layer norm is G = 1, inner = 1
SHAPES = ((5, 1, 7, 1), (3, 1, 64, 1), (6, 1, 300, 1), (2, 1, 1, 1), (4, 3, 2, 5), (3, 2, 1, 49), (2, 6, 1, 16), (5, 1, 6, 9), (3, 4, 4, 1))


def _torch(d, dtype):
    N, G, D, inner = d["x"].shape
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    g, b = t(d["gamma"]).requires_grad_(True), t(d["beta"]).requires_grad_(True)
    if G == 1 and inner == 1:
        x = t(d["x"].reshape(N, D)).requires_grad_(True)
        y = torch.nn.functional.layer_norm(x, (D,), g, b, d["eps"])
    else:
        x = t(d["x"].reshape(N, G * D, inner)).requires_grad_(True)
        y = torch.nn.functional.group_norm(x, G, g, b, d["eps"])
    y.backward(t(d["dy"].reshape(y.shape)))
    shape = d["x"].shape
    return {"y": y.detach().numpy().reshape(shape), "dx": x.grad.numpy().reshape(shape), "dgamma": g.grad.numpy(), "dbeta": b.grad.numpy()}


def _bounds(d):
    """the bounds of y, dx, dgamma and dbeta from float64 values"""
    x, dy = d["x"].astype(F64), d["dy"].astype(F64)
    N, G, D, inner = x.shape
    M, L = N * G, D * inner
    rows = x.reshape(M, L)
    mean, var = rows.mean(axis=1), rows.var(axis=1)
    inv = 1.0 / np.sqrt(var + d["eps"])
    # the mean: one rounding, u |mean|, and one more rounding at the size of the average deviation, u E|x - mean|, which is what an
    # fp32 route to the mean costs at the least where |mean| is far below sigma; invstd: 2 u, its rounding and the route to it
    em, ei = U * (np.abs(mean) + np.abs(rows - mean[:, None]).mean(axis=1)), 2 * U * inv
    e_y = fam.y_bound(d["x"], mean, inv, d["gamma"], d["beta"], em, ei)
    e_xh = fam.y_bound(d["x"], mean, inv, None, None, em, ei).reshape(M, L)
    xh = (rows - mean[:, None]) * inv[:, None]
    g = dy.reshape(M, L) * fam._per_row(d["gamma"].astype(F64), N, G, D, inner)
    e_g = U * np.abs(g)
    mb, mg = g.mean(axis=1), (g * xh).mean(axis=1)
    e_mb = U * np.abs(mb) + e_g.mean(axis=1)
    e_mg = U * np.abs(mg) + (np.abs(g) * e_xh + e_g * np.abs(xh) + e_g * e_xh).mean(axis=1)
    dx = inv[:, None] * ((g - mb[:, None]) - xh * mg[:, None])
    e_dx = fam.dx_bound(g, xh, inv, mb, mg, e_g, e_xh, e_mb, e_mg) + 2 * U * np.abs(dx)      # invstd itself is off by u
    by = lambda v: fam._by_param(v, N, G, D, inner)
    dbeta, dgamma = by(dy.reshape(M, L)).sum(axis=1), (by(dy.reshape(M, L)) * by(xh)).sum(axis=1)
    return {"y": e_y, "dx": e_dx.reshape(x.shape), "dgamma": (np.abs(by(dy.reshape(M, L))) * by(e_xh)).sum(axis=1) + U * np.abs(dgamma),
            "dbeta": U * np.abs(dbeta), "mean": mean.reshape(N, G), "inv": inv.reshape(N, G), "n": N * inner,
            "abs_dbeta": np.abs(by(dy.reshape(M, L))).sum(axis=1), "abs_dgamma": np.abs(by(dy.reshape(M, L)) * by(xh)).sum(axis=1)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("centred", (False, True), ids=("family", "centred"))
def test_evaluator_and_torch_fp32_sit_inside_the_bounds_around_torch_float64(shape, centred):
    """The evaluator is held to torch float64 on the family's rows (means 1 and 1e4) and on centred rows (mean 0, sigma 1); torch
    fp32 is held to twice the bounds on the centred rows alone.  Its backward pass is another expression, dx = a . dy + b . x + c
    with per-row a, b, c: b . x + c cancels to u |b| |x|, an error that grows with |mean| / sigma and that the bounds of the
    three-step expression do not hold; on centred rows |x| is of sigma's size and the two expressions share the bounds.  Its fp32
    statistics are likewise only comparable where u |mean| is not far below u sigma."""
    d = fam.gaussian_family(*shape, seed=sum(shape), zero_mean=False)
    if centred:
        d["x"] = np.random.default_rng(sum(shape)).standard_normal(shape).astype(F32)
    e = _bounds(d)
    f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"])
    b = fam.backward(d["x"], d["dy"], d["gamma"], f["save_mean"], f["save_invstd"])
    t64, t32 = _torch(d, torch.float64), _torch(d, torch.float32)
    # the saved statistics: one rounding of an accurate fp64 value
    assert (np.abs(f["save_mean"] - e["mean"]) <= U * np.abs(e["mean"]) * 1.001).all()
    assert (np.abs(f["save_invstd"] - e["inv"]) <= U * e["inv"] * 1.001).all()
    for name, mine in (("y", f["y"]), ("dx", b["dx"]), ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
        print(name, "evaluator / bound", float((np.abs(mine.astype(F64) - t64[name]) / np.maximum(e[name], 1e-300)).max()),
              "torch fp32 / bound", float((np.abs(t32[name].astype(F64) - t64[name]) / np.maximum(e[name], 1e-300)).max()))
    for name, mine in (("y", f["y"]), ("dx", b["dx"]), ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
        err = np.abs(mine.astype(F64) - t64[name])
        assert (err <= e[name] * 1.001).all(), (name, float((err / np.maximum(e[name], 1e-300)).max()))
        if not centred:
            continue
        err32 = np.abs(t32[name].astype(F64) - t64[name])
        slack = e["n"] * U * e["abs_" + name] if name in ("dgamma", "dbeta") else 0.0      # torch's fp32 sums: n u sum |t| at most
        assert (err32 <= 2 * e[name] + slack).all(), (name, float((err32 / np.maximum(e[name], 1e-300)).max()))
    # without the affine parameters
    f0 = fam.forward(d["x"], None, None, d["eps"])
    assert f0["y"].tobytes() == fam.apply(d["x"], f["save_mean"], f["save_invstd"]).tobytes()
    assert f0["save_mean"].tobytes() == f["save_mean"].tobytes()


def _same(a, b):
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all()


@pytest.mark.parametrize("pattern, shape, constant", [("pm1", (5, 1, 2, 1), ()), ("pm1", (3, 1, 66, 1), (1,)), ("m3", (4, 1, 8, 1), (0,)),
                                                      ("m3", (2, 3, 2, 6), (3, 5)), ("pm1", (2, 2, 3, 50), (2,)), ("m3", (1, 1, 200000, 1), ()),
                                                      ("pm1", (3, 2, 1, 10000), ()), ("m3", (3000, 1, 4, 1), (7,))])
def test_the_exact_family_reproduces_its_closed_form_by_bits(pattern, shape, constant):
    d = fam.exact_family(*shape, pattern, seed=7, constant=constant)
    N, G, D, inner = shape
    for order in fam.ORDERS:
        f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], order=order)
        b = fam.backward(d["x"], d["dy"], d["gamma"], d["save_mean"], d["save_invstd"], order=order)
        for name, got in (("y", f["y"]), ("save_mean", f["save_mean"]), ("save_invstd", f["save_invstd"]), ("dx", b["dx"]),
                          ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
            assert _same(got, d[name]), (name, order)
    y, beta = f["y"].reshape(N * G, D * inner), fam._per_row(d["beta"], N, G, D, inner)
    for r in constant:      # eps > 0: y = beta exactly; eps = 0: NaN
        assert (y[r].view(np.uint32) == beta[r].view(np.uint32)).all() if d["eps"] > 0 else np.isnan(y[r]).all()
    # a batch permutation permutes the outputs and the statistics
    perm = np.random.default_rng(3).permutation(N)
    fp = fam.forward(d["x"][perm], d["gamma"], d["beta"], d["eps"])
    assert _same(fp["y"], f["y"][perm]) and _same(fp["save_mean"], f["save_mean"][perm])


def test_the_array_guard_is_batchnorm_familys_guard_record_by_record():
    d = fam.gaussian_family(5, 3, 2, 7, 11)
    f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"])
    b = fam.backward(d["x"], d["dy"], d["gamma"], f["save_mean"], f["save_invstd"])
    rows = d["x"].reshape(15, 14)
    for order in fam.ORDERS:
        for r in range(15):      # _sums is _sum, row by row
            assert fam._sums(rows.astype(F64), order)[r] == B._sum(rows[r].astype(F64), order)
    for wide, kind, names in ((f["wide"], "forward", ("save_mean", "save_invstd")), (b["wide"], "rows", ("mb", "mg")),
                              (b["wide_param"], "params", ("dbeta", "dgamma"))):
        mine = fam.guard(wide, kind, exact=False)
        for r in range(len(wide["abs1"])):
            record = {k: (v[r] if isinstance(v, np.ndarray) else v) for k, v in wide.items()}
            record["c"] = r
            theirs = B.guard(record, backward_pass=kind != "forward")
            for name in names:
                assert mine[name][0][r] == theirs[name][0] and mine[name][1][r] == theirs[name][1], (kind, name, r)


@pytest.mark.parametrize("case", fam.GAUSSIAN_CASES + sum(fam.OTHER_CASES.values(), ()), ids=lambda c: "x".join(map(str, c)))
def test_the_guard_classifies_every_gaussian_case_of_the_gpu_file(case):
    """For every Gaussian shape and seed of the GPU file: at most 2 % of the rows and 2 % of the parameters are unguarded (fewer
    than 50 rows: none), the three summation orders give the same bits on the guarded ones and differ by at most one ulp in a
    saved scalar elsewhere, and the kernels' summation depth stays within the guard's.  A seed that fails is replaced in
    groupnorm_family.SEEDS."""
    N, G, D, inner, seed, zero_mean = case
    M, L, P, n = fam.geometry(N, G, D, inner)
    d = fam.gaussian_family(N, G, D, inner, seed, zero_mean)
    runs = []
    for order in fam.ORDERS:
        f = fam.forward(d["x"], d["gamma"], d["beta"], d["eps"], order=order)
        runs.append((f, fam.backward(d["x"], d["dy"], d["gamma"], runs[0][0]["save_mean"] if runs else f["save_mean"],
                                     runs[0][0]["save_invstd"] if runs else f["save_invstd"], order=order)))
    f0, b0 = runs[0]
    ok_f, ok_r, ok_p = fam.guarded(f0["wide"], "forward"), fam.guarded(b0["wide"], "rows"), fam.guarded(b0["wide_param"], "params")
    for ok, count in ((ok_f, M), (ok_r, M), (ok_p, P)):
        assert (~ok).sum() <= fam.UNGUARDED_CAP * count, ((~ok).sum(), count)
    ulps = lambda a, b: np.abs(a.reshape(-1).view(np.int32).astype(np.int64) - b.reshape(-1).view(np.int32).astype(np.int64))
    for f, b in runs[1:]:
        for name in ("save_mean", "save_invstd"):
            assert (ulps(f[name], f0[name])[ok_f] == 0).all() and (ulps(f[name], f0[name]) <= 1).all(), name
        assert _same(f["y"].reshape(M, L)[ok_f], f0["y"].reshape(M, L)[ok_f]) and _same(b["dx"].reshape(M, L)[ok_r], b0["dx"].reshape(M, L)[ok_r])
        for name in ("dgamma", "dbeta"):
            assert (ulps(b[name], b0[name])[ok_p] == 0).all() and (ulps(b[name], b0[name]) <= 1).all(), name
    for form in (fam.ROW_SHORT, fam.ROW_WAVE, fam.ROW_GROUP, fam.ROW_SPLIT):
        if fam.row_serves(form, L):
            assert fam.row_depth(form, N, G, D, inner) <= fam.DEPTH, (form, fam.row_depth(form, N, G, D, inner))
    for form in (fam.PARAM_COLUMNS, fam.PARAM_PLANES):
        if fam.param_serves(form, inner):
            assert fam.param_depth(form, N, G, D, inner) <= fam.DEPTH, (form, fam.param_depth(form, N, G, D, inner))


def test_the_cases_cover_the_forms_boundaries_and_slice_counts_the_gpu_file_needs():
    cases = fam.GAUSSIAN_CASES
    Ls = {D * inner for N, G, D, inner, _, _ in cases if G == 1 and inner == 1}
    assert {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257} <= Ls
    for bound in fam.BOUNDS[:4]:
        assert {bound - 1, bound, bound + 1} <= Ls, bound
    assert {1, 2, 3, 5, 63, 64, 65, 257} <= {N * G for N, G, D, inner, _, _ in cases if inner == 1 and G == 1}
    assert {fam.pick_row_form(D * inner) for N, G, D, inner, _, _ in cases} == {fam.ROW_SHORT, fam.ROW_WAVE, fam.ROW_GROUP, fam.ROW_SPLIT}
    S = {fam.row_slices(fam.ROW_SPLIT, *c[:4]) for c in cases if fam.pick_row_form(c[2] * c[3]) == fam.ROW_SPLIT}
    assert 2 in S and 49 in S and fam.row_slices(fam.ROW_SPLIT, 1, 1, 200000, 1) == 49      # the largest S at 2 . 10^5 elements
    assert fam.row_slices(fam.ROW_WAVE, 5, 1, 100, 1) == 0 and fam.row_slices(fam.ROW_SPLIT, 5, 1, 100, 1) == 1
    PS = {(fam.pick_param_form(c[3]), fam.param_slices(fam.pick_param_form(c[3]), *c[:4]) > 1) for c in cases}
    assert PS == {(fam.PARAM_COLUMNS, False), (fam.PARAM_COLUMNS, True), (fam.PARAM_PLANES, False), (fam.PARAM_PLANES, True)}
    for C in (1, 2, 3, 6, 64):
        for g in fam._divisors(C):
            assert any(c[1] == g and c[1] * c[2] == C and c[3] >= 1 for c in fam.GROUP_CASES), (C, g)
    assert {1, 2, 3, 4, 5, 49, 64, 1025} <= {c[3] for c in fam.GROUP_CASES} and {1, 2, 5} <= {c[0] for c in fam.GROUP_CASES}
    assert all(N * G * D * inner <= 200000 for N, G, D, inner, _, _ in cases)


def test_the_shifted_sums_are_accurate_where_fp32_one_pass_is_not():
    """Why the definition is what it is: a row of mean 1e4, sigma 1e-3."""
    rng = np.random.default_rng(5)
    x = (1e4 + 1e-3 * rng.standard_normal((3, 1, 4096, 1))).astype(F32)
    f = fam.forward(x, eps=0.0)
    for r in range(3):
        x64 = x[r].astype(F64).reshape(-1)
        two_pass = ((x64 - x64.mean()) ** 2).mean()
        assert abs(f["wide"]["var64"][r] - two_pass) <= 1e-6 * two_pass
        xf = x[r].reshape(-1)
        m32, q32 = np.cumsum(xf, dtype=F32)[-1] / F32(xf.size), np.cumsum(xf * xf, dtype=F32)[-1] / F32(xf.size)      # fp32 chains
        assert abs(F64(q32 - m32 * m32) - two_pass) > 1.0 * two_pass
