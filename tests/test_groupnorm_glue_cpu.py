"""CPU-tier checks of the boundary of layer and group normalization (np_groupnorm.hip, ext/hip_dnn.c, host/numpower_dnn.cpp,
ndarray.py): the two calls are declared below the batch-normalization block, prototyped and exported; the probes return zeros before
any launch; every refusal comes back on a machine with no device, so nothing ran; each message of the glue is raised with its text;
the header's comment block states each rule; the dispatcher restated in tests/groupnorm_family.py reads the constants the library
reports."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import groupnorm_family as B

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_LN_MSG_NDIM": "dnn_layer_norm: normalized_shape must have between 1 and the input's number of dimensions",
    "NPH_LN_MSG_SHAPE": "dnn_layer_norm: normalized_shape must equal the input's trailing axes",
    "NPH_LN_MSG_EMPTY": "dnn_layer_norm: an operand has no elements",
    "NPH_LN_MSG_GAMMA": "dnn_layer_norm: gamma must have the normalized shape",
    "NPH_LN_MSG_BETA": "dnn_layer_norm: beta must have the normalized shape",
    "NPH_LN_MSG_SAVED": "dnn_layer_norm_backward: save_mean and save_invstd must have the shape of the input's leading axes",
    "NPH_LN_MSG_GRADIENT": "dnn_layer_norm_backward: the gradient must have the shape of the input",
    "NPH_LN_MSG_EPS": "dnn_layer_norm: eps must not be negative",
    "NPH_LN_MSG_DEVICE": "dnn_layer_norm: the operands must be on the same device",
    "NPH_LN_MSG_CPU": "dnn_layer_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
    "NPH_GN_MSG_NDIM": "dnn_group_norm: the input must have at least 2 dimensions (N, C, ...)",
    "NPH_GN_MSG_EMPTY": "dnn_group_norm: an operand has no elements",
    "NPH_GN_MSG_GROUPS": "dnn_group_norm: num_groups must be at least 1",
    "NPH_GN_MSG_DIVISIBLE": "dnn_group_norm: C = the input's shape[1] must be divisible by num_groups",
    "NPH_GN_MSG_GAMMA": "dnn_group_norm: gamma must be a (C) array, C = the input's shape[1]",
    "NPH_GN_MSG_BETA": "dnn_group_norm: beta must be a (C) array, C = the input's shape[1]",
    "NPH_GN_MSG_SAVED": "dnn_group_norm_backward: save_mean and save_invstd must be (N, num_groups) arrays",
    "NPH_GN_MSG_GRADIENT": "dnn_group_norm_backward: the gradient must have the shape of the input",
    "NPH_GN_MSG_EPS": "dnn_group_norm: eps must not be negative",
    "NPH_GN_MSG_DEVICE": "dnn_group_norm: the operands must be on the same device",
    "NPH_GN_MSG_CPU": "dnn_group_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
}
UNIT = ROOT / "numpower_amd" / "csrc" / "np_groupnorm.hip"


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_batchnorm_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert ("int np_groupnorm_forward(const float *x, const float *gamma , const float *beta , size_t N, size_t G, size_t D, size_t inner, "
            "double eps, float *y, float *save_mean , float *save_invstd );") in text
    assert ("int np_groupnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd, "
            "size_t N, size_t G, size_t D, size_t inner, float *dx, float *dgamma , float *dbeta );") in text
    order = [text.index(s) for s in ("int np_cross_entropy(", "int np_batchnorm_forward(", "int np_batchnorm_backward(", "int np_groupnorm_forward(",
                                     "int np_groupnorm_backward(", "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_groupnorm_last_path(int *row_form, int *param_form, int *launches, size_t *row_slices, size_t *param_slices);" in debug
    assert "int np_debug_groupnorm_force_form(int row_form, int param_form);" in debug and "int np_debug_groupnorm_bounds(size_t bounds[], int n);" in debug
    order = [debug.index(s) for s in ("int np_debug_batchnorm_bounds(", "int np_debug_groupnorm_last_path(", "int np_debug_groupnorm_force_form(",
                                      "int np_debug_groupnorm_bounds(", "#define NP_REDUCE_PATH_ROWS_BLOCK")]
    assert order == sorted(order)
    names = ("np_groupnorm_forward", "np_groupnorm_backward", "np_debug_groupnorm_last_path", "np_debug_groupnorm_force_form", "np_debug_groupnorm_bounds")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [11, 12, 5, 2, 2]
    assert _lib.PROTOTYPES["np_groupnorm_forward"][1][7] == C.c_double                      # eps is a double in the C ABI
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_groupnorm.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build
    assert "#pragma clang fp contract(off)" in UNIT.read_text()                             # every fp32 step is rounded on its own


def test_the_probes_are_zero_before_any_launch_and_report_the_constants():
    from numpower_amd import _lib
    lib = _lib.load()
    r, p, n, rs, ps = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_size_t(7), C.c_size_t(7)
    refs = [C.byref(v) for v in (r, p, n, rs, ps)]
    for k in range(5):
        assert lib.np_debug_groupnorm_last_path(*[None if j == k else v for j, v in enumerate(refs)]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_groupnorm_last_path(*refs) == _lib.NP_OK
    assert (r.value, p.value, n.value, rs.value, ps.value) == (0, 0, 0, 0, 0)
    for bad in (-2, 0, 5, 115):
        assert lib.np_debug_groupnorm_force_form(bad, -1) == NP_ERR_INVALID and b"row_form must be -1" in lib.np_last_error()
    for bad in (-2, 0, 3, 115):
        assert lib.np_debug_groupnorm_force_form(-1, bad) == NP_ERR_INVALID and b"param_form must be -1" in lib.np_last_error()
    bounds = (C.c_size_t * 7)()
    assert lib.np_debug_groupnorm_bounds(None, 7) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_groupnorm_bounds(bounds, 6) == NP_ERR_INVALID and b"room for 7" in lib.np_last_error()
    assert lib.np_debug_groupnorm_bounds(bounds, 7) == _lib.NP_OK
    assert tuple(bounds) == B.BOUNDS                                                         # the family's dispatcher uses the library's constants
    short, wave, small, group, target, most, steps = bounds
    assert 1 <= short <= 32 < wave == 64 * 16 < small == 256 * 16 < group == 1024 * 8 < 1 << 31 and most <= target and steps >= 1
    src = UNIT.read_text()
    for name, value in (("kShortMaxL", short), ("kWaveMaxL", wave), ("kGroupSmallL", small), ("kGroupMaxL", group), ("kTargetGroups", target),
                        ("kMaxSlices", most), ("kSliceMinSteps", steps)):
        assert "constexpr unsigned %s = %d;" % (name, value) in src
    a, b, c, d, e = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))      # far apart, never dereferenced
    try:                                       # forcing a form that cannot serve the shape is refused, with no device
        for row, param, shape in ((1, -1, (2, 1, short + 1, 1)), (1, -1, (2, 3, 3, short // 2)), (2, -1, (2, 1, wave + 1, 1)), (3, -1, (2, 2, 2, group // 2 + 1)),
                                  (-1, 1, (2, 1, 8, 2)), (2, 1, (4, 2, 3, 49))):
            assert lib.np_debug_groupnorm_force_form(row, param) == _lib.NP_OK
            assert lib.np_groupnorm_backward(a, b, None, c, d, *shape, e, None, None) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
            if row != -1 and (row, param) != (2, 1):
                assert lib.np_groupnorm_forward(a, None, None, *shape, 1e-5, b, c, d) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
    finally:
        assert lib.np_debug_groupnorm_force_form(-1, -1) == _lib.NP_OK
    assert lib.np_debug_groupnorm_last_path(*refs) == _lib.NP_OK and (r.value, p.value, n.value) == (0, 0, 0)      # no device, no launch


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("layer and group normalization (np_groupnorm.hip"):raw.index("int np_groupnorm_forward(")]
    for phrase in ("contiguous fp32 array seen as (N, G, D, inner)", "M = N.G rows of L = D.inner contiguous floats", "P = G.D affine parameters",
                   "element j of row r uses parameter (r mod G).D + j / inner", "Layer normalization over the trailing axes is G = 1, D = L, inner = 1",
                   "D = C / G, inner = the product of the spatial extents", "Instance normalization is G = C",
                   "batch normalization's definition applied per row", "carried in fp64", "a shift K = x[r, 0]", "accumulated in double from +0.0",
                   "mean64 = K + S1 / L", "var64 = S2 / L - (S1 / L)^2, the biased variance", "save_mean[r] = f32(mean64)",
                   "save_invstd[r] = f32(1 / sqrt(var64 + eps))", "ONE rounding of an fp64 value", "eps is a double",
                   "three separately rounded fp32 steps", "no contraction", "d = x - mean", "h = d . invstd",
                   "y = h . gamma[p] + beta[p], a multiply, then an add", "A NULL gamma means 1 and a NULL beta means 0, and their steps are skipped",
                   "xh = (x - mean) . invstd rounded as above", "g = f32(dy . gamma[p])", "a NULL gamma: g = dy",
                   "each product formed in double from the two floats", "mb = f32(sum g / L)", "mg = f32(sum g . xh / L)",
                   "dx = invstd . ((g - mb) - xh . mg)", "in exactly that association", "dbeta[p] = f32(sum dy)", "dgamma[p] = f32(sum dy . xh)",
                   "over every element that uses parameter p", "Either may be NULL", "with both NULL the reduction is not launched",
                   "a NaN or +-Inf comes out NaN in every element of y and dx", "no other row is touched", "with eps > 0, y = beta exactly",
                   "with eps = 0, invstd = +Inf and y = NaN", "The same holds for L = 1, which is accepted", "eps < 0 is refused", "dx may alias dy",
                   "No other output may overlap an input", "all size_t", "at 2^31 or more is refused with a message, never truncated",
                   "element offsets are size_t", "no float or double atomics", "pool scratch that is released on every path", "on the library stream",
                   "forms and slice counts come from (N, G, D, inner) alone", "bit-identical from run to run", "any 4-byte-aligned pointer is accepted",
                   "the same bits as a 16-byte-aligned one", "pointers are checked first, then the extents, the parameters, the aliasing, then work begins"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f, g = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5, 6, 7))      # far apart, never dereferenced
    ok = (3, 2, 4, 5)
    fwd = lambda x, y, m, i, shape=ok, eps=1e-5, ga=None, be=None: lib.np_groupnorm_forward(x, ga, be, *shape, eps, y, m, i)
    bwd = lambda x, dy, m, i, dx, shape=ok, ga=None, dg=None, db=None: lib.np_groupnorm_backward(x, dy, ga, m, i, *shape, dx, dg, db)
    for args in ((None, b, c, d), (a, None, c, d), (a, b, None, d), (a, b, c, None)):
        assert fwd(*args) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for args in ((None, b, c, d, e), (a, None, c, d, e), (a, b, None, d, e), (a, b, c, None, e), (a, b, c, d, None)):
        assert bwd(*args) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in range(4):
        bad = list(ok)
        bad[k] = 0
        assert fwd(a, b, c, d, bad) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
        assert bwd(a, b, c, d, e, bad) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    big = (1 << 31, (1 << 31) + 5, 1 << 40, 1 << 63)
    for v in big:      # M = N.G and P = G.D: refused, never truncated
        for shape in ((v, 1, 2, 1), (2, v, 1, 1), (1 << 16, v >> 16 if v < 1 << 63 else 1 << 20, 1, 1)):
            assert fwd(a, b, c, d, shape) == NP_ERR_INVALID and b"rows is 2^31 or more" in lib.np_last_error(), shape
        for shape in ((1, 1, v, 1), (1, 1 << 16, v >> 16 if v < 1 << 63 else 1 << 20, 1)):
            assert fwd(a, b, c, d, shape) == NP_ERR_INVALID and b"parameters is 2^31 or more" in lib.np_last_error(), shape
            assert bwd(a, b, c, d, e, shape) == NP_ERR_INVALID and b"parameters is 2^31 or more" in lib.np_last_error(), shape
    assert fwd(a, b, c, d, (1 << 30, 1, 1 << 30, 1 << 10)) == NP_ERR_INVALID and b"does not fit" in lib.np_last_error()
    for eps in (-1e-5, -0.0 - 1e-300, float("-inf"), float("nan")):
        assert fwd(a, b, c, d, eps=eps) == NP_ERR_INVALID and b"eps must not be negative" in lib.np_last_error()
    # aliasing: no output may overlap an input or another output; dx == dy alone is allowed (it runs on the GPU tier with real buffers).
    # Every call in this file is refused on its arguments: none may reach a device, the pointers are not allocations.
    near = lambda p, k=8: C.c_void_p(p.value + k)
    for args, kw in (((a, a, c, d), {}), ((a, near(a), c, d), {}), ((a, b, c, near(c, 4)), {}), ((a, b, near(a, 16), d), {}),
                     ((a, b, c, d), {"ga": near(b, 4)}), ((a, b, c, d), {"be": near(c, 4)})):
        assert fwd(*args, **kw) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    for args, kw in (((a, b, c, d, a), {}), ((a, b, c, d, near(b, 4)), {}), ((a, b, c, d, e), {"dg": near(b, 4)}), ((a, b, c, d, b), {"dg": near(b, 4)}),
                     ((a, b, c, d, e), {"dg": f, "db": near(f, 4)}), ((a, b, c, d, near(c, 4)), {}), ((a, b, c, d, e), {"ga": near(e, 4)})):
        assert bwd(*args, **kw) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()

    src = UNIT.read_text()
    body = _function(src, "int np_groupnorm_forward(")      # pointers, extents, parameters, aliasing, forms, then work
    assert body.index("null pointer") < body.index("check_extents(") < body.index("eps must not") < body.index("any_overlap(") \
        < body.index("pick_forms(") < body.index("ensure_init()") < body.index("launch_rows<")
    assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int np_groupnorm_backward(")
    assert body.index("null pointer") < body.index("check_extents(") < body.index("any_overlap(") < body.index("pick_forms(") \
        < body.index("ensure_init()") < body.index("launch_params(") < body.index("launch_rows<")      # the parameters first: dx may alias dy
    assert "<<<" not in body and "alloc" not in body and "if (params)" in body
    body = _function(src, "int check_extents(")
    assert body.index("at least 1") < body.index("rows is 2^31 or more") < body.index("parameters is 2^31 or more") < body.index("does not fit")
    assert "ensure_init" not in body and "hip" not in body
    body = _function(src, "int pick_forms(")    # the forms come from (D, inner) alone, and from the A-B switch
    assert "row_form = L <= kShortMaxL ? ROW_SHORT : L <= kWaveMaxL ? ROW_WAVE : L <= kGroupMaxL ? ROW_GROUP : ROW_SPLIT;" in body
    assert "param_form = inner == 1 ? PARAM_COLUMNS : PARAM_PLANES;" in body and "num_cus" not in body
    body = _function(src, "void plan_slices(")  # the slices from the extents alone: never from the CU count
    assert "num_cus" not in body and "stream_cap" not in body and "hip" not in body
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "num_cus" not in code and "__fdividef" not in code and "rcp" not in code and "fmaf" not in code
    assert "np::Scratch part, mbmg;" in _function(src, "int launch_rows(") and "np::Scratch ppart;" in _function(src, "int launch_params(")
    assert "hipMalloc" not in code


def test_the_family_restates_the_dispatcher():
    src = UNIT.read_text()
    plan = _function(src, "void plan_slices(")
    for line in ("size_t s = steps / kSliceMinSteps;", "if (s > kTargetGroups / blocks) s = kTargetGroups / blocks;", "if (s > kMaxSlices) s = kMaxSlices;",
                 "per = ceil_div(units, s);", "S = (unsigned)ceil_div(units, per);"):
        assert line in plan, line
    rows = _function(src, "int launch_rows(")
    for line in ("plan_slices(ceil_div(g.L, 4), 256, g.M, g.S, g.per);", "if (g.L <= 256) gn_wave_kernel<OP, 1>", "else if (g.L <= 512) gn_wave_kernel<OP, 2>",
                 "else gn_wave_kernel<OP, 4>", "if (g.L <= kGroupSmallL / 2) gn_group_kernel<OP, 4, 2>", "else if (g.L <= kGroupSmallL) gn_group_kernel<OP, 4, 4>",
                 "else gn_group_kernel<OP, 16, 2>"):
        assert line in rows, line
    params = _function(src, "int launch_params(")
    for line in ("while (g.CW < 64 && g.CW < g.P) g.CW *= 2;", "plan_slices(g.N, 256 / g.CW, ceil_div(g.P, g.CW), g.PS, g.pper);",
                 "plan_slices(ceil_div(g.n, 4), 256, g.P, g.PS, g.pper);"):
        assert line in params, line
    assert [B.pick_row_form(L) for L in (1, 32, 33, 1024, 1025, 8192, 8193)] == [1, 1, 2, 2, 3, 3, 4]
    assert B.pick_param_form(1) == B.PARAM_COLUMNS and B.pick_param_form(2) == B.PARAM_PLANES
    assert B.row_slices(B.ROW_SPLIT, 32, 1, 64, 56 * 56) == 49 and B.row_slices(B.ROW_SPLIT, 64, 1, 10 ** 6, 1) == 32
    assert B.param_slices(B.PARAM_COLUMNS, 65536, 1, 1024, 1) == 128 and B.param_slices(B.PARAM_PLANES, 64, 32, 2, 112 * 112) == 32
    assert B.launches(B.ROW_WAVE, B.PARAM_NONE) == 1 and B.launches(B.ROW_SPLIT, B.PARAM_NONE) == 3 and B.launches(B.ROW_SPLIT, B.PARAM_PLANES) == 5
    assert B.launches(B.ROW_SHORT, B.PARAM_COLUMNS) == 3
    assert B.row_depth(B.ROW_SPLIT, 1, 1, 7 * 1024, 1) == 28 + 6 + 3 + 1 + 6      # seven steps of four, the butterfly, the waves, the fold
    assert B.row_depth(B.ROW_SHORT, 5, 1, 17, 1) == 1 + 5 and B.row_depth(B.ROW_GROUP, 2, 1, 8192, 1) == 8 + 6 + 15


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    for text in ("NDArray **NDArrayDNN_LayerNorm_Forward(NDArray *x, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *beta, double eps);",
                 "NDArray **NDArrayDNN_LayerNorm_Backward(NDArray *x, NDArray *dy, const int *normalized_shape, int normalized_ndim, NDArray *gamma, "
                 "NDArray *save_mean, NDArray *save_invstd);",
                 "NDArray **NDArrayDNN_GroupNorm_Forward(NDArray *x, int num_groups, NDArray *gamma, NDArray *beta, double eps);",
                 "NDArray **NDArrayDNN_GroupNorm_Backward(NDArray *x, NDArray *dy, int num_groups, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd);"):
        assert text in host, text
    order = [host.index(s) for s in ("NDArrayDNN_BatchNorm_Backward(", "NDArrayDNN_LayerNorm_Forward(", "NDArrayDNN_GroupNorm_Backward(")]
    assert order == sorted(order)
    h = ndarray._load_host()
    names = ("LayerNorm_Forward", "LayerNorm_Backward", "GroupNorm_Forward", "GroupNorm_Backward")
    assert all(hasattr(h, "NDArrayDNN_" + n) for n in names)
    glue = _header("hip_dnn.h", "ext")
    for text in ("struct NDArray **NPH_LayerNorm_Forward(struct NDArray *x, const int *normalized_shape, int normalized_ndim, struct NDArray *gamma, "
                 "struct NDArray *beta, double eps);",
                 "struct NDArray **NPH_LayerNorm_Backward(struct NDArray *x, struct NDArray *dy, const int *normalized_shape, int normalized_ndim, "
                 "struct NDArray *gamma, struct NDArray *save_mean, struct NDArray *save_invstd);",
                 "struct NDArray **NPH_GroupNorm_Forward(struct NDArray *x, int num_groups, struct NDArray *gamma, struct NDArray *beta, double eps);",
                 "struct NDArray **NPH_GroupNorm_Backward(struct NDArray *x, struct NDArray *dy, int num_groups, struct NDArray *gamma, "
                 "struct NDArray *save_mean, struct NDArray *save_invstd);"):
        assert text in glue, text
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    shared = _function(src, "static int norm_operands(")
    order = [shared.index("msg->" + n) for n in ("empty", "gamma", "beta", "saved", "gradient", "eps", "device", "cpu")]
    assert order == sorted(order) and "NDArray_Empty" not in shared and "np_groupnorm" not in shared
    layer = _function(src, "static int layernorm_of(")
    assert layer.index("NPH_LN_MSG_NDIM") < layer.index("NPH_LN_MSG_SHAPE") < layer.index("norm_operands(") and "NDArray_Empty" not in layer
    group = _function(src, "static int groupnorm_of(")
    assert group.index("NPH_GN_MSG_NDIM") < group.index("NPH_GN_MSG_EMPTY") < group.index("NPH_GN_MSG_GROUPS") < group.index("NPH_GN_MSG_DIVISIBLE") \
        < group.index("norm_operands(") and "NDArray_Empty" not in group
    fwd = _function(src, "static NDArray **norm_forward(")
    assert fwd.index("empty_like_on_gpu(") < fwd.index("np_groupnorm_forward(") < fwd.index("batchnorm_drop(rtns, y, mean, invstd);\n    }")
    bwd = _function(src, "static NDArray **norm_backward(")
    assert bwd.index("empty_like_on_gpu(") < bwd.index("np_groupnorm_backward(") and bwd.count("batchnorm_drop(") == 2
    for name, check, work in (("LayerNorm_Forward", "layernorm_of(", "norm_forward("), ("LayerNorm_Backward", "layernorm_of(", "norm_backward("),
                              ("GroupNorm_Forward", "groupnorm_of(", "norm_forward("), ("GroupNorm_Backward", "groupnorm_of(", "norm_backward(")):
        body = _function(src, "NDArray **NPH_" + name + "(")
        assert body.index(check) < body.index(work), name
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for n in names:
        body = _function(cpp, "NDArray **NDArrayDNN_" + n + "(")
        assert "on_contiguous(" in body and "NPH_" + n + "(" in body
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "LayerNorm" not in tool and "GroupNorm" not in tool and "groupnorm" not in tool      # the reference has no normalization layer: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message before them needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x = ones(2, 6, 4)
    lf, lb, gf, gb = NDArray.dnn_layer_norm_forward, NDArray.dnn_layer_norm_backward, NDArray.dnn_group_norm_forward, NDArray.dnn_group_norm_backward

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    L, G = (lambda n: MESSAGES["NPH_LN_MSG_" + n]), (lambda n: MESSAGES["NPH_GN_MSG_" + n])
    # layer normalization
    for shape in ((), (2, 6, 4, 1), (1, 2, 6, 4)):
        assert message(lf, x, shape) == L("NDIM") and message(lb, x, x, shape, None, ones(2), ones(2)) == L("NDIM")
    for shape in (5, (4, 6), (6,), (2, 6), (3, 4), (1, 6, 4)):
        assert message(lf, x, shape) == L("SHAPE") and message(lb, x, x, shape, None, ones(2), ones(2)) == L("SHAPE")
    for shape, norm in (((0, 4), 4), ((2, 0), 0), ((2, 0, 4), 4), ((2, 0, 4), (0, 4))):      # an empty input, before anything is said about gamma
        e = ones(*shape)
        assert message(lf, e, norm, ones(7)) == L("EMPTY") and message(lb, e, e, norm, ones(7), ones(2), ones(2)) == L("EMPTY")
    for bad in (ones(5), ones(4, 1), ones(1, 4), ones(6, 4)):
        assert message(lf, x, 4, bad) == L("GAMMA") and message(lf, x, 4, ones(4), bad) == L("BETA") and message(lf, x, 4, None, bad) == L("BETA")
        assert message(lb, x, x, 4, bad, ones(2, 6), ones(2, 6)) == L("GAMMA")
    assert message(lf, x, (6, 4), ones(4)) == L("GAMMA") and message(lf, x, (6, 4), ones(6, 4), ones(24)) == L("BETA")
    for bad in (ones(2), ones(6), ones(2, 6, 1), ones(12), ones(6, 2)):
        assert message(lb, x, x, 4, None, bad, ones(2, 6)) == L("SAVED") and message(lb, x, x, 4, ones(4), ones(2, 6), bad) == L("SAVED")
    assert message(lb, x, x, (2, 6, 4), None, ones(2), ones(1)) == L("SAVED")              # the whole array: statistics of shape (1)
    for dy in (ones(2, 6), ones(2, 6, 5), ones(6, 2, 4), ones(48), ones(2, 6, 2, 2)):
        assert message(lb, x, dy, 4, None, ones(2, 6), ones(2, 6)) == L("GRADIENT")
    for eps in (-1e-5, -1, float("nan")):
        assert message(lf, x, 4, eps=eps) == L("EPS")
    for norm, stat in ((4, (2, 6)), ((6, 4), (2,)), ((2, 6, 4), (1,))):                     # the right operands get as far as the device check
        assert message(lf, x, norm) == L("CPU") and message(lf, x, norm, ones(*(norm if isinstance(norm, tuple) else (norm,)))) == L("CPU")
        assert message(lb, x, x, norm, None, ones(*stat), ones(*stat)) == L("CPU")
    assert message(lf, ones(3, 1), 1) == L("CPU")                                           # L = 1 is accepted
    assert message(lf, x, 4, eps="small") == "dnn_layer_norm_forward: eps must be a number"
    assert message(lf, x, 4.0) == "dnn_layer_norm_forward: normalized_shape must be an int or a tuple of ints"
    assert message(lb, x, x, (4, True), None, ones(2, 6), ones(2, 6)) == "dnn_layer_norm_backward: normalized_shape must be an int or a tuple of ints"
    assert message(lf, None, 4) == "dnn_layer_norm_forward: x must be an array"
    assert message(lb, x, x, 4, None, None, ones(2, 6)) == "dnn_layer_norm_backward: x, dy, save_mean and save_invstd must be arrays"
    # group normalization
    for bad in (ones(6), ones(1)):
        assert message(gf, bad, 1) == G("NDIM") and message(gb, bad, bad, 1, None, ones(1, 1), ones(1, 1)) == G("NDIM")
    for shape in ((0, 6, 4), (2, 0, 4), (2, 6, 0), (0, 6), (2, 6, 4, 0)):                   # an empty input, before anything is said about the groups
        e = ones(*shape)
        assert message(gf, e, 0, ones(7)) == G("EMPTY") and message(gb, e, e, 4, ones(7), ones(2, 4), ones(2, 4)) == G("EMPTY")
    for groups in (0, -1, -6):
        assert message(gf, x, groups, ones(7)) == G("GROUPS") and message(gb, x, x, groups, None, ones(2, 1), ones(2, 1)) == G("GROUPS")
    for groups in (4, 5, 7, 12):
        assert message(gf, x, groups, ones(7)) == G("DIVISIBLE") and message(gb, x, x, groups, None, ones(2, groups), ones(2, groups)) == G("DIVISIBLE")
    for bad in (ones(7), ones(6, 1), ones(1, 6), ones(3), ones(2)):
        assert message(gf, x, 3, bad) == G("GAMMA") and message(gf, x, 3, ones(6), bad) == G("BETA") and message(gf, x, 3, None, bad) == G("BETA")
        assert message(gb, x, x, 3, bad, ones(2, 3), ones(2, 3)) == G("GAMMA")
    for bad in (ones(6), ones(2, 6), ones(3, 2), ones(2, 3, 1), ones(2)):
        assert message(gb, x, x, 3, None, bad, ones(2, 3)) == G("SAVED") and message(gb, x, x, 3, ones(6), ones(2, 3), bad) == G("SAVED")
    for dy in (ones(2, 6), ones(2, 6, 5), ones(6, 2, 4), ones(48), ones(2, 6, 2, 2)):
        assert message(gb, x, dy, 3, None, ones(2, 3), ones(2, 3)) == G("GRADIENT")
    for eps in (-1e-5, -1, float("nan")):
        assert message(gf, x, 3, eps=eps) == G("EPS")
    for shape in ((2, 6), (2, 6, 4), (2, 6, 1, 2, 2)):                                       # the right operands get as far as the device check
        xs = ones(*shape)
        for groups in (1, 2, 3, 6):
            assert message(gf, xs, groups) == G("CPU") and message(gf, xs, groups, ones(6), ones(6)) == G("CPU")
            assert message(gb, xs, xs, groups, ones(6), ones(2, groups), ones(2, groups)) == G("CPU")
    assert message(gf, x, 3, eps="small") == "dnn_group_norm_forward: eps must be a number"
    assert message(gf, x, 3.0) == "dnn_group_norm_forward: num_groups must be an int" and message(gf, x, True) == "dnn_group_norm_forward: num_groups must be an int"
    assert message(gb, x, x, "3", None, ones(2, 3), ones(2, 3)) == "dnn_group_norm_backward: num_groups must be an int"
    assert message(gf, None, 3) == "dnn_group_norm_forward: x must be an array"
    assert message(gb, x, x, 3, None, None, ones(2, 3)) == "dnn_group_norm_backward: x, dy, save_mean and save_invstd must be arrays"
    assert "Instance normalization is num_groups = C" in " ".join(gf.__doc__.split())
