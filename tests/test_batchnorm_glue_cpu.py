"""CPU-tier checks of the boundary of batch normalization (np_batchnorm.hip, ext/hip_dnn.c, host/numpower_dnn.cpp, ndarray.py): the
two calls are declared below the softmax block, prototyped and exported; the probes return zeros before any launch; every refusal
comes back on a machine with no device, so nothing ran; each message of the glue is raised with its text; the header's comment
block states each rule; the dispatcher restated in tests/batchnorm_family.py reads the constants the library reports."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import batchnorm_family as B

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_BN_MSG_NDIM": "dnn_batch_norm: the input must have at least 2 dimensions (N, C, ...)",
    "NPH_BN_MSG_EMPTY": "dnn_batch_norm: an operand has no elements",
    "NPH_BN_MSG_GAMMA": "dnn_batch_norm: gamma must be a (C) array, C = the input's shape[1]",
    "NPH_BN_MSG_BETA": "dnn_batch_norm: beta must be a (C) array, C = the input's shape[1]",
    "NPH_BN_MSG_RUNNING": "dnn_batch_norm: running_mean and running_var must be (C) arrays, C = the input's shape[1]",
    "NPH_BN_MSG_INFERENCE": "dnn_batch_norm: inference needs both running_mean and running_var",
    "NPH_BN_MSG_SAVED": "dnn_batch_norm_backward: save_mean and save_invstd must be (C) arrays, C = the input's shape[1]",
    "NPH_BN_MSG_GRADIENT": "dnn_batch_norm_backward: the gradient must have the shape of the input",
    "NPH_BN_MSG_EPS": "dnn_batch_norm: eps must not be negative",
    "NPH_BN_MSG_MOMENTUM": "dnn_batch_norm: momentum must lie in [0, 1]",
    "NPH_BN_MSG_DEVICE": "dnn_batch_norm: the operands must be on the same device",
    "NPH_BN_MSG_CPU": "dnn_batch_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
    "NPH_BN_MSG_ONE_VALUE": "dnn_batch_norm: training needs more than one value per channel",
    "NPH_BN_MSG_RUNNING_VIEW": "dnn_batch_norm: the running statistics are updated in place and must be contiguous arrays",
}


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_softmax_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert ("int np_batchnorm_forward(const float *x, const float *gamma, const float *beta, size_t N, size_t C, size_t inner, int training, "
            "double momentum, double eps, float *running_mean, float *running_var, float *y, float *save_mean, float *save_invstd);") in text
    assert ("int np_batchnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd, "
            "size_t N, size_t C, size_t inner, float *dx, float *dgamma , float *dbeta );") in text
    order = [text.index(s) for s in ("int np_cross_entropy(", "int np_batchnorm_forward(", "int np_batchnorm_backward(", "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_batchnorm_last_path(int *form, int *launches, size_t *slices);" in debug
    assert "int np_debug_batchnorm_force_form(int form);" in debug and "int np_debug_batchnorm_bounds(size_t bounds[], int n);" in debug
    order = [debug.index(s) for s in ("int np_debug_softmax_bounds(", "int np_debug_batchnorm_last_path(", "int np_debug_batchnorm_force_form(",
                                      "int np_debug_batchnorm_bounds(")]
    assert order == sorted(order)
    names = ("np_batchnorm_forward", "np_batchnorm_backward", "np_debug_batchnorm_last_path", "np_debug_batchnorm_force_form", "np_debug_batchnorm_bounds")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [14, 11, 3, 1, 2]
    assert _lib.PROTOTYPES["np_batchnorm_forward"][1][7:9] == [C.c_double, C.c_double]      # momentum and eps are doubles in the C ABI
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_batchnorm.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build
    src = (ROOT / "numpower_amd" / "csrc" / "np_batchnorm.hip").read_text()
    assert "#pragma clang fp contract(off)" in src                                          # every fp32 step is rounded on its own


def test_the_probes_are_zero_before_any_launch_and_report_the_constants():
    from numpower_amd import _lib
    lib = _lib.load()
    form, launches, slices = C.c_int(-7), C.c_int(-7), C.c_size_t(7)
    assert lib.np_debug_batchnorm_last_path(None, C.byref(launches), C.byref(slices)) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_batchnorm_last_path(C.byref(form), C.byref(launches), C.byref(slices)) == _lib.NP_OK
    assert (form.value, launches.value, slices.value) == (0, 0, 0)
    for bad in (-2, 0, 4, 115):
        assert lib.np_debug_batchnorm_force_form(bad) == NP_ERR_INVALID and b"form must be -1" in lib.np_last_error()
    bounds = (C.c_size_t * 5)()
    assert lib.np_debug_batchnorm_bounds(None, 5) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_batchnorm_bounds(bounds, 4) == NP_ERR_INVALID and b"room for 5" in lib.np_last_error()
    assert lib.np_debug_batchnorm_bounds(bounds, 5) == _lib.NP_OK
    assert tuple(bounds) == B.BOUNDS                                                         # the family's dispatcher uses the library's constants
    one_small, one_max, target, most, steps = bounds
    assert 1 <= one_small < one_max < 1 << 31 and one_small == 256 * 16 and one_max % 1024 == 0 and most <= target and steps >= 1
    src = (ROOT / "numpower_amd" / "csrc" / "np_batchnorm.hip").read_text()
    for name, value in (("kOneSmallN", one_small), ("kOneMaxN", one_max), ("kTargetGroups", target), ("kMaxSlices", most), ("kSliceMinSteps", steps)):
        assert "constexpr unsigned %s = %d;" % (name, value) in src
    a, b, c, d, e = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))      # far apart, never dereferenced
    try:                                       # forcing a form that cannot serve the shape is refused, with no device
        for form_, shape in ((1, (2, 3, one_max // 2 + 1)), (1, (one_max + 1, 3, 1)), (3, (4, 8, 2)), (3, (1, 8, 1 << 12))):
            assert lib.np_debug_batchnorm_force_form(form_) == _lib.NP_OK
            assert lib.np_batchnorm_forward(a, None, None, *shape, 1, 0.1, 1e-5, None, None, b, c, d) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
            assert lib.np_batchnorm_backward(a, b, None, c, d, *shape, e, None, None) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
    finally:
        assert lib.np_debug_batchnorm_force_form(-1) == _lib.NP_OK
    assert lib.np_debug_batchnorm_last_path(C.byref(form), C.byref(launches), C.byref(slices)) == _lib.NP_OK and form.value == 0      # no device, no launch


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("batch normalization (np_batchnorm.hip"):raw.index("int np_batchnorm_forward(")]
    for phrase in ("contiguous fp32 array seen as (N, C, inner)", "inner == 1 is the (N, C) output of a dense layer", "inner = H.W is NCHW",
                   "per channel c over the n = N.inner values", "carried in fp64", "a shift K = x[0, c, 0]", "accumulated in double",
                   "exact in double except for exponent gaps beyond 29", "mean64 = K + S1 / n", "var64 = S2 / n - (S1 / n)^2, the biased variance",
                   "save_mean = f32(mean64)", "save_invstd = f32(1 / sqrt(var64 + eps))", "ONE rounding of an fp64 value", "eps and momentum are doubles",
                   "identical in training and inference", "three separately rounded fp32 steps", "no contraction", "d = x - mean", "h = d . invstd",
                   "y = h . gamma[c] + beta[c], a multiply, then an add", "A NULL gamma means 1 and a NULL beta means 0, and their steps are skipped",
                   "mean = running_mean", "invstd = f32(1 / sqrt((double) running_var + eps))", "gives training's y bit for bit",
                   "NULL pointers skip them", "updated in place", "r = f32((1 - momentum) . (double) r + momentum . s64)",
                   "s64 = var64 . n / (n - 1), the unbiased variance", "training with one value per channel is refused with a message",
                   "inference with n == 1 is fine", "from x, dy, gamma, save_mean, save_invstd", "xh = (x - mean) . invstd rounded as above",
                   "each product formed in double from the two floats", "dbeta = f32(sum dy)", "dgamma = f32(sum dy . xh)", "mb = f32(sum dy / n)",
                   "mg = f32(sum dy . xh / n)", "dx = (gamma . invstd) . ((dy - mb) - xh . mg)", "in exactly that association",
                   "dgamma and dbeta may be NULL", "a NaN or +-Inf comes out NaN in every element of y and dx", "no other channel is touched",
                   "with eps > 0, y = beta exactly", "with eps = 0, invstd = +Inf and y = NaN", "eps < 0 is refused", "dx may alias dy",
                   "No other output may overlap an input", "all size_t", "C >= 2^31 is refused with a message, never truncated",
                   "N.C.inner beyond 2^31 elements works", "no float or double atomics", "pool scratch that is released on every path",
                   "bit-identical from run to run", "any 4-byte-aligned pointer is accepted", "the same bits as a 16-byte-aligned one",
                   "pointers are checked first, then the extents, the parameters, the aliasing, then work begins"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    a, b, c, d, e, f, g = (C.c_void_p(k << 24) for k in (1, 2, 3, 4, 5, 6, 7))      # far apart, never dereferenced
    fwd, bwd = lib.np_batchnorm_forward, lib.np_batchnorm_backward
    ok = (3, 9, 2)
    train = lambda x, y, m, i, shape=ok, mom=0.1, eps=1e-5, rm=None, rv=None, ga=None, be=None: fwd(x, ga, be, *shape, 1, mom, eps, rm, rv, y, m, i)
    infer = lambda x, y, rm, rv, shape=ok, eps=1e-5: fwd(x, None, None, *shape, 0, 0.1, eps, rm, rv, y, None, None)
    for args in ((None, b, c, d), (a, None, c, d), (a, b, None, d), (a, b, c, None)):
        assert train(*args) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for args in ((None, b, c, d), (a, None, c, d), (a, b, None, d), (a, b, c, None)):      # inference needs both running statistics
        assert infer(*args) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for args in ((None, b, c, d, e), (a, None, c, d, e), (a, b, None, d, e), (a, b, c, None, e), (a, b, c, d, None)):
        x_, dy_, m_, i_, dx_ = args
        assert bwd(x_, dy_, None, m_, i_, *ok, dx_, None, None) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in range(3):
        bad = list(ok)
        bad[k] = 0
        assert train(a, b, c, d, bad) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
        assert bwd(a, b, None, c, d, *bad, e, None, None) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    for chans in (1 << 31, (1 << 31) + 5, 1 << 40, 1 << 63):      # refused, never truncated
        assert train(a, b, c, d, (2, chans, 1)) == NP_ERR_INVALID and b"2^31 or more" in lib.np_last_error()
        assert bwd(a, b, None, c, d, 2, chans, 1, e, None, None) == NP_ERR_INVALID and b"2^31 or more" in lib.np_last_error()
    assert train(a, b, c, d, (1 << 40, 1 << 20, 1 << 10)) == NP_ERR_INVALID and b"does not fit" in lib.np_last_error()
    for eps in (-1e-5, -0.0 - 1e-300, float("-inf"), float("nan")):
        assert train(a, b, c, d, eps=eps) == NP_ERR_INVALID and b"eps must not be negative" in lib.np_last_error()
        assert infer(a, b, c, d, eps=eps) == NP_ERR_INVALID and b"eps must not be negative" in lib.np_last_error()
    for mom in (-0.1, 1.0001, float("nan"), float("inf")):
        assert train(a, b, c, d, mom=mom) == NP_ERR_INVALID and b"momentum must lie in [0, 1]" in lib.np_last_error()
    for shape in ((1, 4, 1), (1, 1, 1)):                              # n == 1: refused in training (inference at n == 1 runs on the GPU tier)
        assert train(a, b, c, d, shape) == NP_ERR_INVALID and b"more than one value per channel" in lib.np_last_error()
    # aliasing: no output may overlap an input or another output; dx == dy alone is allowed (it runs on the GPU tier with real buffers).
    # Every call in this file is refused on its arguments: none may reach a device, the pointers are not allocations.
    near = lambda p, k=8: C.c_void_p(p.value + k)
    assert train(a, a, c, d) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert train(a, near(a), c, d) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert train(a, b, c, near(c, 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()          # save_invstd inside save_mean
    assert train(a, b, c, d, rm=near(a, 16), rv=e) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()      # a running statistic inside x
    assert train(a, b, c, d, rm=e, rv=near(e, 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert train(a, b, c, d, ga=near(b, 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()             # gamma inside y
    assert infer(a, a, c, d) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert infer(a, b, near(b, 4), d) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert bwd(a, b, None, c, d, *ok, a, None, None) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert bwd(a, b, None, c, d, *ok, near(b, 4), None, None) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert bwd(a, b, None, c, d, *ok, e, near(b, 4), None) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()      # dgamma inside dy
    assert bwd(a, b, None, c, d, *ok, b, near(b, 4), None) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()      # also when dx == dy
    assert bwd(a, b, None, c, d, *ok, e, f, near(f, 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()

    src = (ROOT / "numpower_amd" / "csrc" / "np_batchnorm.hip").read_text()
    body = _function(src, "int np_batchnorm_forward(")      # pointers, extents, parameters, aliasing, form, then work
    assert body.index("null pointer") < body.index("check_extents(") < body.index("eps must not") < body.index("momentum must") \
        < body.index("more than one value") < body.index("any_overlap(") < body.index("pick_form(") < body.index("ensure_init()") < body.index("launch<")
    assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int np_batchnorm_backward(")
    assert body.index("null pointer") < body.index("check_extents(") < body.index("any_overlap(") < body.index("pick_form(") \
        < body.index("ensure_init()") < body.index("launch<")
    assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int check_extents(")
    assert body.index("at least 1") < body.index("2^31 or more") < body.index("does not fit")
    assert "ensure_init" not in body and "hip" not in body
    body = _function(src, "int pick_form(")    # the form comes from (N, inner) alone, and from the A-B switch
    assert "form = inner == 1 ? FORM_ROWS : n <= kOneMaxN ? FORM_ONE : FORM_SPLIT;" in body and "num_cus" not in body
    body = _function(src, "void plan_of(")     # the slices from the extents alone: never from the CU count
    assert "num_cus" not in body and "stream_cap" not in body and "hip" not in body
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "num_cus" not in code and "__fdividef" not in code and "rcp" not in code and "fmaf" not in code
    launch = _function(src, "int launch(")     # partials in pool scratch, released on every path
    assert "np::Scratch part, mbmg;" in launch and "hipMalloc" not in code


def test_the_family_restates_the_dispatcher():
    src = (ROOT / "numpower_amd" / "csrc" / "np_batchnorm.hip").read_text()
    plan = _function(src, "void plan_of(")
    for line in ("while (g.CW < 64 && g.CW < g.C) g.CW *= 2;", "units = g.N, per_step = 256 / g.CW, blocks = ceil_div(g.C, g.CW);",
                 "units = ceil_div(g.n, 4), per_step = 256, blocks = g.C;", "size_t S = steps / kSliceMinSteps;",
                 "if (S > kTargetGroups / blocks) S = kTargetGroups / blocks;", "if (S > kMaxSlices) S = kMaxSlices;",
                 "g.per = ceil_div(units, S);", "g.S = (unsigned)ceil_div(units, g.per);"):
        assert line in plan, line
    assert B.pick_form(64, 3, 1) == B.FORM_ROWS and B.pick_form(2, 3, 4096) == B.FORM_ONE and B.pick_form(3, 2, 2731) == B.FORM_SPLIT
    assert B.slices(B.FORM_SPLIT, 64, 3, 224 * 224) == 682 and B.slices(B.FORM_SPLIT, 64, 64, 112 * 112) == 32
    assert B.slices(B.FORM_ROWS, 65536, 1024, 1) == 128 and B.slices(B.FORM_ROWS, 10 ** 6, 16, 1) == 1024
    assert B.launches(B.FORM_ONE) == 1 and B.launches(B.FORM_APPLY) == 1 and B.launches(B.FORM_SPLIT) == 3


def test_the_guards_depth_covers_every_kernel_order_at_the_tests_shapes():
    """batchnorm_family.DEPTH is argued from the kernels' structure; this pins the argument to the library's constants: the deepest
    summation tree of every form that can serve a shape of the GPU file, computed from np_debug_batchnorm_bounds, is within DEPTH."""
    from numpower_amd import _lib
    from tests.test_gpu_batchnorm import EXACT
    lib = _lib.load()
    bounds = (C.c_size_t * 5)()
    assert lib.np_debug_batchnorm_bounds(bounds, 5) == _lib.NP_OK
    bounds = tuple(bounds)
    src = (ROOT / "numpower_amd" / "csrc" / "np_batchnorm.hip").read_text()
    assert "constexpr unsigned kOneVals = %d;" % (bounds[0] // 256) in src and "NV = WAVES == 4 ? kOneVals : kOneMaxN / 1024" in src
    shapes = [c[:3] for c in B.GAUSSIAN_CASES + sum(B.OTHER_CASES.values(), ())] + [sh for _, sh, _ in EXACT]
    shapes += [(N, 1, inner) for N, _, inner in shapes]                              # the channel-alone identities
    worst = 0
    for N, C_, inner in shapes:
        assert N * C_ * inner <= 200000 + 70000, (N, C_, inner)
        for form in (B.FORM_ONE, B.FORM_SPLIT, B.FORM_ROWS):
            if B.serves(form, N, C_, inner, bounds):
                worst = max(worst, B.kernel_depth(form, N, C_, inner, bounds))
    assert 16 <= worst <= B.DEPTH, worst
    assert B.kernel_depth(B.FORM_SPLIT, 1, 1, 7 * 1024, bounds) == 28 + 6 + 3 + 1 + 6      # seven steps of four, the butterfly, the waves, the fold


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert ("NDArray **NDArrayDNN_BatchNorm_Forward(NDArray *x, NDArray *gamma, NDArray *beta, NDArray *running_mean, NDArray *running_var, int training, "
            "double momentum, double eps);") in host
    assert "NDArray **NDArrayDNN_BatchNorm_Backward(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd);" in host
    h = ndarray._load_host()
    assert all(hasattr(h, n) for n in ("NDArrayDNN_BatchNorm_Forward", "NDArrayDNN_BatchNorm_Backward"))
    glue = _header("hip_dnn.h", "ext")
    assert ("struct NDArray **NPH_BatchNorm_Forward(struct NDArray *x, struct NDArray *gamma, struct NDArray *beta, struct NDArray *running_mean, "
            "struct NDArray *running_var, int training, double momentum, double eps);") in glue
    assert ("struct NDArray **NPH_BatchNorm_Backward(struct NDArray *x, struct NDArray *dy, struct NDArray *gamma, struct NDArray *save_mean, "
            "struct NDArray *save_invstd);") in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = _function(src, "static int batchnorm_of(")
    order = [checks.index("NPH_BN_MSG_" + n) for n in ("NDIM", "EMPTY", "GAMMA", "BETA", "SAVED", "INFERENCE", "GRADIENT", "EPS", "MOMENTUM", "DEVICE", "CPU", "ONE_VALUE")]
    assert order == sorted(order) and "NDArray_Empty" not in checks and "np_batchnorm" not in checks
    fwd = _function(src, "NDArray **NPH_BatchNorm_Forward(")
    assert fwd.index("batchnorm_of(") < fwd.index("empty_like_on_gpu(") < fwd.index("np_batchnorm_forward(") < fwd.index("batchnorm_drop(rtns, y, mean, invstd);\n    }")
    bwd = _function(src, "NDArray **NPH_BatchNorm_Backward(")
    assert bwd.index("batchnorm_of(") < bwd.index("empty_like_on_gpu(") < bwd.index("np_batchnorm_backward(") and bwd.count("batchnorm_drop(") == 2
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for name, call in (("NDArrayDNN_BatchNorm_Forward(", "NPH_BatchNorm_Forward("), ("NDArrayDNN_BatchNorm_Backward(", "NPH_BatchNorm_Backward(")):
        body = _function(cpp, "NDArray **" + name)
        assert "on_contiguous(" in body and call in body
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "BatchNorm" not in tool and "batchnorm" not in tool      # the reference has no normalization layer: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last but one, so every message before them needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x = ones(2, 3, 4)
    fwd, bwd = NDArray.dnn_batch_norm_forward, NDArray.dnn_batch_norm_backward

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    M = lambda n: MESSAGES["NPH_BN_MSG_" + n]
    for bad in (ones(6), ones(1)):
        assert message(fwd, bad) == M("NDIM") and message(bwd, bad, bad, None, ones(3), ones(3)) == M("NDIM")
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (0, 3), (2, 3, 4, 0)):                  # an empty input, before anything is said about gamma
        e = ones(*shape)
        assert message(fwd, e, ones(7)) == M("EMPTY") and message(bwd, e, e, ones(7), ones(3), ones(3)) == M("EMPTY")
    for bad in (ones(4), ones(3, 1), ones(1, 3), ones(2)):
        assert message(fwd, x, bad) == M("GAMMA") and message(fwd, x, ones(3), bad) == M("BETA") and message(fwd, x, None, bad) == M("BETA")
        assert message(fwd, x, None, None, bad, ones(3)) == M("RUNNING") and message(fwd, x, None, None, ones(3), bad) == M("RUNNING")
        assert message(fwd, x, None, None, None, bad) == M("RUNNING")
        assert message(bwd, x, x, bad, ones(3), ones(3)) == M("GAMMA")
        assert message(bwd, x, x, None, bad, ones(3)) == M("SAVED") and message(bwd, x, x, ones(3), ones(3), bad) == M("SAVED")
    for rm, rv in ((None, None), (ones(3), None), (None, ones(3))):
        assert message(fwd, x, None, None, rm, rv, False) == M("INFERENCE")
    for dy in (ones(2, 3), ones(2, 3, 5), ones(3, 2, 4), ones(24), ones(2, 3, 2, 2)):
        assert message(bwd, x, dy, None, ones(3), ones(3)) == M("GRADIENT")
    for eps in (-1e-5, -1, float("nan")):
        assert message(fwd, x, eps=eps) == M("EPS") and message(fwd, x, None, None, ones(3), ones(3), False, 0.1, eps) == M("EPS")
    for momentum in (-0.5, 1.5, float("nan")):
        assert message(fwd, x, momentum=momentum) == M("MOMENTUM")
    assert message(fwd, x, momentum=7, eps=-1.0) == M("EPS")                              # eps before momentum
    for shape in ((2, 3), (2, 3, 4), (2, 3, 1, 2, 2)):                                     # the right operands get as far as the device check
        xs = ones(*shape)
        assert message(fwd, xs) == M("CPU") and message(fwd, xs, ones(3), ones(3), ones(3), ones(3)) == M("CPU")
        assert message(fwd, xs, None, None, ones(3), ones(3), False) == M("CPU")
        assert message(bwd, xs, xs, ones(3), ones(3), ones(3)) == M("CPU") and message(bwd, xs, xs, None, ones(3), ones(3)) == M("CPU")
    assert message(fwd, ones(1, 3)) == M("CPU")                                           # n == 1 is looked at after the devices
    assert message(fwd, x, eps="small") == "dnn_batch_norm_forward: momentum and eps must be numbers"
    assert message(fwd, x, momentum=True) == "dnn_batch_norm_forward: momentum and eps must be numbers"
    assert message(fwd, None) == "dnn_batch_norm_forward: x must be an array"
    assert message(bwd, x, x, None, None, ones(3)) == "dnn_batch_norm_backward: x, dy, save_mean and save_invstd must be arrays"
