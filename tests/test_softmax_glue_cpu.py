"""CPU-tier checks of the boundary of softmax, log-softmax and cross-entropy (np_softmax.hip, ext/hip_dnn.c, host/numpower_dnn.cpp,
ndarray.py): the enums and the three calls are declared below the pooling block, prototyped and exported; the probes return zeros
before any launch; every refusal comes back on a machine with no device, so nothing ran; each message of the glue is raised with its
text; the header's comment block states each rule."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_SOFTMAX_MSG_MODE": "softmax: unknown mode: 's' (softmax), 'l' (log-softmax)",
    "NPH_SOFTMAX_MSG_AXIS": "softmax: the axis is out of range for the operand's dimensions",
    "NPH_SOFTMAX_MSG_GRADIENT": "softmax_backward: the gradient must have the shape of the output",
    "NPH_XENT_MSG_LOGITS": "dnn_cross_entropy: the logits must be 2-dimensional (rows, classes)",
    "NPH_XENT_MSG_TARGET": "dnn_cross_entropy: the target must be (rows) class indices or (rows, classes) probabilities",
    "NPH_XENT_MSG_REDUCTION": "dnn_cross_entropy: unknown reduction: 'n' (none), 's' (sum), 'm' (mean)",
    "NPH_SOFTMAX_MSG_DEVICE": "softmax: the operands must be on the same device",
    "NPH_SOFTMAX_MSG_CPU": "softmax: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
    "NPH_XENT_MSG_DEVICE": "dnn_cross_entropy: the operands must be on the same device",
    "NPH_XENT_MSG_CPU": "dnn_cross_entropy: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
}


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_pooling_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert "typedef enum np_softmax_mode { NP_SOFTMAX = 0, NP_LOG_SOFTMAX = 1 } np_softmax_mode;" in text
    assert "typedef enum np_xent_target { NP_XENT_INDEX = 0, NP_XENT_PROB = 1 } np_xent_target;" in text
    assert "int np_softmax_forward(const float *x, size_t outer, size_t cols, size_t inner, int mode, float *y);" in text
    assert "int np_softmax_backward(const float *y, const float *dy, size_t outer, size_t cols, size_t inner, int mode, float *dx);" in text
    assert ("int np_cross_entropy(const float *logits, const float *target, size_t rows, size_t cols, int target_kind, float scale, "
            "float *loss_rows, float *dlogits );") in text
    order = [text.index(s) for s in ("int np_pool2d_backward(", "typedef enum np_softmax_mode", "typedef enum np_xent_target", "int np_softmax_forward(",
                                     "int np_softmax_backward(", "int np_cross_entropy(", "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_softmax_last_path(int *form);" in debug and "int np_debug_softmax_force_form(int form);" in debug
    assert "int np_debug_softmax_bounds(size_t bounds[], int n);" in debug
    order = [debug.index(s) for s in ("int np_debug_pool_forward_form(", "int np_debug_softmax_last_path(", "int np_debug_softmax_force_form(",
                                      "int np_debug_softmax_bounds(")]
    assert order == sorted(order)
    names = ("np_softmax_forward", "np_softmax_backward", "np_cross_entropy", "np_debug_softmax_last_path", "np_debug_softmax_force_form",
             "np_debug_softmax_bounds")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [6, 7, 8, 1, 1, 2]
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_softmax.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build      # the division stays the correctly rounded one


def test_the_probes_are_zero_before_any_launch():
    from numpower_amd import _lib
    lib = _lib.load()
    form = C.c_int(-7)
    assert lib.np_debug_softmax_last_path(None) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_softmax_last_path(C.byref(form)) == _lib.NP_OK and form.value == 0
    for bad in (-2, 0, 6, 115):
        assert lib.np_debug_softmax_force_form(bad) == NP_ERR_INVALID and b"form must be -1" in lib.np_last_error()
    bounds = (C.c_size_t * 5)()
    assert lib.np_debug_softmax_bounds(None, 5) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_softmax_bounds(bounds, 4) == NP_ERR_INVALID and b"room for 5" in lib.np_last_error()
    assert lib.np_debug_softmax_bounds(bounds, 5) == _lib.NP_OK
    short, wave, block, slab, slab_rows = list(bounds)
    assert 1 <= short < wave < block < 1 << 31 and slab * 4 * 2 <= 64 * 1024 and slab // (short | 1) >= 1 and slab_rows == 256
    src = (ROOT / "numpower_amd" / "csrc" / "np_softmax.hip").read_text()
    for name, value in (("kShortMaxCols", short), ("kWaveMaxCols", wave), ("kBlockMaxCols", block), ("kSlabFloats", slab), ("kSlabRowsMax", slab_rows)):
        assert "constexpr unsigned %s = %d;" % (name, value) in src
    one = C.c_void_p(64)                       # never dereferenced: every call below is refused on its arguments
    two = C.c_void_p(1 << 20)
    try:                                       # forcing a form that cannot serve the shape is refused, with no device
        for form_, shape in ((1, (4, 65, 1)), (2, (4, 1025, 1)), (3, (4, 32769, 1)), (4, (4, 8, 2)), (1, (4, 8, 2)), (2, (4, 8, 3)), (3, (4, 8, 3))):
            assert lib.np_debug_softmax_force_form(form_) == _lib.NP_OK
            assert lib.np_softmax_forward(one, *shape, 0, two) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error(), (form_, shape)
            assert lib.np_softmax_backward(one, two, *shape, 0, C.c_void_p(1 << 21)) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
        assert lib.np_debug_softmax_force_form(5) == _lib.NP_OK
        assert lib.np_cross_entropy(one, two, 4, 8, 0, 1.0, C.c_void_p(1 << 21), None) == NP_ERR_INVALID and b"cannot serve" in lib.np_last_error()
    finally:
        assert lib.np_debug_softmax_force_form(-1) == _lib.NP_OK
    assert lib.np_debug_softmax_last_path(C.byref(form)) == _lib.NP_OK and form.value == 0      # no device, no launch


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("softmax, log-softmax and cross-entropy (np_softmax.hip"):raw.index("typedef enum np_softmax_mode")]
    for phrase in ("contiguous fp32 array seen as (outer, cols, inner)", "the softmax runs over cols", "inner == 1 is the row case",
                   "m is the row maximum", "d_i = x_i - m is one fp32 subtract", "e_i = fast_exp(d_i)", "that NDArray.exp uses",
                   "exp(0) == 1 and exp(-Inf) == 0 exactly", "a chain or tree of plain fp32 adds", "depends on (cols, inner) and the kernel form alone",
                   "never depends on outer, on the row's position or on pointer alignment", "a running maximum over chunks of 8 elements",
                   "y_i = e_i / s, one correctly rounded division", "No reciprocal", "y_i = d_i - logf(s)", "as torch's CPU softmax behaves",
                   "a NaN or a +Inf, or that is entirely -Inf, comes out NaN in every element", "no other row is touched",
                   "+0.0f for softmax and -Inf for log-softmax", "dx_i = y_i . (dy_i - sum_j dy_j . y_j)", "dx_i = dy_i - fast_exp(y_i) . sum_j dy_j",
                   "fixed-order fp32 sums", "the same rule as s", "No float atomics", "class indices as fp32", "the library has one element type",
                   "loss_rows[r] = logf(s) - d_label", "bit for bit -np_softmax_forward(..., NP_LOG_SOFTMAX)[r, label]",
                   "not an integer in [0, cols), a NaN included", "that row's loss NaN and every element of its gradient NaN",
                   "Nothing is read out of bounds", "no sticky device error", "target is (rows, cols)", "loss_r = sum_j t_j . (logf(s) - d_j)",
                   "from +0.0f in ascending j", "Terms with t_j == 0 are skipped", "a one-hot row over -Inf logits is finite",
                   "gives the same bits as the index form", "dlogits_i = (p_i - t_i) . scale", "one fp32 subtract and then one multiply",
                   "p_i is bit for bit what np_softmax_forward returns", "t is assumed to sum to 1", "the one-hot of the label",
                   "ONE read of the logits, in one launch", "outputs may not overlap inputs", "dx may alias dy", "all size_t",
                   "cols >= 2^31 is refused with a message, never truncated", "outer.cols.inner beyond 2^31 elements works",
                   "runs on the library stream", "bit-identical from run to run", "a row alone gives the same bits as the same row inside a larger outer",
                   "any 4-byte-aligned pointer is accepted", "the same bits as a 16-byte-aligned one",
                   "pointers are checked first, then the extents, the mode, the aliasing, then work begins"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    a, b, c, d = (C.c_void_p(k << 24) for k in (1, 2, 3, 4))      # far apart, never dereferenced
    fwd, bwd, xent = lib.np_softmax_forward, lib.np_softmax_backward, lib.np_cross_entropy
    ok = (3, 9, 2)
    for x, y in ((None, b), (a, None)):
        assert fwd(x, *ok, 0, y) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for y, dy, dx in ((None, b, c), (a, None, c), (a, b, None)):
        assert bwd(y, dy, *ok, 1, dx) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for l, t, out in ((None, b, c), (a, None, c), (a, b, None)):
        assert xent(l, t, 3, 9, 0, 1.0, out, d) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in range(3):
        bad = list(ok)
        bad[k] = 0
        assert fwd(a, *bad, 0, b) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
        assert bwd(a, b, *bad, 0, c) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    assert xent(a, b, 0, 9, 0, 1.0, c, None) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    assert xent(a, b, 3, 0, 0, 1.0, c, None) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    for cols in (1 << 31, (1 << 31) + 5, 1 << 40, 1 << 63):      # refused, never truncated
        assert fwd(a, 1, cols, 1, 0, b) == NP_ERR_INVALID and b"2^31 or more" in lib.np_last_error()
        assert bwd(a, b, 1, cols, 1, 0, c) == NP_ERR_INVALID and b"2^31 or more" in lib.np_last_error()
        assert xent(a, b, 1, cols, 0, 1.0, c, d) == NP_ERR_INVALID and b"2^31 or more" in lib.np_last_error()
    assert fwd(a, 1 << 40, 1 << 20, 1 << 10, 0, b) == NP_ERR_INVALID and b"does not fit" in lib.np_last_error()
    for mode in (-1, 2, 115):                  # 115 = 's': the C ABI takes the enum, the characters are the glue's
        assert fwd(a, *ok, mode, b) == NP_ERR_INVALID and b"unknown mode" in lib.np_last_error()
        assert bwd(a, b, *ok, mode, c) == NP_ERR_INVALID and b"unknown mode" in lib.np_last_error()
        assert xent(a, b, 3, 9, mode, 1.0, c, d) == NP_ERR_INVALID and b"unknown target kind" in lib.np_last_error()
    # aliasing: outputs may not overlap inputs; dx == dy alone is allowed (it goes on to the device check, which is not NP_ERR_INVALID's)
    near = C.c_void_p(a.value + 8)
    assert fwd(a, *ok, 0, a) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert fwd(a, *ok, 0, near) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert bwd(a, b, *ok, 0, a) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert bwd(a, b, *ok, 0, C.c_void_p(b.value + 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert xent(a, b, 3, 9, 0, 1.0, a, None) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert xent(a, b, 3, 9, 1, 1.0, c, b) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    assert xent(a, b, 3, 9, 0, 1.0, c, C.c_void_p(c.value + 4)) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()

    src = (ROOT / "numpower_amd" / "csrc" / "np_softmax.hip").read_text()
    for name in ("int np_softmax_forward(", "int np_softmax_backward(", "int np_cross_entropy("):      # pointers, extents, mode, aliasing, form, then work
        body = _function(src, name)
        assert body.index("null pointer") < body.index("check_extents(") < body.index("unknown ") < body.index("overlap") < body.index("pick_form(") \
            < body.index("ensure_init()") < body.index("launch<")
        assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int check_extents(")
    assert body.index("at least 1") < body.index("2^31 or more") < body.index("does not fit")
    assert "ensure_init" not in body and "hip" not in body
    body = _function(src, "int pick_form(")    # the form comes from (cols, inner) alone, and from the A-B switch
    assert ("form = inner > 1 ? FORM_STRIDED : cols <= kShortMaxCols ? FORM_SHORT : cols <= kWaveMaxCols ? FORM_WAVE : cols <= kBlockMaxCols ? "
            "FORM_BLOCK : FORM_STREAM;") in body and "outer" not in body and "rows" not in body
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__fdividef" not in code and "rcp" not in code and "__expf" not in code and "Scratch" not in code


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert "NDArray *NDArrayDNN_Softmax_Forward(NDArray *x, int axis, char mode);" in host
    assert "NDArray *NDArrayDNN_Softmax_Backward(NDArray *y, NDArray *dy, int axis, char mode);" in host
    assert "NDArray *NDArrayDNN_CrossEntropy(NDArray *logits, NDArray *target, char reduction, int with_grad, NDArray **dlogits);" in host
    h = ndarray._load_host()
    assert all(hasattr(h, n) for n in ("NDArrayDNN_Softmax_Forward", "NDArrayDNN_Softmax_Backward", "NDArrayDNN_CrossEntropy"))
    glue = _header("hip_dnn.h", "ext")
    assert "struct NDArray *NPH_Softmax_Forward(struct NDArray *x, int axis, char mode);" in glue
    assert "struct NDArray *NPH_Softmax_Backward(struct NDArray *y, struct NDArray *dy, int axis, char mode);" in glue
    assert ("struct NDArray *NPH_CrossEntropy(struct NDArray *logits, struct NDArray *target, char reduction, int with_grad, "
            "struct NDArray **dlogits);") in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = _function(src, "static int softmax_of(")
    order = [checks.index("NPH_SOFTMAX_MSG_" + n) for n in ("MODE", "AXIS", "GRADIENT", "DEVICE", "CPU")]
    assert order == sorted(order) and "NDArray_Empty" not in checks and "np_softmax" not in checks
    checks = _function(src, "static int xent_of(")
    order = [checks.index("NPH_XENT_MSG_" + n) for n in ("LOGITS", "TARGET", "REDUCTION", "DEVICE", "CPU")]
    assert order == sorted(order) and "NDArray_Empty" not in checks and "np_cross_entropy" not in checks
    fwd = _function(src, "NDArray *NPH_Softmax_Forward(")
    assert fwd.index("softmax_of(") < fwd.index("empty_like_on_gpu(") < fwd.index("np_softmax_forward(")
    bwd = _function(src, "NDArray *NPH_Softmax_Backward(")
    assert bwd.index("softmax_of(") < bwd.index("empty_like_on_gpu(") < bwd.index("np_softmax_backward(")
    xe = _function(src, "NDArray *NPH_CrossEntropy(")      # one launch for the loss and the gradient, then the library's sum; the mean divides once
    assert xe.index("xent_of(") < xe.index("empty_on_gpu(") < xe.index("np_cross_entropy(") < xe.index("np_reduce_all(NP_SUM, NDArray_FDATA(loss_rows)") \
        < xe.index("total / (float) rows") < xe.index("return rtn;")
    assert xe.count("np_cross_entropy(") == 1 and "1.0f / (float) rows : 1.0f" in xe
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for name, call in (("NDArrayDNN_Softmax_Forward(", "NPH_Softmax_Forward("), ("NDArrayDNN_Softmax_Backward(", "NPH_Softmax_Backward("),
                       ("NDArrayDNN_CrossEntropy(", "NPH_CrossEntropy(")):
        body = _function(cpp, "NDArray *" + name)
        assert "on_contiguous(" in body and call in body
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "Softmax" not in tool and "CrossEntropy" not in tool      # the reference has neither: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message but the device ones needs no device."""
    from numpower_amd import ndarray
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x = ones(2, 3, 4)

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    for fn in (NDArray.softmax, NDArray.log_softmax):
        for axis in (3, -4, 17):
            assert message(fn, x, axis) == MESSAGES["NPH_SOFTMAX_MSG_AXIS"]
        for axis in (-3, -1, 0, 1, 2):                      # the right axes get as far as the device check
            assert message(fn, x, axis) == MESSAGES["NPH_SOFTMAX_MSG_CPU"]
        assert message(fn, ones(5)) == MESSAGES["NPH_SOFTMAX_MSG_CPU"] and message(fn, ones(5), 1) == MESSAGES["NPH_SOFTMAX_MSG_AXIS"]
        assert message(fn, x, 1.0) == "%s: axis must be an int" % fn.__name__
    for log in (False, True):
        assert message(NDArray.softmax_backward, x, x, 3, log) == MESSAGES["NPH_SOFTMAX_MSG_AXIS"]
        for dy in (ones(2, 3), ones(2, 3, 5), ones(3, 2, 4), ones(24)):
            assert message(NDArray.softmax_backward, x, dy, -1, log) == MESSAGES["NPH_SOFTMAX_MSG_GRADIENT"]
        assert message(NDArray.softmax_backward, x, x, 1, log) == MESSAGES["NPH_SOFTMAX_MSG_CPU"]
    logits = ones(4, 6)
    xe = NDArray.dnn_cross_entropy
    for bad in (ones(24), ones(2, 2, 6)):
        assert message(xe, bad, ones(4)) == MESSAGES["NPH_XENT_MSG_LOGITS"]
    for target in (ones(5), ones(6), ones(4, 5), ones(6, 4), ones(4, 6, 1), ones(1, 4)):
        assert message(xe, logits, target) == MESSAGES["NPH_XENT_MSG_TARGET"]
    for reduction in ("none", "sum", "mean"):
        for target in (ones(4), ones(4, 6)):
            for with_grad in (False, True):
                assert message(xe, logits, target, reduction, with_grad) == MESSAGES["NPH_XENT_MSG_CPU"]
    for reduction in ("n", "Mean", "avg", None, 0, b"mean"):
        assert message(xe, logits, ones(4), reduction) == "dnn_cross_entropy: reduction must be 'none', 'sum' or 'mean', not %r" % (reduction,)
    # the character codes: through the host library itself
    h = ndarray._load_host()
    grad = ndarray._P()
    l3, t4, t5 = ones(3), ones(4), ones(5)                  # held: a temporary would be freed before the call
    for code in (b"x", b"S", b"\0", b"m"):
        assert not h.NDArrayDNN_Softmax_Forward(x._p, 0, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_SOFTMAX_MSG_MODE"]
        assert not h.NDArrayDNN_Softmax_Backward(x._p, x._p, 0, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_SOFTMAX_MSG_MODE"]
    assert not h.NDArrayDNN_Softmax_Forward(x._p, 9, b"q")                  # the mode is checked before the axis
    assert message(ndarray._raise_pending, h) == MESSAGES["NPH_SOFTMAX_MSG_MODE"]
    for code in (b"x", b"N", b"\0", b"a"):
        assert not h.NDArrayDNN_CrossEntropy(logits._p, t4._p, code, 1, C.byref(grad)) and not grad
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_XENT_MSG_REDUCTION"]
    assert not h.NDArrayDNN_CrossEntropy(logits._p, t5._p, b"x", 0, None)      # the target is checked before the reduction
    assert message(ndarray._raise_pending, h) == MESSAGES["NPH_XENT_MSG_TARGET"]
    assert not h.NDArrayDNN_CrossEntropy(l3._p, t5._p, b"x", 0, None)      # and the logits before the target
    assert message(ndarray._raise_pending, h) == MESSAGES["NPH_XENT_MSG_LOGITS"]
