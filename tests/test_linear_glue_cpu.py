"""CPU-tier checks of the boundary of the dense layer (np_linear.hip, ext/hip_dnn.c, host/numpower_dnn.cpp, ndarray.py): the two
calls are declared below the optimizer block, prototyped and exported; the probes return zeros before any launch and report the
constants that tests/linear_family.py restates; every refusal comes back on a machine with no device, so nothing ran; each
message of the glue is raised with its text; the header's comment block states each rule; the family restates the launch rules."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import linear_family as fam

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "ACTIVATION": "dnn_linear: unknown activation: 'r' (relu), 't' (tanh), 's' (sigmoid), 'n' or 0 (none)",
    "NDIM": "dnn_linear: x must have at least 1 dimension (..., K) and the weight exactly 2 (N, K)",
    "FEATURES": "dnn_linear: the last axis of x must equal the weight's second axis K (in_features)",
    "BIAS": "dnn_linear: the bias must be 1-dimensional with one element per output feature (N,)",
    "EMPTY": "dnn_linear: an operand has no elements",
    "GRADIENT": "dnn_linear_backward: the gradient must have the shape of the forward result (..., N)",
    "OUT": "dnn_linear_backward: an activation needs out, the forward result, in the shape of the gradient",
    "DEVICE": "dnn_linear: the operands must be on the same device",
    "CPU": "dnn_linear: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
}


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def _source():
    return (ROOT / "numpower_amd" / "csrc" / "np_linear.hip").read_text()


def test_abi_is_declared_below_the_optimizer_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert "int np_linear_forward(const float *x, const float *w, const float *bias , size_t M, size_t K, size_t N, int act, float *y);" in text
    assert ("int np_linear_backward(const float *x, const float *w, const float *y, const float *dy, size_t M, size_t K, size_t N, int act, "
            "float *dz, float *dx, float *dw, float *db);") in text
    order = [text.index(s) for s in ("int np_sgd_step(", "int np_grad_norm(", "int np_linear_forward(", "int np_linear_backward(", "int np_identity(")]
    assert order == sorted(order)
    assert "typedef enum np_conv_act { NP_ACT_NONE = 0, NP_ACT_RELU = 1, NP_ACT_TANH = 2, NP_ACT_SIGMOID = 3 } np_conv_act;" in text
    assert fam.ACT == {None: 0, "relu": 1, "tanh": 2, "sigmoid": 3}
    assert "int np_debug_linear_last_path(int product, int *form, int *tm, int *slices, int *launches);" in debug
    assert "int np_debug_linear_bounds(size_t bounds[], int n);" in debug and "int np_debug_linear_force_form(int form);" in debug
    names = ("np_linear_forward", "np_linear_backward", "np_debug_linear_last_path", "np_debug_linear_bounds", "np_debug_linear_force_form")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [8, 12, 5, 2, 1]
    assert _lib.PROTOTYPES["np_linear_forward"][1][3:7] == [C.c_size_t] * 3 + [C.c_int]
    assert _lib.PROTOTYPES["np_linear_backward"][1][4:8] == [C.c_size_t] * 3 + [C.c_int]
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_linear.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    code = re.sub(r"//[^\n]*", "", _source())
    assert "atomicAdd" not in code and "__hip_atomic" not in code and "hipMalloc" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in (ROOT / "numpower_amd" / "csrc" / "np_dnn_tile.h").read_text()
    # one text for the activation and the tile step: both units include the header and neither defines the functions itself
    tile = (ROOT / "numpower_amd" / "csrc" / "np_dnn_tile.h").read_text()
    dnn = (ROOT / "numpower_amd" / "csrc" / "np_dnn.hip").read_text()
    for fn in ("float act_apply(float v)", "float act_grad(float y, float dy)", "void mma_step(", "constexpr int kWgradMinSteps", "size_t mul_lim("):
        assert tile.count(fn) == 1 and fn not in dnn and fn not in code, fn
    assert '#include "np_dnn_tile.h"' in dnn and '#include "np_dnn_tile.h"' in code


def test_the_probes_are_zero_before_any_launch_and_report_the_constants():
    from numpower_amd import _lib
    lib = _lib.load()
    v = [C.c_int(-7) for _ in range(4)]
    refs = [C.byref(c) for c in v]
    assert lib.np_debug_linear_last_path(0, None, *refs[1:]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for bad in (-1, 4):
        assert lib.np_debug_linear_last_path(bad, *refs) == NP_ERR_INVALID and b"unknown product" in lib.np_last_error()
    for product in range(4):
        assert lib.np_debug_linear_last_path(product, *refs) == _lib.NP_OK and [c.value for c in v] == [0, 0, 0, 0]
    bounds = (C.c_size_t * 16)()
    assert lib.np_debug_linear_bounds(None, 16) == NP_ERR_INVALID and lib.np_debug_linear_bounds(bounds, 15) == NP_ERR_INVALID
    assert lib.np_debug_linear_bounds(bounds, 16) == _lib.NP_OK and tuple(bounds) == fam.BOUNDS       # the family's dispatcher uses the library's constants
    for bad in (-1, 3):
        assert lib.np_debug_linear_force_form(bad) == NP_ERR_INVALID and b"0 (by the extents), 1 (tile) or 2 (library)" in lib.np_last_error()
    for form in (1, 2, 0):
        assert lib.np_debug_linear_force_form(form) == _lib.NP_OK


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))
    block = raw[raw.index("dense layers (np_linear.hip"):raw.index("int np_linear_backward(")]
    for phrase in ("x (M, K), w (N, K) = (out_features, in_features), bias (N) or NULL, y (M, N)", "ONE fp32 add after the reduction",
                   "the derivative goes through the OUTPUT y", "relu a select", "dy * (1 - y*y)", "dy * ((1 - y) * y)", "each operation rounded on its own",
                   "no transposed copy of x, w or dz is written", "ONE fp32 fmaf chain from +0.0f over its reduction index in ascending order",
                   "For y the order depends on K alone, for dx on N alone", "bit for bit the row it gives inside any batch",
                   "want = min(steps / 8, ceil(512 / tiles), 256)", "adds them in slice order (S == 1 writes dw directly)",
                   "want = min(M / 256, ceil(1024 / ceil(N / 64)), 256)", "((s0 + s1) + s2) + s3", "No float atomics anywhere",
                   "a NaN in row m of x reaches exactly row m of y", "a NaN in bias[n] exactly column n", "reaches nothing",
                   "dz is NOT written and neither y nor dz is read", "it may be NULL only when dx and dw are both NULL",
                   "costs no launch; at least one must not be", "dz may be dy itself", "y may not overlap x, w or bias",
                   "no written range (dz, dx, dw, db) may overlap another written range or a range the call reads",
                   "16-byte loads", "both give the same bits", "pointers are checked first, then the extents, the activation",
                   "M.N, M.K or N.K at 2^31 or more", "Two forms", "chosen per product from (M, K, N) alone", "np_transpose2d", "batch invariance holds for the tile form only",
                   "the bits of the composition of the public calls"):
        assert phrase in block, phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    A = [C.c_void_p(k << 28) for k in range(1, 10)]                      # far apart, never dereferenced
    X, W, B, Y, DY, DZ, DX, DW, DB = A
    refused = lambda rc, text: rc == NP_ERR_INVALID and text in lib.np_last_error()
    at = lambda p, floats: C.c_void_p(p.value + 4 * floats)

    def fwd(x=X, w=W, b=B, M=5, K=7, N=3, act=1, y=Y):
        return lib.np_linear_forward(x, w, b, M, K, N, act, y)

    def bwd(x=X, w=W, y=Y, dy=DY, M=5, K=7, N=3, act=1, dz=DZ, dx=DX, dw=DW, db=DB):
        return lib.np_linear_backward(x, w, y, dy, M, K, N, act, dz, dx, dw, db)

    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        assert refused(fwd(**kw), b"np_linear_forward: null pointer")
    assert refused(fwd(x=None, M=0, act=9), b"null pointer")                                  # pointers before extents before the activation
    for kw in (dict(M=0), dict(K=0), dict(N=0)):
        assert refused(fwd(act=9, **kw), b"every extent must be at least 1") and refused(bwd(act=9, **kw), b"every extent must be at least 1")
    for kw in (dict(M=1 << 16, N=1 << 15), dict(M=1 << 16, K=1 << 15), dict(N=1 << 16, K=1 << 15), dict(M=1 << 40), dict(K=1 << 63)):
        assert refused(fwd(act=9, **kw), b"2^31 elements or more") and refused(bwd(act=9, **kw), b"2^31 elements or more")
    for bad in (-1, 4, 100):
        assert refused(fwd(act=bad), b"unknown activation") and refused(bwd(act=bad), b"unknown activation")
    assert refused(fwd(y=at(X, 34)), b"y overlaps an operand") and refused(fwd(y=at(W, -14)), b"y overlaps") and refused(fwd(y=at(B, 2)), b"y overlaps")
    assert refused(fwd(y=X), b"y overlaps")
    # backward: pointers
    assert refused(bwd(dy=None), b"np_linear_backward: null pointer")
    assert refused(bwd(dx=None, dw=None, db=None), b"nothing is asked for")
    assert refused(bwd(w=None), b"dx needs w and dw needs x") and refused(bwd(x=None), b"dx needs w and dw needs x")
    assert refused(bwd(y=None), b"an activation needs y") and refused(bwd(dz=None), b"dz where dx or dw is asked for")
    assert refused(bwd(dz=None, dx=None), b"an activation needs y, and dz")
    assert refused(bwd(dy=None, M=0), b"null pointer") and refused(bwd(y=None, act=7), b"unknown activation")
    # overlaps: dz may be dy and nothing else
    over = b"overlaps"
    assert refused(bwd(dz=at(DY, 1)), b"dz overlaps dy without being dy") and refused(bwd(dz=at(DY, -14)), b"dz overlaps dy")
    for kw in (dict(dz=Y), dict(dz=at(X, 3)), dict(dz=W), dict(dx=X), dict(dx=at(DY, 14)), dict(dx=at(Y, -30)), dict(dx=W), dict(dw=W), dict(dw=at(X, 34)),
               dict(dw=DY), dict(db=at(DY, 14)), dict(db=at(W, 20)), dict(db=at(X, -2)), dict(db=Y), dict(dx=DZ), dict(dw=at(DZ, 14)), dict(db=at(DZ, 1)),
               dict(dw=at(DX, 34)), dict(db=at(DX, 34)), dict(db=at(DW, 20)), dict(dw=DX, dx=DX)):
        assert refused(bwd(**kw), over), kw
    v = [C.c_int(-7) for _ in range(4)]
    for product in range(4):
        assert lib.np_debug_linear_last_path(product, *(C.byref(c) for c in v)) == _lib.NP_OK and [c.value for c in v] == [0, 0, 0, 0]


def test_the_family_restates_the_launch_rules():
    # the rules themselves, at the seams the GPU tests use
    assert [fam.pick_tm(r) for r in (1, 32, 33, 64, 65, 128, 129, 5000)] == [32, 32, 64, 64, 128, 128, 128, 128]
    assert [fam.dw_plan(M, 8, 8)[2] for M in (1, 480, 481, 512, 65536, 1 << 20)] == [1, 1, 2, 2, 256, 256]
    assert fam.dw_plan(4096, 1024, 1024) == (128, 16, 8) and fam.dw_plan(512, 3900, 2100)[2] == 1
    assert [fam.act_plan(M, 8)[1] for M in (1, 511, 512, 65536, 1 << 20)] == [1, 1, 2, 256, 256]
    assert fam.act_plan(4096, 1024) == (256, 16) and fam.act_plan(5, 8) == (8, 1)
    # the dispatcher: per product, by the work M.K.N alone; a forced form overrides it
    for p in (fam.Y, fam.DX, fam.DW):
        t = fam.LIB_MIN_WORK[p]
        assert fam.form_of(p, 1, 1, 1) == fam.TILE or t <= 1
        assert fam.form_of(p, 4096, 4096, 4096) == (fam.LIBRARY if 4096 ** 3 >= t else fam.TILE)
        assert fam.form_of(p, 1, 1, 1, force=2) == fam.LIBRARY and fam.form_of(p, 4096, 4096, 4096, force=1) == fam.TILE
        if 1 < t < 1 << 60:
            assert fam.form_of(p, t, 1, 1) == fam.LIBRARY and fam.form_of(p, t - 1, 1, 1) == fam.TILE
    for M, K, N in ((1, 1, 1), (481, 8, 8), (1025, 40, 130), (100000, 7, 300)):
        tm, per, S = fam.dw_plan(M, K, N)
        assert (S - 1) * per * fam.STEP < M <= S * per * fam.STEP                          # every slice holds rows
        rows, Sb = fam.act_plan(M, N)
        assert rows % 4 == 0 and (Sb - 1) * rows < M <= Sb * rows


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert "NDArray *NDArrayDNN_Linear_Forward(NDArray *x, NDArray *weight, NDArray *bias, char activation);" in host
    assert "NDArray **NDArrayDNN_Linear_Backward(NDArray *x, NDArray *out, NDArray *dy, NDArray *weight, char activation, int use_bias, int need_dx);" in host
    h = ndarray._load_host()
    assert all(hasattr(h, n) for n in ("NDArrayDNN_Linear_Forward", "NDArrayDNN_Linear_Backward", "NPH_Linear_Forward", "NPH_Linear_Backward"))
    glue = _header("hip_dnn.h", "ext")
    assert "struct NDArray *NPH_Linear_Forward(struct NDArray *x, struct NDArray *weight, struct NDArray *bias, char activation);" in glue
    assert "struct NDArray **NPH_Linear_Backward(struct NDArray *x, struct NDArray *out, struct NDArray *dy, struct NDArray *weight, char activation," in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = _function(src, "static int linear_of(")
    order = [checks.index("NPH_LINEAR_MSG_" + n) for n in ("ACTIVATION", "NDIM", "FEATURES", "BIAS", "EMPTY", "GRADIENT", "OUT", "DEVICE", "CPU")]
    assert order == sorted(order) and "np_linear_" not in checks
    body = _function(src, "NDArray **NPH_Linear_Backward(")
    assert body.index("linear_of(") < body.index("np_malloc(&dz") < body.index("np_linear_backward(") < body.index("np_free(dz)") < body.index("batchnorm_drop(")
    assert "need_dx ? empty_like_on_gpu(x) : NULL" in body
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    assert "NPH_Linear_Forward(cx, cw, cb, activation)" in cpp and "NPH_Linear_Backward(cx, co, cy, cw, activation, use_bias, need_dx)" in cpp
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "Linear_" not in tool and "dnn_linear" not in tool and "np_linear" not in tool  # the reference has no dense layer: no anchored edit
    example = (ROOT / "examples" / "linear_classifier.py").read_text()
    assert "transpose" not in example and "matmul" not in example and "optim.AdamW(" in example and "need_dx=False" in example


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message before them needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define NPH_LINEAR_MSG_%s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    fwd, bwd = NDArray.dnn_linear_forward, NDArray.dnn_linear_backward

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    M = MESSAGES
    assert message(fwd, ones(3, 4), ones(2, 3, 4)) == M["NDIM"] and message(fwd, ones(3, 4), ones(4)) == M["NDIM"]
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4, 1)) == M["NDIM"]
    assert message(fwd, ones(3, 4), ones(5, 3)) == M["FEATURES"] and message(bwd, ones(3, 4), ones(3, 5), ones(5, 3)) == M["FEATURES"]
    assert message(fwd, ones(3, 4), ones(5, 4), ones(4)) == M["BIAS"] and message(fwd, ones(3, 4), ones(5, 4), ones(5, 1)) == M["BIAS"]
    empty = NDArray.array(np.ones((0, 4), np.float32))
    assert message(fwd, empty, ones(5, 4)) == M["EMPTY"] and message(fwd, ones(3, 4), NDArray.array(np.ones((0, 4), np.float32))) == M["EMPTY"]
    assert message(bwd, ones(3, 4), ones(3, 4), ones(5, 4)) == M["GRADIENT"] and message(bwd, ones(3, 4), ones(4, 5), ones(5, 4)) == M["GRADIENT"]
    assert message(bwd, ones(2, 3, 4), ones(6, 5), ones(5, 4)) == M["GRADIENT"] and message(bwd, ones(4), ones(1, 5), ones(5, 4)) == M["GRADIENT"]
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4), out=ones(3, 4), activation="tanh") == M["OUT"]
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4), out=ones(15), activation="relu") == M["OUT"]
    assert message(fwd, ones(3, 4), ones(5, 3), ones(4)) == M["FEATURES"]                      # in the order of the header
    # the right operands get as far as the device check
    assert message(fwd, ones(3, 4), ones(5, 4)) == M["CPU"] and message(fwd, ones(2, 3, 4), ones(5, 4), ones(5), "sigmoid") == M["CPU"]
    assert message(fwd, ones(4), ones(5, 4)) == M["CPU"]
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4)) == M["CPU"] and message(bwd, ones(3, 4), ones(3, 5), ones(5, 4), bias=True, need_dx=False) == M["CPU"]
    assert message(bwd, ones(2, 3, 4), ones(2, 3, 5), ones(5, 4), out=ones(2, 3, 5), activation="relu") == M["CPU"]
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4), out=ones(7)) == M["CPU"]          # without an activation out is not looked at
    # the binding's own argument checks
    assert message(fwd, ones(3, 4), ones(5, 4), activation="gelu") == "dnn_linear: activation must be None, 'relu', 'tanh' or 'sigmoid', not 'gelu'"
    assert message(bwd, ones(3, 4), ones(3, 5), ones(5, 4), activation="relu") == \
        "dnn_linear_backward: an activation needs out, the forward result (gradients are expressed through the output)"
    assert message(NDArray.dnn_conv2d_forward, ones(1, 1, 3, 3), ones(1, 1, 2, 2), activation="gelu").startswith("dnn_conv2d: activation must be")
    # the glue's own activation check, through the host library
    h = __import__("numpower_amd.ndarray", fromlist=["_load_host"])._load_host()
    assert not h.NDArrayDNN_Linear_Forward(ones(3, 4)._p, ones(5, 4)._p, None, b"x")
    with pytest.raises(Error) as e:
        __import__("numpower_amd.ndarray", fromlist=["_raise_pending"])._raise_pending(h)
    assert str(e.value) == M["ACTIVATION"]
