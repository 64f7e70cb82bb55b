"""CPU-tier checks of the boundary of the pooling layers (np_pool.hip, ext/hip_dnn.c, host/numpower_dnn.cpp, ndarray.py): the enum
and the three calls are declared below the conv block, prototyped and exported; the probe returns zeros before any launch; every
refusal comes back on a machine with no device, so nothing ran; each message of the glue is raised with its text; the header's
comment block states each rule."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_POOL_MSG_MODE": "dnn_pool2d: unknown mode: 'm' (max), 'a' (average, padding counts), 'v' (average over the real cells)",
    "NPH_POOL_MSG_NDIM": "dnn_pool2d: the input must be 4-dimensional (N, C, H, W), and so must the gradient",
    "NPH_POOL_MSG_WINDOW": "dnn_pool2d: the window must be at least 1 along both axes",
    "NPH_POOL_MSG_STRIDE": "dnn_pool2d: the stride must be at least 1 along both axes",
    "NPH_POOL_MSG_PADDING": "dnn_pool2d: the padding must be at least 0 and at most half the window (2 ph <= kh and 2 pw <= kw)",
    "NPH_POOL_MSG_LARGER": "dnn_pool2d: the window must not be larger than the padded input (H + 2 ph, W + 2 pw)",
    "NPH_POOL_MSG_GRADIENT": "dnn_pool2d_backward: the gradient must have the shape of the forward result "
                             "(N, C, (H + 2 ph - kh) / sh + 1, (W + 2 pw - kw) / sw + 1)",
    "NPH_POOL_MSG_DEVICE": "dnn_pool2d: the operands must be on the same device",
    "NPH_POOL_MSG_CPU": "dnn_pool2d: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
}


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_conv_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, lib = _header("np_hip.h"), _lib.load()
    assert "typedef enum np_pool_mode { NP_POOL_MAX = 0, NP_POOL_AVG = 1, NP_POOL_AVG_VALID = 2 } np_pool_mode;" in text
    assert ("int np_pool2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t *oh, "
            "size_t *ow);") in text
    assert ("int np_pool2d_forward(const float *x, size_t planes, size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, "
            "size_t sh, size_t sw, int mode, float *y, int32_t *idx);") in text
    assert ("int np_pool2d_backward(const float *dy, const int32_t *idx, size_t planes, size_t H, size_t W, size_t kh, size_t kw, "
            "size_t ph, size_t pw, size_t sh, size_t sw, int mode, float *dx);") in text
    order = [text.index(s) for s in ("int np_conv2d_shape(", "int np_conv2d_backward_act(", "typedef enum np_pool_mode", "int np_pool2d_shape(",
                                     "int np_pool2d_forward(", "int np_pool2d_backward(", "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_pool_last_path(int *forward_form, int *backward_form);" in _header("np_hip_debug.h")
    assert "int np_debug_pool_forward_form(int form);" in _header("np_hip_debug.h")
    names = ("np_pool2d_shape", "np_pool2d_forward", "np_pool2d_backward", "np_debug_pool_last_path", "np_debug_pool_forward_form")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [10, 13, 13, 2, 1]
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_pool.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build      # the division stays the correctly rounded one


def test_the_probe_returns_zeros_before_any_launch():
    from numpower_amd import _lib
    lib = _lib.load()
    f, b = C.c_int(-1), C.c_int(-1)
    assert lib.np_debug_pool_last_path(None, C.byref(b)) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_pool_last_path(C.byref(f), None) == NP_ERR_INVALID and f.value == -1
    assert lib.np_debug_pool_last_path(C.byref(f), C.byref(b)) == _lib.NP_OK
    assert (f.value, b.value) == (0, 0)
    for form in (-1, 2, 109):
        assert lib.np_debug_pool_forward_form(form) == NP_ERR_INVALID and b"form must be 0" in lib.np_last_error()
    assert lib.np_debug_pool_forward_form(1) == _lib.NP_OK and lib.np_debug_pool_forward_form(0) == _lib.NP_OK      # no device, no launch
    assert lib.np_debug_pool_last_path(C.byref(f), C.byref(b)) == _lib.NP_OK and (f.value, b.value) == (0, 0)


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("pooling layers: max and average pool2d"):raw.index("typedef enum np_pool_mode")]
    for phrase in ("(planes, H, W) row-major fp32, contiguous", "planes = N.C", "2 ph <= kh and 2 pw <= kw", "at least one real cell",
                   "no dilation and no ceil mode", "oh = floor((H + 2 ph - kh) / sh) + 1", "clipped to [0, H)", "row-major order",
                   "best = -Inf", "idx = the first real cell", "v > best || v != v", "the first of equal maxima wins", "-0.0 and +0.0 are equal",
                   "the index is that of the last NaN", "Padding is never a candidate", "idx[plane, i, j] = u.W + v", "int32 within the plane",
                   "writing idx is optional", "one chain of plain fp32 adds from +0.0f", "one correctly rounded fp32 division by (float) divisor",
                   "divisor = kh.kw: padding counts", "No multiplication by a reciprocal", "divisor = the number of real cells",
                   "a gather, never a scatter", "i ascending, then j ascending", "idx[i,j] == u.W + v", "dy[i,j] / (float) divisor(i,j)",
                   "rounded on its own before the add", "stride > window, or the floor remainder", "get +0.0f", "No float atomics",
                   "bit-identical from run to run", "does not depend on how many planes are in the call",
                   "reaches exactly the outputs whose window holds it", "reaches exactly the dx cells that term is added to",
                   "library stream and need no scratch", "np_pool2d_shape needs no device",
                   "pointers are checked first, then the shape, then work begins", "idx == NULL for a max backward", "a zero extent, window or stride",
                   "an unknown mode", "2 ph > kh or 2 pw > kw", "kh > H + 2 ph or kw > W + 2 pw", "kh.kw at 2^24 or more",
                   "H.W, numel(x), numel(y), a stride, H + 2 ph or W + 2 pw at 2^31 or more", "refused, never truncated"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                       # never dereferenced: every call below is refused on its arguments
    ok = (3, 9, 9, 3, 3, 1, 1, 2, 2)           # planes H W kh kw ph pw sh sw
    big = 1 << 31
    fwd, bwd = lib.np_pool2d_forward, lib.np_pool2d_backward
    for x, y in ((None, one), (one, None)):
        for idx in (None, one):
            assert fwd(x, *ok, 0, y, idx) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for mode in (0, 1, 2):
        assert bwd(None, one, *ok, mode, one) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
        assert bwd(one, one, *ok, mode, None) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert bwd(one, None, *ok, 0, one) == NP_ERR_INVALID and b"null pointer: the max mode needs idx" in lib.np_last_error()

    def both(shape, word, modes=(0, 1, 2)):
        for mode in modes:
            assert fwd(one, *shape, mode, one, one) == NP_ERR_INVALID and word in lib.np_last_error(), (shape, lib.np_last_error())
            assert bwd(one, one, *shape, mode, one) == NP_ERR_INVALID and word in lib.np_last_error(), (shape, lib.np_last_error())
        if shape[0] == 1:
            oh, ow = C.c_size_t(77), C.c_size_t(77)
            assert lib.np_pool2d_shape(*shape[1:], C.byref(oh), C.byref(ow)) == NP_ERR_INVALID and word in lib.np_last_error(), shape
            assert (oh.value, ow.value) == (77, 77)

    for k in (0, 1, 2, 3, 4, 7, 8):            # every extent, window and stride
        bad = list(ok)
        bad[k] = 0
        both(bad, b"at least 1")
    for mode in (-1, 3, 109):                  # 109 = 'm': the C ABI takes the enum, the characters are the glue's
        both(ok, b"unknown mode", modes=(mode,))
    both((1, 9, 9, 3, 3, 2, 1, 1, 1), b"padding")              # 2 ph > kh
    both((1, 9, 9, 3, 2, 1, 2, 1, 1), b"padding")              # 2 pw > kw
    both((1, 9, 9, 1, 1, 1, 0, 1, 1), b"padding")
    both((1, 9, 9, 3, 3, big, 0, 1, 1), b"padding")
    both((1, 4, 9, 5, 3, 0, 0, 1, 1), b"larger than the padded image")
    both((1, 9, 2, 3, 5, 1, 1, 1, 1), b"larger than the padded image")     # kw = 5 > W + 2 pw = 4
    both((1, 1 << 40, 9, 1 << 50, 3, 0, 0, 1, 1), b"larger than the padded image")
    both((1, 4096, 4096, 4096, 4096, 0, 0, 1, 1), b"2^24")     # kh.kw = 2^24
    both((1, 1 << 25, 8, 1 << 24, 1, 0, 0, 1, 1), b"2^24")
    both((1, 1 << 16, 1 << 15, 2, 2, 0, 0, 2, 2), b"2^31")     # H.W
    both((1, big, 1, 1, 1, 0, 0, 1, 1), b"2^31")
    both((1, 1, 1 << 62, 1, 1, 0, 0, 1, 1), b"2^31")
    both((1 << 16, 1 << 8, 1 << 7, 2, 2, 0, 0, 2, 2), b"2^31")     # numel(x)
    both((big, 1, 1, 1, 1, 0, 0, 1, 1), b"2^31")
    both((1 << 40, 1 << 40, 1 << 40, 1, 1, 0, 0, 1, 1), b"2^31")
    both((1, 9, 9, 3, 3, 1, 1, big, 1), b"2^31")               # a stride
    both((1, 9, 9, 3, 3, 1, 1, 1, 1 << 63), b"2^31")
    both((1, big - 2, 1, 2, 1, 1, 0, 1, 1), b"2^31")           # H + 2 ph = 2^31
    both((1, 1, big - 2, 1, 3, 0, 1, 1, 1), b"2^31")           # W + 2 pw = 2^31
    # numel(y) alone cannot pass numel(x) + padding by much: planes . oh . ow with a padded 1 x 1 window of stride 1
    both(((1 << 30) + (1 << 29), 1, 1, 2, 2, 1, 1, 1, 1), b"numel(y)")      # numel(x) = 1.5 . 2^30, numel(y) = 4 numel(x)

    oh, ow = C.c_size_t(0), C.c_size_t(0)
    assert lib.np_pool2d_shape(9, 9, 3, 3, 1, 1, 2, 2, None, C.byref(ow)) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_pool2d_shape(9, 9, 3, 3, 1, 1, 2, 2, C.byref(oh), None) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_pool2d_shape(9, 9, 3, 3, 1, 1, 2, 2, C.byref(oh), C.byref(ow)) == _lib.NP_OK and (oh.value, ow.value) == (5, 5)      # no device

    src = (ROOT / "numpower_amd" / "csrc" / "np_pool.hip").read_text()
    for name in ("int np_pool2d_forward(", "int np_pool2d_backward("):       # pointers, the shape, the mode, then work
        body = _function(src, name)
        assert body.index("null pointer") < body.index("check_pool(") < body.index("unknown mode") < body.index("ensure_init()") < body.index("launch_")
        assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int check_pool(")
    assert body.index("at least 1") < body.index("padding") < body.index("larger than the padded image") < body.index("2^24") < body.index("2^31")
    assert "ensure_init" not in body and "hip" not in body.replace("np_hip", "")
    assert "atomic" not in src.replace("No float atomics", "") and "__fdividef" not in src and "rcp" not in src
    assert "kPoolBlock = 256" in src and "kStageCells = 8192" in src         # tests/test_gpu_dnn_pool.py mirrors them
    body = _function(src, "int launch_forward(")                             # the form comes from the extents alone (and the A-B switch)
    assert "const bool staged = !g_pool_force_direct && (size_t)a.H * (size_t)a.W <= (size_t)kStageCells;" in body


def test_host_and_glue_declare_the_pooling_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert "NDArray *NDArrayDNN_Pool2D_Forward(NDArray *x, const int *kernel, const int *stride, const int *padding, char mode);" in host
    assert "NDArray *NDArrayDNN_Pool2D_Backward(NDArray *x, NDArray *dy, const int *kernel, const int *stride, const int *padding, char mode);" in host
    h = ndarray._load_host()
    assert hasattr(h, "NDArrayDNN_Pool2D_Forward") and hasattr(h, "NDArrayDNN_Pool2D_Backward")
    glue = _header("hip_dnn.h", "ext")
    assert ("struct NDArray *NPH_Pool2D_Forward(struct NDArray *x, const int kernel[2], const int stride[2], const int padding[2], "
            "char mode);") in glue
    assert ("struct NDArray *NPH_Pool2D_Backward(struct NDArray *x, struct NDArray *dy, const int kernel[2], const int stride[2], "
            "const int padding[2], char mode);") in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = _function(src, "static int pool_of(")
    order = [checks.index("NPH_POOL_MSG_" + n) for n in ("MODE", "NDIM", "WINDOW", "STRIDE", "PADDING", "LARGER", "GRADIENT", "DEVICE", "CPU")]
    assert order == sorted(order) and "NDArray_Empty" not in checks and "np_pool2d" not in checks
    fwd = _function(src, "NDArray *NPH_Pool2D_Forward(")
    assert fwd.index("pool_of(") < fwd.index("empty_on_gpu(") < fwd.index("np_pool2d_forward(")
    bwd = _function(src, "NDArray *NPH_Pool2D_Backward(")      # max: the forward pass again into scratch, then the gather; released on every path
    assert bwd.index("pool_of(") < bwd.index("empty_on_gpu(") < bwd.index("np_malloc(&again") < bwd.index("np_pool2d_forward(") \
        < bwd.index("np_pool2d_backward(") < bwd.index("np_free(again)") < bwd.index("if (!ok)") < bwd.index("return dx;")
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for name, call in (("NDArrayDNN_Pool2D_Forward(", "NPH_Pool2D_Forward("), ("NDArrayDNN_Pool2D_Backward(", "NPH_Pool2D_Backward(")):
        body = _function(cpp, "NDArray *" + name)
        assert "on_contiguous(" in body and call in body
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "Pool2D" not in tool                # the reference has no pooling: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message but the device one needs no device."""
    from numpower_amd import ndarray
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x = ones(2, 3, 8, 9)

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    fwd, bwd = NDArray.dnn_pool2d_forward, NDArray.dnn_pool2d_backward
    for mode in ("max", "avg", "avg_valid"):
        assert message(fwd, ones(3, 8, 9), 2, mode=mode) == MESSAGES["NPH_POOL_MSG_NDIM"]
        assert message(bwd, x, ones(2, 3, 16), 2, mode=mode) == MESSAGES["NPH_POOL_MSG_NDIM"]
        for k in (0, (2, 0), (-1, 2)):
            assert message(fwd, x, k, mode=mode) == MESSAGES["NPH_POOL_MSG_WINDOW"]
        for s in (0, (1, 0), (-2, 1)):
            assert message(fwd, x, 2, stride=s, mode=mode) == MESSAGES["NPH_POOL_MSG_STRIDE"]
        for k, p in ((2, 2), (3, 2), (3, (1, 2)), (3, -1), (1, 1), ((2, 5), (1, 3))):
            assert message(fwd, x, k, padding=p, mode=mode) == MESSAGES["NPH_POOL_MSG_PADDING"]
        for k, p in ((9, 0), ((8, 10), 0), ((11, 3), 1), ((3, 12), (1, 1))):
            assert message(fwd, x, k, padding=p, mode=mode) == MESSAGES["NPH_POOL_MSG_LARGER"]
        for dy in (ones(2, 3, 4, 5), ones(2, 3, 5, 4), ones(1, 3, 4, 4), ones(2, 2, 4, 4)):      # the result is (2, 3, 4, 4): stride = the window
            assert message(bwd, x, dy, 2, mode=mode) == MESSAGES["NPH_POOL_MSG_GRADIENT"]
        assert message(bwd, x, ones(2, 3, 4, 4), 2, stride=1, mode=mode) == MESSAGES["NPH_POOL_MSG_GRADIENT"]
        # the right shapes get as far as the device check
        assert message(fwd, x, 2, mode=mode) == MESSAGES["NPH_POOL_MSG_CPU"]
        assert message(fwd, x, (3, 2), stride=(2, 1), padding=(1, 0), mode=mode) == MESSAGES["NPH_POOL_MSG_CPU"]
        assert message(fwd, x, (8, 9), mode=mode) == MESSAGES["NPH_POOL_MSG_CPU"]          # window = image
        assert message(bwd, x, ones(2, 3, 4, 4), 2, mode=mode) == MESSAGES["NPH_POOL_MSG_CPU"]
        assert message(bwd, x, ones(2, 3, 4, 5), 3, stride=2, padding=1, mode=mode) == MESSAGES["NPH_POOL_MSG_CPU"]
    # the character codes and a missing window: through the host library itself
    h = ndarray._load_host()
    two = (C.c_int * 2)(2, 2)
    for code in (b"x", b"M", b"\0", b"r"):
        assert not h.NDArrayDNN_Pool2D_Forward(x._p, two, None, None, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_POOL_MSG_MODE"]
        assert not h.NDArrayDNN_Pool2D_Backward(x._p, x._p, two, None, None, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_POOL_MSG_MODE"]
    for code in (b"m", b"a", b"v"):
        assert not h.NDArrayDNN_Pool2D_Forward(x._p, two, None, None, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_POOL_MSG_CPU"]
        assert not h.NDArrayDNN_Pool2D_Forward(x._p, None, None, None, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_POOL_MSG_WINDOW"]


def test_the_arguments_of_the_ndarray_methods():
    from numpower_amd.ndarray import NDArray, Error
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, dy = ones(2, 3, 8, 9), ones(2, 3, 4, 4)
    for mode in ("m", "Max", "average", None, 0, b"max"):
        for call in (lambda: NDArray.dnn_pool2d_forward(x, 2, mode=mode), lambda: NDArray.dnn_pool2d_backward(x, dy, 2, mode=mode)):
            with pytest.raises(Error) as e:
                call()
            assert str(e.value) == "dnn_pool2d: mode must be 'max', 'avg' or 'avg_valid', not %r" % (mode,)
    for what, kw in (("kernel_size", {"kernel_size": 2.0}), ("kernel_size", {"kernel_size": (2, 2, 2)}), ("kernel_size", {"kernel_size": True}),
                     ("stride", {"kernel_size": 2, "stride": "2"}), ("stride", {"kernel_size": 2, "stride": (1,)}),
                     ("padding", {"kernel_size": 2, "padding": None}), ("padding", {"kernel_size": 2, "padding": (1, 1.5)})):
        with pytest.raises(Error) as e:
            NDArray.dnn_pool2d_forward(x, **kw)
        assert str(e.value) == "dnn_pool2d: %s must be an int or a pair of ints" % what
        with pytest.raises(Error) as e:
            NDArray.dnn_pool2d_backward(x, dy, **kw)
        assert str(e.value) == "dnn_pool2d: %s must be an int or a pair of ints" % what
    k, s, p, code = NDArray._dnn_pool_geometry((3, 2), None, 1, "avg_valid")
    assert (list(k), s, list(p), code) == ([3, 2], None, [1, 1], b"v")
    k, s, p, code = NDArray._dnn_pool_geometry(np.int64(2), [2, 1], (0, 1), "max")
    assert (list(k), list(s), list(p), code) == ([2, 2], [2, 1], [0, 1], b"m")
