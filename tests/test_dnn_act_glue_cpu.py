"""CPU-tier checks of the boundary of the convolution layer's bias and activation (np_dnn.hip, ext/hip_dnn.c,
host/numpower_dnn.cpp, ndarray.py): np_conv2d_forward_act / np_conv2d_backward_act and the epilogue probe are declared below the
_ex block, prototyped and exported; every refusal comes back on a machine with no device, so nothing ran; each new message of
the glue is raised with its text; the defaults of both NDArray methods reach the old host functions; the reference-signature
functions still say that they ignore `activation` and `use_bias`."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_DNN_MSG_ACTIVATION": "dnn_conv2d: unknown activation: 'r' (relu), 't' (tanh), 's' (sigmoid), 'n' or 0 (none)",
    "NPH_DNN_MSG_BIAS": "dnn_conv2d: the bias must be 1-dimensional with one element per filter (F,)",
    "NPH_DNN_MSG_OUT": "dnn_conv2d_backward: out, the forward result, must have the shape of the gradient",
    "NPH_DNN_MSG_BIAS_DEVICE": "dnn_conv2d: the bias must be on the device of the input and the filters",
}
NEEDS_OUT = "dnn_conv2d_backward: an activation needs out, the forward result (gradients are expressed through the output)"
CPU = "operands are on the CPU"


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_ex_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, lib = _header("np_hip.h"), _lib.load()
    assert "typedef enum np_conv_act { NP_ACT_NONE = 0, NP_ACT_RELU = 1, NP_ACT_TANH = 2, NP_ACT_SIGMOID = 3 } np_conv_act;" in text
    assert ("int np_conv2d_forward_act(const float *x, const float *w, const float *bias, size_t N, size_t C, size_t H, size_t W, size_t F, "
            "size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, int act, float *y);") in text
    assert "int np_conv2d_backward_act(const float *y, const float *dy, size_t N, size_t F, size_t P, int act, float *dz, float *db);" in text
    order = [text.index(s) for s in ("int np_conv2d_shape(", "int np_conv2d_shape_ex(", "int np_conv2d_backward_filter_ex(", "typedef enum np_conv_act",
                                     "int np_conv2d_forward_act(", "int np_conv2d_backward_act(")]
    assert order == sorted(order)
    assert "int np_debug_dnn_last_epilogue(int *act, int *has_bias, int *bias_slices);" in _header("np_hip_debug.h")
    for n in ("np_conv2d_forward_act", "np_conv2d_backward_act", "np_debug_dnn_last_epilogue"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in ("np_conv2d_forward_act", "np_conv2d_backward_act", "np_debug_dnn_last_epilogue")] == [18, 8, 3]


def test_the_probe_returns_zeros_before_any_launch():
    from numpower_amd import _lib
    lib = _lib.load()
    act, bias, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.np_debug_dnn_last_epilogue(None, C.byref(bias), C.byref(s)) == NP_ERR_INVALID
    assert lib.np_debug_dnn_last_epilogue(C.byref(act), C.byref(bias), None) == NP_ERR_INVALID and act.value == -1
    assert lib.np_debug_dnn_last_epilogue(C.byref(act), C.byref(bias), C.byref(s)) == _lib.NP_OK
    assert (act.value, bias.value, s.value) == (0, 0, 0)


def test_the_header_states_the_layer():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("convolution layers with a bias and an activation"):raw.index("typedef enum np_conv_act")]
    for phrase in ("v = bias ? acc + bias[f] : acc", "ONE fp32 add after the chain", "NOT the chain's start value", "(v <= 0) ? +0.0f : v",
                   "a NaN stays NaN, -0.0 becomes +0.0", "tanhf(v)", "bit for bit the unfused result", "1 / (1 + exp(-v))",
                   "0 and 1 at -Inf and +Inf, NaN at NaN", "read for f < F only", "launches the same kernels as np_conv2d_forward_ex",
                   "expressed through the output", "(y <= 0) ? +0.0f : dy", "a select, not a product", "a NaN y passes dy", "dy * (1 - y*y)",
                   "dy * ((1 - y) * y)", "db[f] = sum_{n,i,j} dz[n,f,i,j]", "dz is NOT written", "only dz is written", "m = n.P + i.ow + j",
                   "S and L from (N, F, P) alone", "in ascending order", "fixed tree", "in slice order", "S == 1 writes db directly",
                   "No float atomics", "bit-identical from run to run", "dz may not overlap y or dy; db may not overlap anything",
                   "pointers are checked first, then the shape, then work begins", "an unknown act", "dz and db both NULL",
                   "NULL with an activation", "an extent of zero", "2^31 or more"):
        assert phrase.lower() in block.lower(), phrase
    old = raw[raw.index("convolution layers (np_dnn.hip"):raw.index("int np_conv2d_shape(")]
    assert "no bias, no activation" in old                       # the plain calls say what they always said


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                       # never dereferenced: every call below is refused on its arguments
    ok = (1, 2, 9, 9, 3, 3, 3, 1, 1, 2, 2, 2, 2)          # N C H W F kh kw ph pw sh sw dh dw: keh = kew = 5
    big = 1 << 31
    fwd = lib.np_conv2d_forward_act
    for ptrs in ((None, one, one), (one, None, one), (one, one, None)):
        for bias in (None, one):
            assert fwd(ptrs[0], ptrs[1], bias, *ok, 1, ptrs[2]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12):      # every extent, stride and dilation
        bad = list(ok)
        bad[k] = 0
        assert fwd(one, one, one, *bad, 1, one) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error(), k
    for bad, word in (((1, 2, 9, 9, 3, 3, 3, 5, 0, 2, 2, 2, 2), b"padding"), ((1, 2, 9, 9, 3, 3, 3, 3, 0, 1, 1, 1, 1), b"padding"),
                      ((1, 2, 4, 9, 3, 3, 3, 0, 0, 1, 1, 2, 1), b"larger than the padded image"),
                      ((1, 1, 9, 9, 1, 2, 2, 0, 0, 1, 1, big, 1), b"2^31"), ((1, 1, 9, 9, 1, 2, 2, 0, 0, big, 1, 1, 1), b"2^31"),
                      ((1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0, 0, 2, 2, 1, 1), b"2^31"), ((1 << 40, 1 << 40, 1, 1, 1, 1, 1, 0, 0, 1, 1, 2, 2), b"2^31")):
        for act in (0, 1):
            assert fwd(one, one, None, *bad, act, one) == NP_ERR_INVALID and word in lib.np_last_error(), bad
            assert lib.np_conv2d_forward_ex(one, one, *bad, one) == NP_ERR_INVALID and word in lib.np_last_error(), bad
    for act in (-1, 4, 114):                    # 114 = 'r': the C ABI takes the enum, the characters are the glue's
        assert fwd(one, one, one, *ok, act, one) == NP_ERR_INVALID and b"unknown activation" in lib.np_last_error()

    bwd = lib.np_conv2d_backward_act
    assert bwd(one, None, 2, 3, 4, 1, one, one) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for act in (0, 1, 2, 3):
        assert bwd(one, one, 2, 3, 4, act, None, None) == NP_ERR_INVALID and b"dz and db are both null" in lib.np_last_error()
    for act in (1, 2, 3):                       # dz (or y) NULL with an activation
        assert bwd(one, one, 2, 3, 4, act, None, one) == NP_ERR_INVALID and b"an activation needs y and dz" in lib.np_last_error()
        assert bwd(None, one, 2, 3, 4, act, one, one) == NP_ERR_INVALID and b"an activation needs y and dz" in lib.np_last_error()
    for k in range(3):
        ext = [2, 3, 4]
        ext[k] = 0
        assert bwd(one, one, *ext, 1, one, one) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    for ext in ((1 << 11, 1 << 10, 1 << 10), (big, 1, 1), (1, big, 1), (1, 1, big), (1 << 40, 1 << 40, 1 << 40)):
        assert bwd(one, one, *ext, 1, one, one) == NP_ERR_INVALID and b"2^31" in lib.np_last_error(), ext
    for act in (-1, 4, 114):
        assert bwd(one, one, 2, 3, 4, act, one, one) == NP_ERR_INVALID and b"unknown activation" in lib.np_last_error()
    assert bwd(None, one, 2, 3, 4, 0, one, None) == _lib.NP_OK         # no activation, no db: dz = dy, nothing to do, no device

    src = (ROOT / "numpower_amd" / "csrc" / "np_dnn.hip").read_text()
    body = _function(src, "int np_conv2d_forward_act(")            # pointers, then the one forward body; inside that: shape, activation, work
    assert body.index("null pointer") < body.index("return conv_forward(") and "<<<" not in body and ".alloc(" not in body
    body = _function(src, "int conv_forward(")
    assert body.index("check_layer(") < body.index("unknown activation") < body.index("ensure_init()") < body.index("launch_fprop(a, bias, act)")
    body = _function(src, "int launch_fprop(")                     # one launcher: no bias and no activation take the plain instantiations
    assert "const bool epi = bias || act != NP_ACT_NONE;" in body and "launch_fprop_form<0, false>" in body and "launch_fprop_form<2, true>" not in body
    body = src[src.index("int np_conv2d_backward_act("):]
    body = body[:body.index("\n}\n")]
    assert body.index("null pointer") < body.index("at least 1") < body.index("2^31") < body.index("unknown activation") < body.index("ensure_init()") \
        < body.index(".alloc(") < body.index("launch_act_grad(")
    assert "<<<" not in body and "atomic" not in src.replace("No float atomics", "")
    for name in ("kActBlock = 256", "kActMinSlice = 4096", "kActTargetGroups = 2048", "kActMaxSlices = 256"):      # tests/dnn_act_family.py mirrors them
        assert name in src[:src.index("struct ConvCore")], name
    # the epilogue's operands travel in a struct of their own: the plain kernels' argument is what it was
    core = src[src.index("struct ConvCore {"):src.index("// a kernel's argument")]
    assert "bias" not in core and "act" not in core.replace("extents", "") and "struct EpiArgs : KernelArgs<FORM>" in src


def test_host_and_glue_declare_the_layer_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert ("NDArray *NDArrayDNN_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int *stride, const int *padding, "
            "const int *dilation, char activation);") in host
    assert ("NDArray **NDArrayDNN_Conv2D_LayerBackward(NDArray *input, NDArray *out, NDArray *dy, NDArray *filters, const int *stride, "
            "const int *padding, const int *dilation, char activation, int use_bias);") in host
    h = ndarray._load_host()
    assert hasattr(h, "NDArrayDNN_Conv2D_LayerForward") and hasattr(h, "NDArrayDNN_Conv2D_LayerBackward")
    glue = _header("hip_dnn.h", "ext")
    assert ("struct NDArray *NPH_Conv2D_LayerForward(struct NDArray *x, struct NDArray *filters, struct NDArray *bias, const int stride[2], "
            "const int padding[2], const int dilation[2], char activation);") in glue
    assert ("struct NDArray **NPH_Conv2D_LayerBackward(struct NDArray *x, struct NDArray *out, struct NDArray *dy, struct NDArray *filters, "
            "const int stride[2], const int padding[2], const int dilation[2], char activation, int use_bias);") in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    fwd = _function(src, "NDArray *NPH_Conv2D_LayerForward(")      # a wrapper: the geometry, the activation's code, then the one forward pass
    assert fwd.index("geometry_of(stride, padding, dilation)") < fwd.index("return forward(x, filters, bias, &g, activation_of(activation));")
    fwd = _function(src, "static NDArray *forward(")
    assert fwd.index("layer_extras(") < fwd.index("layer_of(") < fwd.index("np_conv2d_shape_ex(") < fwd.index("empty_on_gpu(") < fwd.index("np_conv2d_forward_act(")
    bwd = _function(src, "NDArray **NPH_Conv2D_LayerBackward(")
    assert bwd.index("geometry_of(stride, padding, dilation)") < bwd.index("return backward(x, out, dy, filters, &g, activation_of(activation), use_bias, 3);")
    bwd = _function(src, "static NDArray **backward(")
    assert bwd.index("layer_extras(") < bwd.index("layer_of(") < bwd.index("empty_on_gpu(") < bwd.index("np_malloc(&dz") \
        < bwd.index("np_conv2d_backward_act(") < bwd.index("np_conv2d_backward_filter_ex(") < bwd.index("np_conv2d_backward_data_ex(") \
        < bwd.index("np_free(dz)") < bwd.index("if (!ok)") < bwd.index("rtns[0] = dw;") < bwd.index("rtns[1] = dx;") < bwd.index("rtns[2] = db;")
    extras = src[src.index("static int layer_extras("):src.index("/* a new GPU array")]
    order = [extras.index("NPH_DNN_MSG_" + n) for n in ("ACTIVATION", "BIAS)", "OUT", "BIAS_DEVICE")]
    assert order == sorted(order) and "NDArray_Empty" not in extras and "np_conv2d" not in extras
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "LayerForward" not in tool and "LayerBackward" not in tool      # the reference-signature early-outs are what they were


def test_the_reference_signature_functions_still_ignore_activation_and_use_bias():
    host = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for name, call in (("NDArrayDNN_Conv2D_Forward(", "NPH_Conv2D_Forward("), ("NDArrayDNN_Conv2D_Backward(", "NPH_Conv2D_Backward(")):
        body = host[host.index(name):]
        body = body[:body.index("\n}\n")]
        assert "(void) kernel_size, (void) activation, (void) use_bias;" in body and call in body and "Layer" not in body
    assert "are ignored" in host[:host.index("#include")]
    glue = (ROOT / "ext" / "hip_dnn.h").read_text()
    assert "the reference ignores `activation` and `use_bias` on both paths" in glue and "keep\n * ignoring them" in glue
    assert "struct NDArray *NPH_Conv2D_Forward(struct NDArray *x, struct NDArray *filters);" in glue
    public = re.sub(r"\s+", " ", (ROOT / "include" / "numpower_host.h").read_text().replace(" * ", " "))
    assert "activation and use_bias are ignored" in public and "still ignore `activation` and `use_bias`" in public


def test_each_new_message_is_raised_with_its_text():
    """CPU operands: the layer's own checks come before the shared ones, so every message but the device one needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 8, 9), ones(4, 3, 3, 2), ones(2, 4, 6, 8)

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    for bias in (ones(3), ones(5), ones(4, 1), ones(1, 4), ones(2, 2)):
        assert message(NDArray.dnn_conv2d_forward, x, w, bias=bias) == MESSAGES["NPH_DNN_MSG_BIAS"]
        assert message(NDArray.dnn_conv2d_forward, x, w, bias=bias, activation="tanh", stride=2) == MESSAGES["NPH_DNN_MSG_BIAS"]
    for out in (ones(2, 4, 6, 7), ones(2, 4, 48), ones(1, 4, 6, 8), ones(2, 4, 6, 8, 1)):
        for act in ("relu", "tanh", "sigmoid", None):
            assert message(NDArray.dnn_conv2d_backward, x, dy, w, out=out, activation=act) == MESSAGES["NPH_DNN_MSG_OUT"]
    # the right shapes get as far as the device check, through the layer's functions
    assert CPU in message(NDArray.dnn_conv2d_forward, x, w, bias=ones(4))
    assert CPU in message(NDArray.dnn_conv2d_forward, x, w, activation="relu")
    assert CPU in message(NDArray.dnn_conv2d_forward, x, w, bias=ones(4), activation="sigmoid", stride=2, padding=1)
    assert CPU in message(NDArray.dnn_conv2d_backward, x, dy, w, out=dy, activation="relu", bias=True)
    assert CPU in message(NDArray.dnn_conv2d_backward, x, dy, w, bias=True)
    # the shared checks keep their messages behind the layer's
    assert "4-dimensional" in message(NDArray.dnn_conv2d_forward, ones(3, 8, 9), w, bias=ones(4))
    assert "number of channels" in message(NDArray.dnn_conv2d_forward, x, ones(4, 2, 3, 2), bias=ones(4), activation="relu")
    assert "the stride must be at least 1" in message(NDArray.dnn_conv2d_forward, x, w, activation="relu", stride=0)
    assert "the gradient must have the shape of the forward result" in message(NDArray.dnn_conv2d_backward, x, ones(2, 4, 6, 7), w,
                                                                               out=ones(2, 4, 6, 7), activation="relu")
    # the character codes: through the host library itself
    from numpower_amd import ndarray
    h = ndarray._load_host()
    for code in (b"x", b"R", b"1"):
        assert not h.NDArrayDNN_Conv2D_LayerForward(x._p, w._p, None, None, None, None, code)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_DNN_MSG_ACTIVATION"]
        assert not h.NDArrayDNN_Conv2D_LayerBackward(x._p, dy._p, dy._p, w._p, None, None, None, code, 1)
        assert message(ndarray._raise_pending, h) == MESSAGES["NPH_DNN_MSG_ACTIVATION"]
    for code in (b"r", b"t", b"s", b"n", b"\0"):
        assert not h.NDArrayDNN_Conv2D_LayerForward(x._p, w._p, None, None, None, None, code)
        assert CPU in message(ndarray._raise_pending, h)
    assert not h.NDArrayDNN_Conv2D_LayerBackward(x._p, None, dy._p, w._p, None, None, None, b"r", 0)      # an activation and no out
    assert message(ndarray._raise_pending, h) == MESSAGES["NPH_DNN_MSG_OUT"]


def test_the_keywords_of_the_ndarray_methods():
    from numpower_amd.ndarray import NDArray, Error
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 8, 9), ones(4, 3, 3, 2), ones(2, 4, 6, 8)
    for act in ("r", "Relu", "none", 1, b"relu", True):
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_forward(x, w, activation=act)
        assert str(e.value) == "dnn_conv2d: activation must be None, 'relu', 'tanh' or 'sigmoid', not %r" % (act,)
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(x, dy, w, out=dy, activation=act)
        assert str(e.value) == "dnn_conv2d: activation must be None, 'relu', 'tanh' or 'sigmoid', not %r" % (act,)
    for act in ("relu", "tanh", "sigmoid"):     # backward with an activation needs out
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(x, dy, w, activation=act)
        assert str(e.value) == NEEDS_OUT
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(x, dy, w, activation=act, bias=True, stride=2)
        assert str(e.value) == NEEDS_OUT
    geometry = NDArray._dnn_geometry(np.ones((4, 3, 3, 3), np.float32), 1, 0, 1)      # four arguments, as before
    assert geometry is None


def test_the_defaults_reach_the_old_host_functions(monkeypatch):
    from numpower_amd import ndarray
    from numpower_amd.ndarray import NDArray, Error
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 8, 9), ones(4, 3, 3, 2), ones(2, 4, 6, 8)
    real, calls = ndarray._load_host(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("NDArrayDNN_"):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped

    monkeypatch.setattr(ndarray, "_load_host", lambda: Spy())

    def refused(fn, *a, **kw):
        del calls[:]
        with pytest.raises(Error):
            fn(*a, **kw)
        return list(calls)

    assert refused(NDArray.dnn_conv2d_forward, x, w) == ["NDArrayDNN_Conv2D_Forward"]
    assert refused(NDArray.dnn_conv2d_forward, x, w, bias=None, activation=None) == ["NDArrayDNN_Conv2D_Forward"]
    assert refused(NDArray.dnn_conv2d_forward, x, w, stride=2) == ["NDArrayDNN_Conv2D_LayerForward"]      # any keyword: the layer's function
    assert refused(NDArray.dnn_conv2d_forward, x, w, activation="relu") == ["NDArrayDNN_Conv2D_LayerForward"]
    assert refused(NDArray.dnn_conv2d_forward, x, w, bias=ones(4), stride=2) == ["NDArrayDNN_Conv2D_LayerForward"]
    assert refused(NDArray.dnn_conv2d_backward, x, dy, w) == ["NDArrayDNN_Conv2D_Backward"]
    assert refused(NDArray.dnn_conv2d_backward, x, dy, w, out=None, activation=None, bias=False) == ["NDArrayDNN_Conv2D_Backward"]
    assert refused(NDArray.dnn_conv2d_backward, x, ones(2, 4, 3, 4), w, stride=2) == ["NDArrayDNN_Conv2D_LayerBackward"]
    assert refused(NDArray.dnn_conv2d_backward, x, dy, w, bias=True) == ["NDArrayDNN_Conv2D_LayerBackward"]
    assert refused(NDArray.dnn_conv2d_backward, x, dy, w, out=dy, activation="tanh") == ["NDArrayDNN_Conv2D_LayerBackward"]
    assert refused(NDArray.dnn_conv2d_backward, x, dy, w, activation="tanh") == []                  # refused before any host call
