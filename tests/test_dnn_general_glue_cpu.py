"""CPU-tier checks of the strided / dilated convolution layer's boundary (np_dnn.hip, ext/hip_dnn.c, host/numpower_dnn.cpp,
ndarray.py): np_conv2d_shape_ex / _forward_ex / _backward_data_ex / _backward_filter_ex and the form probe are declared below
the old block, prototyped and exported; every refusal comes back on a machine with no device, so nothing ran; at (1, 1, 1, 1)
they refuse what the old calls refuse; each new message of the glue is raised with its text; the arithmetic of padding='same'
and its refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EX = ("np_conv2d_forward_ex", "np_conv2d_backward_data_ex", "np_conv2d_backward_filter_ex")
OLD = ("np_conv2d_forward", "np_conv2d_backward_data", "np_conv2d_backward_filter")
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_DNN_MSG_STRIDE": "dnn_conv2d: the stride must be at least 1 along both axes",
    "NPH_DNN_MSG_DILATION": "dnn_conv2d: the dilation must be at least 1 along both axes",
    "NPH_DNN_MSG_PADDING": "dnn_conv2d: the padding must be at least 0 and smaller than the effective window, dilation . (k - 1) + 1",
    "NPH_DNN_MSG_EFFECTIVE": "dnn_conv2d: the effective window, dilation . (k - 1) + 1, must not be larger than the padded input "
                             "(H + 2 ph, W + 2 pw)",
    "NPH_DNN_MSG_STRIDED_GRADIENT": "dnn_conv2d_backward: the gradient must have the shape of the forward result "
                                    "(N, F, (H + 2 ph - keh) / sh + 1, (W + 2 pw - kew) / sw + 1)",
}
SAME_REFUSED = "dnn_conv2d: padding 'same' needs stride 1 and an odd effective window, dilation . (k - 1) + 1, along both axes"


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_old_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, lib = _header("np_hip.h"), _lib.load()
    assert ("int np_conv2d_shape_ex(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, "
            "size_t dw, size_t *oh, size_t *ow);") in text
    tail = ("size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, "
            "size_t dw, float *%s);")
    assert "int np_conv2d_forward_ex(const float *x, const float *w, " + tail % "y" in text
    assert "int np_conv2d_backward_data_ex(const float *dy, const float *w, " + tail % "dx" in text
    assert "int np_conv2d_backward_filter_ex(const float *x, const float *dy, " + tail % "dw_out" in text
    assert text.index("int np_conv2d_backward_filter(") < text.index("int np_conv2d_shape_ex(")
    debug = _header("np_hip_debug.h")
    assert "int np_debug_dnn_last_form(int *host_form);" in debug and "int np_debug_dnn_last_path(int *host_tm, int *host_slices);" in debug
    for n in ("np_conv2d_shape_ex", "np_debug_dnn_last_form") + EX:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in ("np_conv2d_shape_ex",) + EX] == [12, 16, 16, 16]
    form = C.c_int(-1)
    assert lib.np_debug_dnn_last_form(None) == NP_ERR_INVALID
    assert lib.np_debug_dnn_last_form(C.byref(form)) == _lib.NP_OK and form.value == 0      # nothing launched yet


def test_the_header_states_the_general_gather():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    block = raw[raw.index("convolution layers with a stride and a dilation"):raw.index("int np_conv2d_shape_ex(")]
    for phrase in ("keh = dh (kh - 1) + 1", "0 <= ph < keh", "oh = floor((H + 2 ph - keh) / sh) + 1", "i.sh+p.dh-ph", "(u+ph-p.dh)/sh",
                   "t mod l == 0", "STORED zero", "input dilation (sh, sw)", "pad (keh - 1 - ph, kew - 1 - pw)", "sh.sw times",
                   "bit for bit the subsample", "zero-stuffed filter", "zero-stuffed dy", "return the same bits",
                   "an extent, stride or dilation of zero", "ph >= keh or pw >= kew", "keh > H + 2 ph or kew > W + 2 pw", "2^31 or more"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                       # never dereferenced: every call below is refused on its arguments
    ok = (1, 2, 9, 9, 3, 3, 3, 1, 1, 2, 2, 2, 2)          # N C H W F kh kw ph pw sh sw dh dw: keh = kew = 5
    big = 1 << 31
    cases = [((1, 2, 9, 9, 3, 3, 3, 5, 0, 2, 2, 2, 2), b"padding"), ((1, 2, 9, 9, 3, 3, 3, 0, 5, 2, 2, 2, 2), b"padding"),
             ((1, 2, 9, 9, 3, 3, 3, 3, 0, 1, 1, 1, 1), b"padding"),                                     # ph = kh at dilation 1
             ((1, 2, 4, 9, 3, 3, 3, 0, 0, 1, 1, 2, 1), b"larger than the padded image"),                # keh = 5 > 4
             ((1, 2, 9, 4, 3, 3, 3, 0, 0, 1, 1, 1, 2), b"larger than the padded image"),
             ((1, 2, 9, 9, 3, 3, 3, 0, 0, 1, 1, 5, 1), b"larger than the padded image"),                # keh = 11 > 9
             ((1, 1, 9, 9, 1, 2, 2, 0, 0, 1, 1, big, 1), b"2^31"), ((1, 1, 9, 9, 1, 2, 2, 0, 0, 1, 1, 1, big - 1), b"2^31"),   # keh, kew
             ((1, 1, 9, 9, 1, 2, 2, 0, 0, big, 1, 1, 1), b"2^31"), ((1, 1, 9, 9, 1, 2, 2, 0, 0, 1, big, 1, 1), b"2^31"),       # a stride
             ((1, 1, big - 2, 1, 1, 3, 1, 2, 0, 1, 1, 1, 1), b"2^31"), ((1, 1, 1, big - 2, 1, 1, 3, 0, 2, 1, 1, 1, 1), b"2^31"),   # H + 2 ph, W + 2 pw
             ((1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0, 0, 2, 2, 1, 1), b"2^31"), ((1, 1 << 16, 1, 1, 1 << 15, 1, 1, 0, 0, 2, 2, 1, 1), b"2^31"),
             ((1 << 16, 1, 1, 1, 1 << 15, 1, 1, 0, 0, 2, 2, 1, 1), b"2^31"), ((1, 1, big, 1, 1, 1, 1, 0, 0, 2, 2, 1, 1), b"2^31"),
             ((1 << 40, 1 << 40, 1, 1, 1, 1, 1, 0, 0, 1, 1, 2, 2), b"2^31")]
    for name in EX:
        call = getattr(lib, name)
        for ptrs in ((None, one, one), (one, None, one), (one, one, None)):
            assert call(ptrs[0], ptrs[1], *ok, ptrs[2]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
        for k in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12):      # every extent, stride and dilation
            bad = list(ok)
            bad[k] = 0
            assert call(one, one, *bad, one) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error(), (name, k)
        for bad, word in cases:
            assert call(one, one, *bad, one) == NP_ERR_INVALID and word in lib.np_last_error(), (name, bad)
    oh, ow = C.c_size_t(77), C.c_size_t(77)
    assert lib.np_conv2d_shape_ex(9, 9, 3, 3, 1, 1, 2, 2, 2, 2, None, C.byref(ow)) == NP_ERR_INVALID
    assert lib.np_conv2d_shape_ex(9, 9, 3, 3, 1, 1, 0, 2, 2, 2, C.byref(oh), C.byref(ow)) == NP_ERR_INVALID and (oh.value, ow.value) == (77, 77)
    assert lib.np_conv2d_shape_ex(9, 9, 3, 3, 1, 1, 2, 2, 0, 2, C.byref(oh), C.byref(ow)) == NP_ERR_INVALID and (oh.value, ow.value) == (77, 77)
    assert lib.np_conv2d_shape_ex(9, 10, 3, 3, 1, 1, 2, 3, 2, 2, C.byref(oh), C.byref(ow)) == _lib.NP_OK and (oh.value, ow.value) == (4, 3)
    assert lib.np_conv2d_shape_ex(224, 224, 7, 7, 3, 3, 2, 2, 1, 1, C.byref(oh), C.byref(ow)) == _lib.NP_OK and (oh.value, ow.value) == (112, 112)
    src = (ROOT / "numpower_amd" / "csrc" / "np_dnn.hip").read_text()
    for name, body_name in zip(EX, ("conv_forward", "conv_backward_data", "conv_backward_filter")):
        # the order inside each entry point: pointers, then the one body it calls; inside that: the shape, then work
        wrapper = _function(src, "int %s(" % name)
        assert wrapper.index("null pointer") < wrapper.index("return %s(" % body_name) and "<<<" not in wrapper and ".alloc(" not in wrapper, name
        body = _function(src, "int %s(" % body_name)
        work = min(body.index(w) for w in ("<<<", "launch_fprop(", "flip_filters(", "plan_wgrad(", ".alloc(") if w in body)
        assert body.index("check_layer(") < body.index("ensure_init()") < work, name


def test_unit_geometry_refuses_what_the_old_calls_refuse():
    from numpower_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)
    shapes = [(1, 2, 5, 5, 3, 3, 3, 3, 0), (1, 2, 5, 5, 3, 3, 3, 0, 3), (1, 2, 5, 5, 3, 6, 3, 0, 0), (1, 2, 5, 5, 3, 3, 10, 0, 2),
              (1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0, 0), (1, 1 << 16, 1, 1, 1 << 15, 1, 1, 0, 0), (1 << 16, 1, 1, 1, 1 << 15, 1, 1, 0, 0),
              (1, 1, 1 << 31, 1, 1, 1, 1, 0, 0), (1 << 40, 1 << 40, 1, 1, 1, 1, 1, 0, 0)]
    shapes += [tuple(0 if i == k else v for i, v in enumerate((1, 2, 5, 5, 3, 3, 3, 0, 0))) for k in range(7)]
    for old, ex in zip(OLD, EX):
        for shape in shapes:
            assert getattr(lib, old)(one, one, *shape, one) == NP_ERR_INVALID, (old, shape)
            assert getattr(lib, ex)(one, one, *shape, 1, 1, 1, 1, one) == NP_ERR_INVALID, (ex, shape)
        assert getattr(lib, old)(None, one, 1, 2, 5, 5, 3, 3, 3, 0, 0, one) == getattr(lib, ex)(None, one, 1, 2, 5, 5, 3, 3, 3, 0, 0, 1, 1, 1, 1, one)
    oh, ow, eh, ew = (C.c_size_t() for _ in range(4))
    for H, W, kh, kw, ph, pw in ((5, 7, 3, 2, 2, 1), (3, 3, 5, 5, 4, 4), (5, 5, 6, 3, 0, 0), (5, 5, 3, 3, 3, 0), (1, 1, 1, 1, 0, 0), (0, 5, 1, 1, 0, 0)):
        rc = lib.np_conv2d_shape(H, W, kh, kw, ph, pw, C.byref(oh), C.byref(ow))
        assert lib.np_conv2d_shape_ex(H, W, kh, kw, ph, pw, 1, 1, 1, 1, C.byref(eh), C.byref(ew)) == rc
        if rc == _lib.NP_OK:
            assert (eh.value, ew.value) == (oh.value, ow.value)


def test_host_and_glue_declare_the_ex_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert ("NDArray *NDArrayDNN_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int *stride, const int *padding, "
            "const int *dilation);") in host
    assert ("NDArray **NDArrayDNN_Conv2D_BackwardEx(NDArray *input, NDArray *y, NDArray *filters, const int *stride, const int *padding, "
            "const int *dilation);") in host
    h = ndarray._load_host()
    assert hasattr(h, "NDArrayDNN_Conv2D_ForwardEx") and hasattr(h, "NDArrayDNN_Conv2D_BackwardEx")
    glue = _header("hip_dnn.h", "ext")
    assert ("struct NDArray *NPH_Conv2D_ForwardEx(struct NDArray *x, struct NDArray *filters, const int stride[2], const int padding[2], "
            "const int dilation[2]);") in glue
    assert ("struct NDArray **NPH_Conv2D_BackwardEx(struct NDArray *x, struct NDArray *y, struct NDArray *filters, const int stride[2], "
            "const int padding[2], const int dilation[2]);") in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    fwd = _function(src, "NDArray *NPH_Conv2D_ForwardEx(")         # a wrapper: the geometry, then the one forward pass
    assert fwd.index("geometry_of(stride, padding, dilation)") < fwd.index("return forward(x, filters, NULL, &g, NP_ACT_NONE);")
    fwd = _function(src, "static NDArray *forward(")
    assert fwd.index("layer_of(") < fwd.index("np_conv2d_shape_ex(") < fwd.index("empty_on_gpu(") < fwd.index("np_conv2d_forward_act(")
    bwd = _function(src, "NDArray **NPH_Conv2D_BackwardEx(")
    assert bwd.index("geometry_of(stride, padding, dilation)") < bwd.index("return backward(x, NULL, y, filters, &g, NP_ACT_NONE, 0, 2);")
    bwd = _function(src, "static NDArray **backward(")
    assert bwd.index("layer_of(") < bwd.index("empty_on_gpu(") < bwd.index("np_conv2d_backward_filter_ex(") < bwd.index("np_conv2d_backward_data_ex(")
    assert bwd.index("rtns[0] = dw;") < bwd.index("rtns[1] = dx;")
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "ForwardEx" not in tool and "BackwardEx" not in tool          # the reference-signature early-outs are what they were


def test_each_new_message_is_raised_with_its_text():
    """CPU operands: the shape checks come before the device checks, so every message but the last needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, w = ones(2, 3, 8, 9), ones(4, 3, 3, 2)
    for kw, name in (({"stride": 0}, "STRIDE"), ({"stride": (2, -1)}, "STRIDE"), ({"stride": 2, "dilation": 0}, "DILATION"),
                     ({"dilation": (1, -3)}, "DILATION"), ({"stride": 2, "padding": 3}, "PADDING"), ({"stride": 2, "padding": (0, 2)}, "PADDING"),
                     ({"stride": 2, "padding": -1}, "PADDING"), ({"dilation": 2, "padding": (5, 0)}, "PADDING"),
                     ({"dilation": (4, 1)}, "EFFECTIVE"), ({"stride": 2, "dilation": (1, 9)}, "EFFECTIVE")):
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_forward(x, w, **kw)
        assert str(e.value) == MESSAGES["NPH_DNN_MSG_" + name], kw
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(x, ones(2, 4, 3, 4), w, **kw)
        assert str(e.value) == MESSAGES["NPH_DNN_MSG_" + name], kw
    # stride 2, padding 1: (8 + 2 - 3) / 2 + 1 = 4, (9 + 2 - 2) / 2 + 1 = 5
    for g in (ones(2, 4, 4, 4), ones(2, 4, 3, 5), ones(2, 4, 8, 10), ones(1, 4, 4, 5), ones(2, 3, 4, 5)):
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(x, g, w, stride=2, padding=1)
        assert str(e.value) == MESSAGES["NPH_DNN_MSG_STRIDED_GRADIENT"]
    with pytest.raises(Error) as e:                                     # the right shape gets as far as the device check
        NDArray.dnn_conv2d_backward(x, ones(2, 4, 4, 5), w, stride=2, padding=1)
    assert "operands are on the CPU" in str(e.value)
    for a, b in ((ones(3, 8, 9), w), (x, ones(4, 2, 3, 2))):            # the shared checks keep their messages and their order
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_forward(a, b, stride=0)
        assert "4-dimensional" in str(e.value) or "number of channels" in str(e.value)


def test_same_padding_arithmetic_and_refusals():
    from numpower_amd.ndarray import NDArray, Error
    geometry = lambda ws, **kw: NDArray._dnn_geometry(np.ones(ws, np.float32), kw.get("stride", 1), kw.get("padding", 0), kw.get("dilation", 1))
    values = lambda g: None if g is None else tuple(tuple(v) for v in g)          # (stride, padding, dilation)
    assert geometry((4, 3, 3, 3)) is None and geometry((4, 3, 3, 3), padding="valid") is None and geometry((4, 3, 1, 1), padding="same") is None
    assert values(geometry((4, 3, 3, 5), padding="same")) == ((1, 1), (1, 2), (1, 1))
    assert values(geometry((4, 3, 3, 3), padding="same", dilation=(2, 3))) == ((1, 1), (2, 3), (2, 3))      # keh = 5, kew = 7
    assert values(geometry((4, 3, 2, 3), padding="same", dilation=(2, 1))) == ((1, 1), (1, 1), (2, 1))      # keh = 3: even kh, odd keh
    assert values(geometry((4, 3, 3, 3), stride=2, padding=1)) == ((2, 2), (1, 1), (1, 1))
    assert values(geometry((4, 3, 3, 3), stride=(2, 3), padding=(0, 1), dilation=[1, 2])) == ((2, 3), (0, 1), (1, 2))
    assert values(geometry((4, 3, 3, 3), stride=np.int64(2))) == ((2, 2), (0, 0), (1, 1))
    for ws, kw in (((4, 3, 2, 3), {}), ((4, 3, 3, 4), {}), ((4, 3, 3, 3), {"stride": 2}), ((4, 3, 3, 3), {"stride": (1, 2)}),
                   ((4, 3, 3, 2), {"dilation": (2, 3)}), ((4, 3, 3, 3), {"dilation": 0})):
        with pytest.raises(Error) as e:
            geometry(ws, padding="same", **kw)
        assert str(e.value) == SAME_REFUSED, (ws, kw)
    for kw, what in (({"stride": 1.5}, "stride"), ({"dilation": (1, 2, 3)}, "dilation"), ({"padding": (1,)}, "padding"), ({"stride": True}, "stride"),
                     ({"padding": None}, "padding")):
        with pytest.raises(Error) as e:
            geometry((4, 3, 3, 3), **kw)
        assert str(e.value) == "dnn_conv2d: %s must be an int or a pair of ints" % what
    with pytest.raises(Error) as e:
        geometry((4, 3, 3, 3), padding="full")
    assert str(e.value) == "dnn_conv2d: padding must be an int, a pair of ints, 'valid' or 'same'"
    with pytest.raises(Error) as e:
        geometry((3, 3, 3), padding="same")
    assert "4-dimensional filters" in str(e.value)
    with pytest.raises(Error) as e:                                     # 'same' reaches the layer: (5, 5) stays (5, 5), then the device check
        NDArray.dnn_conv2d_backward(NDArray.array(np.ones((1, 1, 5, 5), np.float32)), NDArray.array(np.ones((1, 2, 5, 5), np.float32)),
                                    NDArray.array(np.ones((2, 1, 3, 3), np.float32)), padding="same")
    assert "operands are on the CPU" in str(e.value)
