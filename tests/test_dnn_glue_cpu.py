"""CPU-tier checks of the convolution layer's boundary (np_dnn.hip, ext/hip_dnn.c, host/numpower_dnn.cpp): np_conv2d_shape /
_forward / _backward_data / _backward_filter are declared, prototyped and exported and refuse null and bad-shape arguments before
any device work; the header states the convention; NDArrayDNN_Conv2D_Forward / _Backward have the reference's signatures and this
project's messages; the --with-hip early-outs are a list of their own that is NOT part of EDITS and reaches a tree, with the glue,
only under --dnn; dnn_bodies shows CPU operands reaching the reference's own code."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT_INCLUDE = "dnn.c:4: <hip_dnn.h>"
WHAT_FORWARD = "dnn.c:275 NDArrayDNN_Conv2D_Forward: GPU early-out"
WHAT_BACKWARD = "dnn.c:314 NDArrayDNN_Conv2D_Backward: GPU early-out"
ENTRY_POINTS = ("np_conv2d_forward", "np_conv2d_backward_data", "np_conv2d_backward_filter")
MESSAGES = {
    "NPH_DNN_MSG_NDIM": "dnn_conv2d: the operands must be 4-dimensional: the input (N, C, H, W), the filters (F, C, kh, kw)",
    "NPH_DNN_MSG_CHANNELS": "dnn_conv2d: the filters' second extent must equal the input's number of channels",
    "NPH_DNN_MSG_WINDOW": "dnn_conv2d: the filter window must not be larger than the input (kh <= H and kw <= W)",
    "NPH_DNN_MSG_GRADIENT": "dnn_conv2d_backward: the gradient must have the shape of the forward result (N, F, H - kh + 1, W - kw + 1)",
    "NPH_DNN_MSG_DEVICE": "dnn_conv2d: the operands must be on the same device",
    "NPH_DNN_MSG_CPU": "dnn_conv2d: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first, the CPU path "
                       "is the reference's own)",
}
GCC_CHECK = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-I", str(ROOT / "include"), "-I", str(ROOT / "ext")]
NP_ERR_INVALID = -1            # np_hip.h: np_status
HAS_REF = (REF / "numpower.c").exists()


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _tool():
    sys.path.insert(0, str(ROOT / "tools"))
    import apply_with_hip
    return apply_with_hip


def test_abi_is_declared_prototyped_and_exported():
    from numpower_amd import _lib
    text = _header("np_hip.h")
    lib = _lib.load()
    assert "int np_conv2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t *oh, size_t *ow);" in text
    tail = "size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw, size_t ph, size_t pw, float *%s);"
    assert "int np_conv2d_forward(const float *x, const float *w, " + tail % "y" in text
    assert "int np_conv2d_backward_data(const float *dy, const float *w, " + tail % "dx" in text
    assert "int np_conv2d_backward_filter(const float *x, const float *dy, " + tail % "dw" in text
    assert "int np_debug_dnn_last_path(int *host_tm, int *host_slices);" in _header("np_hip_debug.h")
    for n in ("np_conv2d_shape", "np_debug_dnn_last_path") + ENTRY_POINTS:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in ("np_conv2d_shape",) + ENTRY_POINTS] == [8, 12, 12, 12]
    assert "np_dnn.hip" in (ROOT / "numpower_amd" / "build.py").read_text()


def test_the_header_states_the_convention():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    block = raw[raw.index("convolution layers (np_dnn.hip"):raw.index("int np_conv2d_shape(")]
    for phrase in ("x (N, C, H, W), w (F, C, kh, kw)", "Cross-correlation with stride 1, dilation 1", "0 <= ph < kh, 0 <= pw < kw",
                   "no bias, no activation", "STORED zeros", "an Inf tap gives NaN", "no im2col matrix is written",
                   "flipped and transposed into pool scratch", "pad (kh - 1 - ph, kw - 1 - pw)", "S from the extents alone",
                   "added in slice order", "No float atomics", "depends on (C, kh, kw)", "never on N",
                   "same bits at any batch size and position", "bit-identical from run to run",
                   "pointers are checked first, then the shape, then work begins", "an extent of zero", "ph >= kh or pw >= kw",
                   "kh > H + 2 ph or kw > W + 2 pw", "2^31 or more", "refused, never truncated", "released on every path"):
        assert phrase.lower() in block.lower(), phrase


def test_null_and_bad_shape_arguments_are_refused_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                       # never dereferenced: every call below is refused on its arguments
    ok = (1, 2, 5, 5, 3, 3, 3, 0, 0)
    for name in ENTRY_POINTS:
        call = getattr(lib, name)
        for ptrs in ((None, one, one), (one, None, one), (one, one, None)):
            assert call(ptrs[0], ptrs[1], *ok, ptrs[2]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
        for k in range(7):
            bad = list(ok)
            bad[k] = 0
            assert call(one, one, *bad, one) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
        for bad, word in (((1, 2, 5, 5, 3, 3, 3, 3, 0), b"padding"), ((1, 2, 5, 5, 3, 3, 3, 0, 3), b"padding"),
                          ((1, 2, 5, 5, 3, 6, 3, 0, 0), b"larger than the padded image"), ((1, 2, 5, 5, 3, 3, 10, 0, 2), b"larger than the padded image"),
                          ((1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0, 0), b"2^31"), ((1, 1 << 16, 1, 1, 1 << 15, 1, 1, 0, 0), b"2^31"),
                          ((1 << 16, 1, 1, 1, 1 << 15, 1, 1, 0, 0), b"2^31"), ((1, 1, 1 << 31, 1, 1, 1, 1, 0, 0), b"2^31"),
                          ((1 << 40, 1 << 40, 1, 1, 1, 1, 1, 0, 0), b"2^31"),
                          # a padded extent H + 2 ph (W + 2 pw) of 2^31 + 4 with every count below 2^31: the row index i + p - ph is an int
                          ((1, 1, (1 << 31) - 2, 1, 1, 6, 1, 3, 0), b"2^31"), ((1, 1, 1, (1 << 31) - 2, 1, 1, 6, 0, 3), b"2^31")):
            assert call(one, one, *bad, one) == NP_ERR_INVALID and word in lib.np_last_error(), (name, bad)
    oh, ow = C.c_size_t(77), C.c_size_t(77)
    assert lib.np_conv2d_shape(5, 5, 3, 3, 0, 0, None, C.byref(ow)) == NP_ERR_INVALID
    assert lib.np_conv2d_shape(5, 5, 6, 3, 0, 0, C.byref(oh), C.byref(ow)) == NP_ERR_INVALID and (oh.value, ow.value) == (77, 77)
    assert lib.np_conv2d_shape(5, 7, 3, 2, 2, 1, C.byref(oh), C.byref(ow)) == _lib.NP_OK and (oh.value, ow.value) == (7, 8)
    assert lib.np_conv2d_shape(3, 3, 5, 5, 4, 4, C.byref(oh), C.byref(ow)) == _lib.NP_OK and (oh.value, ow.value) == (7, 7)
    src = (ROOT / "numpower_amd" / "csrc" / "np_dnn.hip").read_text()
    for name, body_name in zip(ENTRY_POINTS, ("conv_forward", "conv_backward_data", "conv_backward_filter")):
        # the order inside each entry point: pointers, then the one body it calls; inside that: the shape, then work
        wrapper = _function(src, "int %s(" % name)
        assert wrapper.index("null pointer") < wrapper.index("return %s(" % body_name) and "<<<" not in wrapper and ".alloc(" not in wrapper, name
        body = _function(src, "int %s(" % body_name)
        work = min(body.index(w) for w in ("<<<", "launch_fprop(", "flip_filters(", "plan_wgrad(", ".alloc(") if w in body)
        assert body.index("check_layer(") < body.index("ensure_init()") < work, name
    checks = src[src.index("int check_spatial("):src.index("ConvArgs dgrad_layer(")]
    assert "int check_layer(" in checks and checks.count("NP_ERR_INVALID") >= 5 and "<<<" not in checks and "alloc" not in checks
    assert "atomic" not in src.replace("No float atomics", "")


def test_host_functions_have_the_reference_signatures():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert "NDArray *NDArrayDNN_Conv2D_Forward(NDArray *x, NDArray *filters, int *kernel_size, char activation, int use_bias);" in host
    assert ("NDArray **NDArrayDNN_Conv2D_Backward(NDArray *input, NDArray *y, NDArray *filters, int kernel_size, char activation, "
            "int use_bias);") in host
    h = ndarray._load_host()
    assert hasattr(h, "NDArrayDNN_Conv2D_Forward") and hasattr(h, "NDArrayDNN_Conv2D_Backward")
    glue = _header("hip_dnn.h", "ext")
    assert "struct NDArray *NPH_Conv2D_Forward(struct NDArray *x, struct NDArray *filters);" in glue
    assert "struct NDArray **NPH_Conv2D_Backward(struct NDArray *x, struct NDArray *y, struct NDArray *filters);" in glue
    assert callable(ndarray.NDArray.dnn_conv2d_forward) and callable(ndarray.NDArray.dnn_conv2d_backward)


@pytest.mark.skipif(not (REF / "src" / "dnn.h").exists(), reason="needs a NumPower checkout to compare with")
def test_the_signatures_are_the_ones_the_reference_declares():
    ref = re.sub(r"\s+", "", (REF / "src" / "dnn.h").read_text())
    ours = re.sub(r"\s+", "", _header("numpower_host.h"))
    for decl in ("NDArray*NDArrayDNN_Conv2D_Forward(NDArray*x,NDArray*filters,int*kernel_size,charactivation,intuse_bias);",
                 "NDArray**NDArrayDNN_Conv2D_Backward(NDArray*input,NDArray*y,NDArray*filters,intkernel_size,charactivation,intuse_bias);"):
        assert decl in ref and decl in ours


def test_each_message_is_raised_with_its_text():
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    x, w, dy = ones(2, 3, 6, 7), ones(4, 3, 3, 2), ones(2, 4, 4, 6)
    for a, b, name in ((ones(3, 6, 7), w, "NDIM"), (x, ones(3, 3, 2), "NDIM"), (x, ones(4, 2, 3, 2), "CHANNELS"), (x, ones(4, 3, 7, 2), "WINDOW"),
                       (x, ones(4, 3, 3, 8), "WINDOW"), (x, w, "CPU")):
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_forward(a, b)
        assert str(e.value) == MESSAGES["NPH_DNN_MSG_" + name]
    for a, g, b, name in ((x, ones(2, 4, 4), w, "NDIM"), (x, dy, ones(4, 2, 3, 2), "CHANNELS"), (x, dy, ones(4, 3, 7, 2), "WINDOW"),
                          (x, ones(2, 4, 4, 5), w, "GRADIENT"), (x, ones(2, 3, 4, 6), w, "GRADIENT"), (x, ones(1, 4, 4, 6), w, "GRADIENT"),
                          (x, dy, w, "CPU")):
        with pytest.raises(Error) as e:
            NDArray.dnn_conv2d_backward(a, g, b)
        assert str(e.value) == MESSAGES["NPH_DNN_MSG_" + name]


def test_the_glue_checks_before_it_allocates_and_keeps_the_reference_order():
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = src[src.index("static int layer_of("):src.index("/* NULL: the default */")]
    order = [checks.index("NPH_DNN_MSG_" + n) for n in ("NDIM", "CHANNELS", "WINDOW", "GRADIENT", "DEVICE", "CPU")]
    assert order == sorted(order) and "NDArray_Empty" not in checks and "np_conv2d" not in checks
    assert "NDArray *NPH_Conv2D_Forward(NDArray *x, NDArray *filters) { return forward(x, filters, NULL, NULL, NP_ACT_NONE); }" in src
    assert ("NDArray **NPH_Conv2D_Backward(NDArray *x, NDArray *y, NDArray *filters) { return backward(x, NULL, y, filters, NULL, NP_ACT_NONE, 0, 2); }"
            in src)
    fwd = _function(src, "static NDArray *forward(")              # the one forward pass, which the call above reaches
    assert fwd.index("layer_of(") < fwd.index("np_conv2d_shape_ex(") < fwd.index("empty_on_gpu(") < fwd.index("np_conv2d_forward_act(")
    assert "np_ext_throw_last();" in fwd and "NDArray_FREE(rtn);" in fwd
    bwd = _function(src, "static NDArray **backward(")            # and the one backward pass
    assert bwd.index("layer_of(") < bwd.index("empty_on_gpu(") < bwd.index("np_conv2d_backward_filter_ex(") < bwd.index("np_conv2d_backward_data_ex(")
    assert bwd.index("rtns[0] = dw;") < bwd.index("rtns[1] = dx;") and "np_ext_throw_last();" in bwd
    assert "dw_dims[4] = {l.F, l.C, l.kh, l.kw}" in bwd and "dx_dims[4] = {l.N, l.C, l.H, l.W}" in bwd      # the filters' own shape, the input's
    assert "empty_on_gpu(4, dw_dims)" in bwd and "empty_on_gpu(4, dx_dims)" in bwd
    assert "hip_dnn.c" in (ROOT / "ext" / "config.m4").read_text() and "hip_dnn.c" in (ROOT / "ext" / "README.md").read_text()


def test_the_edits_are_a_list_of_their_own_outside_edits_and_pass_the_snippet_check(tmp_path):
    tool = _tool()
    assert len(tool.DNN_EDITS) == 3
    for other in (tool.EDITS, tool.SIGNAL_EDITS, tool.EIG_EDITS, tool.QR_EDITS):
        assert not any(e in other for e in tool.DNN_EDITS)
    assert len(tool.EDITS) == 77
    include, fwd, bwd = tool.DNN_EDITS
    assert (include.what, fwd.what, bwd.what) == (WHAT_INCLUDE, WHAT_FORWARD, WHAT_BACKWARD)
    assert include.new == "#include <hip_dnn.h>" and all(e.after and not e.guard and e.file == "src/dnn.c" for e in tool.DNN_EDITS)
    assert "NPH_DNN_TAKES(x, filters)" in fwd.new and "return NPH_Conv2D_Forward(x, filters);" in fwd.new
    assert "NPH_DNN_TAKES3(input, y, filters)" in bwd.new and "return NPH_Conv2D_Backward(input, y, filters);" in bwd.new
    assert not any("hip_dnn" in g for g in tool.GLUE_FILES) and "hip_dnn" not in tool.HIP_M4_BLOCK
    default = tool.snippet_check_source()
    assert "NPH_Conv2D" not in default and "hip_dnn" not in default
    src = tool.snippet_check_source(tool.DNN_EDITS)
    assert "/* %s */" % WHAT_FORWARD in src and "/* %s */" % WHAT_BACKWARD in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    for k, (old, new) in enumerate((("return NPH_Conv2D_Forward(x, filters);", "return NPH_Conv2D_Forward(x);"),
                                    ("return NPH_Conv2D_Backward(input, y, filters);", "return NPH_Conv2D_Backward(input, filters);"),
                                    ("NPH_DNN_TAKES3(", "NPH_DNN_TAKES("))):
        bad_src = src.replace(old, new)
        assert bad_src != src
        bad = tmp_path / ("bad%d.c" % k)
        bad.write_text(bad_src)
        assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_dnn_bodies_cpu_operands_reach_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "dnn_bodies"
    tool = _tool()
    gen = tool.dnn_program_source()
    for e in tool.DNN_EDITS[1:]:
        for line in e.new.split("\n"):
            assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "dnn_bodies cpu: 2 calls reached the reference's own code, 0 failures" in proc.stdout


def test_the_layer_stays_out_of_the_translation_unit_the_null_device_build_compiles():
    for path in (ROOT / "tests" / "null_device").iterdir():
        if path.is_file():
            text = path.read_text(errors="replace")
            assert "np_conv2d" not in text and "Conv2D" not in text, path
    host = (ROOT / "numpower_amd" / "host" / "numpower_host.cpp").read_text()
    assert "np_conv2d" not in host and "Conv2D" not in host and "hip_dnn" not in host
    dnn = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    assert "NDArrayDNN_Conv2D_Forward" in dnn and "NDArrayDNN_Conv2D_Backward" in dnn and "Operand" in dnn


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_device_layer_only_when_asked(tmp_path):
    tool = _tool()
    plain, out = tmp_path / "plain", tmp_path / "numpower"
    before = tool.apply(REF, plain)
    applied = tool.apply(REF, out, extra=tool.DNN_EDITS)
    assert dict(applied) == dict(before) and len(applied) == len(tool.EDITS)
    assert applied.extra == {WHAT_INCLUDE: 1, WHAT_FORWARD: 1, WHAT_BACKWARD: 1}
    for path in plain.rglob("*"):                                  # the default tree: no mention of the glue anywhere
        if path.is_file():
            assert "hip_dnn" not in path.name
            text = path.read_text(errors="replace")
            assert "hip_dnn" not in text and "NPH_Conv2D" not in text, path
    assert (out / "src" / "hip" / "hip_dnn.c").read_text() == (ROOT / "ext" / "hip_dnn.c").read_text()
    assert (out / "src" / "hip" / "hip_dnn.h").read_text() == (ROOT / "ext" / "hip_dnn.h").read_text()
    m4, plain_m4 = (out / "config.m4").read_text(), (plain / "config.m4").read_text()
    assert m4.count("src/hip/hip_dnn.c") == 1 and m4.replace(" src/hip/hip_dnn.c", "") == plain_m4
    text, plain_text = (out / "src" / "dnn.c").read_text(), (plain / "src" / "dnn.c").read_text()
    assert text.count("#include <hip_dnn.h>") == 1
    text = text.replace("#ifdef HAVE_NP_HIP\n#include <hip_dnn.h>\n#endif\n", "", 1)
    for opening, call, first in (("NDArrayDNN_Conv2D_Forward(NDArray *x,", "return NPH_Conv2D_Forward(x, filters);", "NDArray *rtn = NULL;"),
                                 ("NDArrayDNN_Conv2D_Backward(NDArray *input,", "return NPH_Conv2D_Backward(input, y, filters);", "emalloc(")):
        body = _function(text, opening)
        assert body.count(call) == 1
        assert body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_DNN_TAKES") < body.index(call) < body.index("#endif") < body.index(first)
        inserted = body[body.index("#ifdef HAVE_NP_HIP"):body.index("#endif") + len("#endif\n")]
        text = text.replace(inserted, "", 1)
    assert text == plain_text                                      # without the inserted blocks: the tree the tool makes without `extra`
    others = {p.relative_to(out) for p in out.rglob("*") if p.is_file()} - {p.relative_to(plain) for p in plain.rglob("*") if p.is_file()}
    assert others == {Path("src/hip/hip_dnn.c"), Path("src/hip/hip_dnn.h")}


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_command_line_counts(tmp_path, capsys):
    tool = _tool()
    assert "[--dnn]" in tool.__doc__
    assert tool.main(["apply_with_hip.py", str(REF), str(tmp_path / "a")]) == 0
    out = capsys.readouterr().out
    assert "79 edits in" in out and "dnn.c" not in out
    assert tool.main(["apply_with_hip.py", "--dnn", str(REF), str(tmp_path / "b")]) == 0
    out = capsys.readouterr().out
    assert "82 edits in" in out and all("applied x1  %s" % w in out for w in (WHAT_INCLUDE, WHAT_FORWARD, WHAT_BACKWARD))
    assert tool.main(["apply_with_hip.py", "--qr", "--dnn", str(REF), str(tmp_path / "c")]) == 0
    assert "84 edits in" in capsys.readouterr().out
    assert not (tmp_path / "a" / "src" / "hip" / "hip_dnn.c").exists() and (tmp_path / "b" / "src" / "hip" / "hip_dnn.c").exists()
    assert "NPH_Conv2D" not in (tmp_path / "a" / "src" / "dnn.c").read_text() and "NPH_Conv2D" in (tmp_path / "b" / "src" / "dnn.c").read_text()
