"""CPU-tier checks of the 2-D correlation's boundary (np_signal.hip, ext/hip_signal.c, host/numpower_signal.cpp): the ABI is
declared, prototyped and exported and refuses bad arguments before any device work; NDArray_Correlate2D has the reference's
signature and messages; the --with-hip early-out is a list of its own that leaves the 77 edits of EDITS as they were, sits in
front of the reference's GPU throw and compiles; signal_bodies shows CPU operands reaching the reference's own code."""
import ctypes as C
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT = "signal.c:218 NDArray_Correlate2D: GPU early-out"
CALL = "if (NPH_SIGNAL_TAKES(a, b)) return NPH_Correlate2D(a, b, mode, boundary, fill_value, flip);"
PROTO = "NDArray *NDArray_Correlate2D(NDArray *a, NDArray *b, int mode, int boundary, NDArray *fill_value, int flip);"
GCC_CHECK = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-I", str(ROOT / "include"), "-I", str(ROOT / "ext")]


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
    assert "int np_correlate2d_shape(size_t ah, size_t aw, size_t bh, size_t bw, int mode, size_t *oh, size_t *ow);" in text
    assert ("int np_correlate2d(const float *a, size_t ah, size_t aw, const float *b, size_t bh, size_t bw, int mode, int boundary, "
            "float fill_value, int flip, float *out);") in text
    assert "NP_CONV_VALID = 0, NP_CONV_SAME = 1, NP_CONV_FULL = 2" in text           # signal.h:16-18
    assert "NP_CONV_FILL = 0, NP_CONV_SYMM = 4, NP_CONV_WRAP = 8" in text            # signal.h:20-22
    assert "int np_debug_conv2d_last_path(int *host_path);" in _header("np_hip_debug.h")
    for n in ("np_correlate2d", "np_correlate2d_shape", "np_debug_conv2d_last_path", "np_debug_conv2d_staged_path"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert len(_lib.PROTOTYPES["np_correlate2d"][1]) == 11 and len(_lib.PROTOTYPES["np_correlate2d_shape"][1]) == 7


def test_the_header_states_the_fine_print():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    for phrase in ("every tap is multiplied and added", "fixed order", "boundary once per cell", "bit-identical from run to run",
                   "must not overlap a or b", "All extents >= 1", "beyond INT_MAX"):
        assert phrase.lower() in raw.lower(), phrase


def test_bad_arguments_are_refused_before_any_device_work():
    """np_correlate2d checks its arguments before it initialises a device: NP_ERR_INVALID with a message, with or without a GPU"""
    from numpower_amd import _lib
    lib = _lib.load()
    lib.np_last_error.restype = C.c_char_p
    p = 4096          # never dereferenced: every call below is refused
    for args, msg in (((None, 4, 4, p, 2, 2, 1, 0), b"null pointer"), ((p, 4, 4, None, 2, 2, 1, 0), b"null pointer"),
                      ((p, 4, 4, p, 2, 2, 3, 0), b"unknown mode 3"), ((p, 4, 4, p, 2, 2, 1, 2), b"unknown boundary 2"),
                      ((p, 4, 4, p, 2, 2, 1, 12), b"unknown boundary 12"), ((p, 0, 4, p, 2, 2, 1, 0), b"at least 1"),
                      ((p, 4, 1, p, 2, 2, 0, 0), b"For 'valid' mode"), ((p, 2 ** 31, 1, p, 1, 1, 1, 0), b"int shape")):
        assert lib.np_correlate2d(*args, C.c_float(0.0), 0, p) == -1, args
        assert msg in lib.np_last_error(), (args, lib.np_last_error())
    assert lib.np_correlate2d(p, 4, 4, p, 2, 2, 1, 0, C.c_float(0.0), 0, None) == -1
    assert lib.np_debug_conv2d_last_path(None) == -1
    path = C.c_int(-1)
    assert lib.np_debug_conv2d_last_path(C.byref(path)) == 0 and path.value in (0, 1, 2)
    assert lib.np_debug_conv2d_staged_path(1) == 0


def test_host_function_has_the_reference_signature():
    from numpower_amd import ndarray
    assert PROTO in _header("numpower_host.h")
    assert hasattr(ndarray._load_host(), "NDArray_Correlate2D")
    glue = _header("hip_signal.h", "ext")
    assert ("struct NDArray *NPH_Correlate2D(struct NDArray *a, struct NDArray *b, int mode, int boundary, "
            "struct NDArray *fill_value, int flip);") in glue
    assert "#define NPH_SIGNAL_TAKES(a, b) (NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU && NDArray_DEVICE(b) == NDARRAY_DEVICE_GPU)" in glue


@pytest.mark.skipif(not (REF / "src" / "ndmath" / "signal.h").exists(), reason="needs a NumPower checkout to compare with")
def test_the_signature_is_the_one_the_reference_declares():
    ref = re.sub(r"\s+", "", (REF / "src" / "ndmath" / "signal.h").read_text())
    assert PROTO.replace(" ", "") in ref
    for name, value in (("FULL", 2), ("SAME", 1), ("VALID", 0), ("CIRCULAR", 8), ("REFLECT", 4), ("PAD", 0)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), (REF / "src" / "ndmath" / "signal.h").read_text()), name


def test_hip_signal_uses_only_what_the_reference_headers_declare():
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "ext" / "hip_signal.c").read_text(), flags=re.S)
    used = sorted(set(re.findall(r"\b(NDArray_\w+|NDARRAY_\w+)\b", src)))
    ref = json.loads((ROOT / "tests" / "golden" / "reference_abi.json").read_text())
    ours = (ROOT / "include" / "numpower_host.h").read_text()
    assert "NDArray_Empty" in used and "NDArray_FREE" in used
    for name in used:
        assert name in ref["ndarray_header_names"], name
        assert re.search(r"#define\s+%s\b|\b%s\s*\(" % (name, name), ours), name
    for message in ("NDArray::correlate2d inputs must be both 2-D arrays", "fillValue must be a scalar or an array with one element.",
                    "invalid mode.", "correlate2d not implemented for GPU computation.",
                    "For 'valid' mode, one input must be at least as large as the other in every dimension"):
        assert '"%s"' % message in src, message
        if (REF / "src" / "ndmath" / "signal.c").exists():
            assert message in (REF / "src" / "ndmath" / "signal.c").read_text(), message
    assert "`hip_signal.c`" in (ROOT / "ext" / "README.md").read_text()
    assert "hip_signal.c" in (ROOT / "ext" / "config.m4").read_text()


def test_shape_device_and_fill_messages_on_cpu_arrays():
    from numpower_amd.ndarray import NDArray, Error
    a, b = NDArray.array(np.ones((6, 8), np.float32)), NDArray.array(np.ones((3, 3), np.float32))
    for call, msg in ((lambda: NDArray.correlate2d(a, NDArray.array([1.0, 2.0]), "same", "fill"), "NDArray::correlate2d inputs must be both 2-D arrays"),
                      (lambda: NDArray.convolve2d(NDArray.array(np.ones((2, 2, 2), np.float32)), b, "full", "wrap"),
                       "NDArray::correlate2d inputs must be both 2-D arrays"),
                      (lambda: NDArray.correlate2d(a, NDArray.array(np.ones((2, 9), np.float32)), "valid", "fill"),
                       "For 'valid' mode, one input must be at least as large as the other in every dimension"),
                      (lambda: NDArray.convolve2d(a, b, "same", "fill", NDArray.array([1.0, 2.0])),
                       "fillValue must be a scalar or an array with one element.")):
        with pytest.raises(Error) as e:
            call()
        assert str(e.value) == msg
    for call in (lambda: NDArray.convolve2d(a, b, "same", "fill"), lambda: NDArray.correlate2d(a, b, "valid", "symm", 2.0),
                 lambda: NDArray.correlate2d(a, b, "full", "wrap", NDArray.array([3.0]))):
        with pytest.raises(Error, match="only computes on the GPU"):
            call()
    # the first letter picks the flag as in the PHP methods; an empty string or an unknown letter is an Error here (a deviation)
    for mode, boundary, msg in (("", "fill", "mode must begin with"), ("x", "fill", "mode must begin with"), ("same", "", "boundary must begin with"),
                                ("same", "reflect", "boundary must begin with"), (None, "fill", "mode must begin with")):
        with pytest.raises(Error, match=msg):
            NDArray.convolve2d(a, b, mode, boundary)
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.convolve2d(a, b, "s", "wrapped")
    from numpower_amd import ndarray
    h = ndarray._load_host()
    assert not h.NDArray_Correlate2D(a._p, b._p, 7, 0, None, 0) and h.numpower_host_last_error() == b"invalid mode."
    h.numpower_host_clear_error()


def test_the_edit_is_a_list_of_its_own_and_the_77_stay_77(tmp_path):
    tool = _tool()
    assert isinstance(tool.SIGNAL_EDITS, list) and len(tool.SIGNAL_EDITS) == 2           # the include, the early-out
    assert not any(e in tool.EDITS for e in tool.SIGNAL_EDITS)
    assert len(tool.EDITS) == 77
    include, edit = tool.SIGNAL_EDITS
    assert include.what == "signal.c:41: <hip_signal.h>" and include.after and include.new == "#include <hip_signal.h>"
    assert edit.what == WHAT and edit.after and edit.context and not edit.guard and edit.file == "src/ndmath/signal.c"
    assert edit.new.strip().endswith(CALL)
    assert not any(e is edit for _, e in tool.FAST_BINARY)
    assert "/* %s */" % WHAT not in tool.snippet_check_source() and "hip_signal.h" not in tool.snippet_check_source()   # the old unit is what it was
    src = tool.snippet_check_source(tool.SIGNAL_EDITS)
    assert "/* %s */" % WHAT in src and CALL in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    for mutated in (src.replace("fill_value, flip);", "flip, fill_value);"), src.replace("NPH_Correlate2D(a, b, mode,", "NPH_Correlate2D(a, mode,")):
        assert mutated != src
        bad = tmp_path / "bad.c"
        bad.write_text(mutated)
        assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


@pytest.mark.skipif(not (REF / "numpower.c").exists(), reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_puts_the_early_out_in_front_of_the_throw(tmp_path):
    tool = _tool()
    plain = tool.apply(REF, tmp_path / "plain")
    assert len(plain) == 77 == len(tool.EDITS) and plain.extra == {}
    assert (tmp_path / "plain" / "src" / "ndmath" / "signal.c").read_text() == (REF / "src" / "ndmath" / "signal.c").read_text()
    out = tmp_path / "numpower"
    applied = tool.apply(REF, out, extra=tool.SIGNAL_EDITS)
    assert len(applied) == 77 and WHAT not in applied
    assert applied.extra == {"signal.c:41: <hip_signal.h>": 1, WHAT: 1}
    assert tool.check_tree(out, raw=True) == []
    text = (out / "src" / "ndmath" / "signal.c").read_text()
    assert "#include \"../initializers.h\"\n#ifdef HAVE_NP_HIP\n#include <hip_signal.h>\n#endif\n" in text
    body = text[text.index("NDArray_Correlate2D(NDArray *a, NDArray *b, int mode, int boundary, NDArray* fill_value, int flip) {"):]
    assert body.count(CALL) == 1
    assert body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_SIGNAL_TAKES(a, b)") < body.index("#endif") < \
        body.index("correlate2d not implemented for GPU computation.") < body.index("_inputs_swap(mode, a, b)")
    # nothing of the reference is replaced: without the two inserted blocks the file is the reference's
    stripped = re.sub(r"#ifdef HAVE_NP_HIP\n.*?#endif\n", "", text, flags=re.S)
    assert stripped == (REF / "src" / "ndmath" / "signal.c").read_text()
    assert (out / "src" / "hip" / "hip_signal.c").read_bytes() == (ROOT / "ext" / "hip_signal.c").read_bytes()
    assert (out / "src" / "hip" / "hip_signal.h").exists() and "src/hip/hip_signal.c" in (out / "config.m4").read_text()
    # numpower.c keeps passing NULL for fill_value: no edit there
    assert "NDArray_Correlate2D(nda, ndb, imode, iboundary, NULL, 1)" in (out / "numpower.c").read_text()


@pytest.mark.skipif(not (REF / "numpower.c").exists(), reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_main_applies_the_signal_edits_unless_told_not_to(tmp_path):
    tool = str(ROOT / "tools" / "apply_with_hip.py")
    proc = subprocess.run([sys.executable, tool, str(REF), str(tmp_path / "with")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert "applied x1  %s" % WHAT in proc.stdout and "79 edits in" in proc.stdout
    assert CALL in (tmp_path / "with" / "src" / "ndmath" / "signal.c").read_text()
    proc = subprocess.run([sys.executable, tool, "--no-signal", str(REF), str(tmp_path / "without")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert WHAT not in proc.stdout and "77 edits in" in proc.stdout
    assert "NPH_" not in (tmp_path / "without" / "src" / "ndmath" / "signal.c").read_text()


def test_signal_bodies_cpu_operands_reach_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "signal_bodies"
    tool = _tool()
    gen = tool.signal_program_source()
    for line in tool.SIGNAL_EDITS[-1].new.split("\n"):
        assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "signal_bodies cpu: 1 calls reached the reference's own code, 0 failures" in proc.stdout


def test_the_feature_stays_out_of_the_translation_units_the_null_device_build_compiles():
    """tests/test_host_sanitizers_cpu.py builds numpower_host.cpp against the null device (tests/null_device), which has no
    stencil.  The host code therefore lives in numpower_signal.cpp, which that build leaves out (the reason
    tests/test_svd_glue_cpu.py gives for the SVD): neither numpower_host.cpp nor the null device may name the feature."""
    for path in sorted((ROOT / "tests" / "null_device").glob("*")):
        if path.is_file():
            text = path.read_text(errors="replace")
            assert "correlate2d" not in text.lower() and "hip_signal" not in text, path
    host = (ROOT / "numpower_amd" / "host" / "numpower_host.cpp").read_text()
    assert "np_correlate2d" not in host and "NDArray_Correlate2D" not in host and "hip_signal" not in host
    assert "NDArray_Correlate2D" in (ROOT / "numpower_amd" / "host" / "numpower_signal.cpp").read_text()
    assert "np_signal.hip" in (ROOT / "numpower_amd" / "build.py").read_text()
