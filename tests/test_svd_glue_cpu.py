"""CPU-tier checks of the SVD's boundary (np_jacobi.hip, ext/hip_linalg.c, host/numpower_linalg.cpp): np_svd / np_svdvals
and the sweep-cap knob are declared, prototyped and exported and refuse null arguments; NDArray_SVD / MatrixRank / Norm /
Cond have the reference's signatures and messages; the --with-hip early-out is one edit in a list of its own, at the top of
NDArray_SVD; svd_bodies shows a CPU operand reaching the reference's own code."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT = "linalg.c:112 NDArray_SVD: GPU early-out"
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
    assert "int np_svd(const float *a, size_t m, size_t n, float *u, float *s, float *vt, int *info_host);" in text
    assert "int np_svdvals(const float *a, size_t m, size_t n, float *s, int *info_host);" in text
    assert "int np_debug_svd_max_sweeps(int sweeps);" in _header("np_hip_debug.h")
    for n in ("np_svd", "np_svdvals", "np_debug_svd_max_sweeps", "np_debug_svd_last_sweeps", "np_debug_svd_small_path"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert len(_lib.PROTOTYPES["np_svd"][1]) == 7 and len(_lib.PROTOTYPES["np_svdvals"][1]) == 5


def test_the_header_states_the_fine_print():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    for phrase in ("signs are not normalised", "written as +0.0f", "non-finite input", "m, n <= 65536", "Scratch:",
                   "bit-identical from run to run"):
        assert phrase.lower() in raw.lower(), phrase


def test_null_arguments_are_refused_before_any_device_work():
    from numpower_amd import _lib
    lib = _lib.load()
    info = C.c_int()
    # argument checks come after np_init: without a device they report that instead; either way nothing runs
    for rc in (lib.np_svd(None, 4, 4, None, None, None, C.byref(info)), lib.np_svd(None, 4, 4, None, None, None, None),
               lib.np_svdvals(None, 4, 4, None, C.byref(info)), lib.np_svdvals(None, 4, 4, None, None)):
        assert rc != _lib.NP_OK
    assert lib.np_debug_svd_max_sweeps(-1) != _lib.NP_OK
    assert lib.np_debug_svd_max_sweeps(0) == _lib.NP_OK


def test_host_functions_have_the_reference_signatures():
    from numpower_amd import ndarray
    text = _header("numpower_host.h")
    for proto in ("NDArray **NDArray_SVD(NDArray *target);", "NDArray *NDArray_MatrixRank(NDArray *target, float *tol);",
                  "NDArray *NDArray_Norm(NDArray *target, int type);", "NDArray *NDArray_Cond(NDArray *a);"):
        assert proto in text, proto                                                # src/ndmath/linalg.h of the reference
    h = ndarray._load_host()
    for name in ("NDArray_SVD", "NDArray_MatrixRank", "NDArray_Norm", "NDArray_Cond"):
        assert hasattr(h, name)
    assert "struct NDArray **NPH_SVD(struct NDArray *a);" in _header("hip_linalg.h", "ext")


@pytest.mark.skipif(not (REF / "src" / "ndmath" / "linalg.h").exists(), reason="needs a NumPower checkout to compare with")
def test_the_signatures_are_the_ones_the_reference_declares():
    ref = re.sub(r"\s+", " ", (REF / "src" / "ndmath" / "linalg.h").read_text()).replace("* ", " *").replace("  ", " ")
    for proto in ("NDArray **NDArray_SVD(NDArray *target);", "NDArray *NDArray_MatrixRank(NDArray *target, float *tol);",
                  "NDArray *NDArray_Norm(NDArray *target, int type);", "NDArray *NDArray_Cond(NDArray *a);"):
        assert proto.replace(" ", "") in ref.replace(" ", ""), proto


def test_shape_errors_and_the_cpu_refusal():
    from numpower_amd.ndarray import NDArray, Error
    with pytest.raises(Error) as e:
        NDArray.svd(NDArray.array([1.0, 2.0]))
    assert str(e.value) == "Array must be at least two-dimensional"
    with pytest.raises(Error, match="only two-dimensional"):
        NDArray.svd(NDArray.array(np.ones((2, 2, 2), np.float32)))
    for call in (NDArray.svd, NDArray.matrix_rank, NDArray.norm, NDArray.cond):
        with pytest.raises(Error, match="only computes on the GPU"):
            call(NDArray.array(np.eye(3, dtype=np.float32)))
    with pytest.raises(Error) as e:
        NDArray.norm(NDArray.array(np.eye(3, dtype=np.float32)), 3)
    assert str(e.value) == "NDArray_Norm: The provided norm `3` is invalid"
    with pytest.raises(Error, match="norm `1` is not available for GPU arrays"):
        NDArray.norm(NDArray.array(np.eye(3, dtype=np.float32)), 1)


def test_the_glue_raises_the_reference_message_and_declares_the_reference_shapes():
    src = (ROOT / "ext" / "hip_linalg.c").read_text()
    body = src[src.index("NDArray **NPH_SVD(NDArray *a) {"):]
    assert '"Array must be at least two-dimensional"' in body and "np_svd(" in body
    assert "zeros_on_gpu(2, m, m)" in body and "zeros_on_gpu(1, k, 0)" in body and "zeros_on_gpu(2, n, n)" in body


def test_the_stub_of_the_cuda_entry_point_keeps_its_prototype():
    text = (ROOT / "ext" / "hip_math.c").read_text()
    assert "cuda_svd_float(" in text and 'not_available("svd")' in text


def test_the_edit_is_a_list_of_its_own_and_passes_the_snippet_check(tmp_path):
    tool = _tool()
    assert len(tool.LINALG_EDITS) == 5 and len(tool.CHOLESKY_EDITS) == 1
    assert len(tool.SVD_EDITS) == 1 and all(e in tool.EDITS for e in tool.SVD_EDITS)
    assert len(tool.EDITS) == 77
    (edit,) = tool.SVD_EDITS
    assert edit.what == WHAT and edit.after and edit.context and not edit.guard
    assert edit not in tool.LINALG_EDITS + tool.CHOLESKY_EDITS and not any(e is edit for _, e in tool.FAST_BINARY)
    assert "NPH_LINALG_TAKES(target)" in edit.new and "return NPH_SVD(target);" in edit.new
    src = tool.snippet_check_source()
    assert "/* %s */" % WHAT in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    bad_src = src.replace("return NPH_SVD(target);", "return NPH_SVD(target, target);")
    assert bad_src != src
    bad = tmp_path / "bad.c"
    bad.write_text(bad_src)
    assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_svd_bodies_cpu_operand_reaches_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "svd_bodies"
    tool = _tool()
    gen = tool.svd_program_source()
    for line in tool.SVD_EDITS[0].new.split("\n"):
        assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "svd_bodies cpu: 1 calls reached the reference's own code, 0 failures" in proc.stdout


def test_the_svd_stays_out_of_the_translation_unit_the_null_device_build_compiles():
    """tests/test_host_sanitizers_cpu.py builds numpower_host.cpp against the null device (tests/null_device), which has no
    factorizations.  The SVD's host code therefore lives in numpower_linalg.cpp, which that build leaves out: this checks that
    neither numpower_host.cpp nor the null device names it, which is what keeps that build linking.  (It links nothing itself,
    and the SVD's host code does not run under the sanitizers.)"""
    null = (ROOT / "tests" / "null_device" / "null_device.c").read_text()
    assert "np_svd" not in null
    host = (ROOT / "numpower_amd" / "host" / "numpower_host.cpp").read_text()
    assert "np_svd" not in host and "NDArray_SVD" not in host
    assert "NDArray_SVD" in (ROOT / "numpower_amd" / "host" / "numpower_linalg.cpp").read_text()


@pytest.mark.skipif(not (REF / "numpower.c").exists(), reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_device_svd(tmp_path):
    tool = _tool()
    out = tmp_path / "numpower"
    applied = tool.apply(REF, out)
    assert applied[WHAT] == 1
    assert len(applied) == len(tool.EDITS)
    text = (out / "src" / "ndmath" / "linalg.c").read_text()
    body = text[text.index("NDArray_SVD(NDArray *target) {"):]
    body = body[:body.index("\n}\n")]
    assert body.count("return NPH_SVD(target);") == 1
    assert body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_LINALG_TAKES(target)") < body.index("return NPH_SVD(target);") < \
        body.index("#endif") < body.index("Array must be at least two-dimensional") < body.index("computeSVDFloat(")
    before = (REF / "src" / "ndmath" / "linalg.c").read_text()
    ref_body = before[before.index("NDArray_SVD(NDArray *target) {"):]
    ref_body = ref_body[:ref_body.index("\n}\n")]
    inserted = body[body.index("#ifdef HAVE_NP_HIP"):body.index("#endif") + len("#endif\n")]
    assert body.replace(inserted, "", 1).count("NPH_") == 0      # what is left is the reference's text and the earlier copy edit
