"""CPU-tier checks of the Cholesky factorization's boundary (np_cholesky.hip, ext/hip_linalg.c, host/numpower_linalg.cpp):
np_potrf / np_cholesky are declared, prototyped and exported and refuse null arguments; NDArray_Cholesky has the
reference's signature and messages; the --with-hip early-out applies once, in front of the reference's GPU throw."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT = "linalg.c:1057 NDArray_Cholesky: GPU early-out"
GCC_CHECK = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-I", str(ROOT / "include"), "-I", str(ROOT / "ext")]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def _tool():
    sys.path.insert(0, str(ROOT / "tools"))
    import apply_with_hip
    return apply_with_hip


def _function(text):
    """NDArray_Cholesky from its opening line to its closing brace (the last function of the file)"""
    body = text[text.index("NDArray_Cholesky(NDArray *a) {"):]
    return body[:re.search(r"\n}[ \t]*(\n|$)", body).start()]


def test_abi_is_declared_prototyped_and_exported():
    from numpower_amd import _lib
    text = re.sub(r"\s+", " ", _header("np_hip.h"))
    lib = _lib.load()
    assert "int np_potrf(float *a, size_t n, int *info);" in text
    assert "int np_cholesky(const float *a, size_t n, float *out, int *info_host);" in text
    for n in ("np_potrf", "np_cholesky"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert len(_lib.PROTOTYPES["np_potrf"][1]) == 3 and len(_lib.PROTOTYPES["np_cholesky"][1]) == 4


def test_null_arguments_are_refused_before_any_device_work():
    from numpower_amd import _lib
    lib = _lib.load()
    info = C.c_int()
    # argument checks come after np_init: without a device they report that instead; either way nothing runs
    for rc in (lib.np_potrf(None, 4, None), lib.np_cholesky(None, 4, None, C.byref(info)), lib.np_cholesky(None, 4, None, None)):
        assert rc != _lib.NP_OK


def test_host_function_has_the_reference_signature():
    from numpower_amd import ndarray
    text = re.sub(r"\s+", " ", _header("numpower_host.h"))
    assert "NDArray *NDArray_Cholesky(NDArray *a);" in text                       # src/ndmath/linalg.h of the reference
    assert hasattr(ndarray._load_host(), "NDArray_Cholesky")
    glue = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / "ext" / "hip_linalg.h").read_text(), flags=re.S))
    assert "struct NDArray *NPH_Cholesky(struct NDArray *a);" in glue


def test_shape_errors_and_the_cpu_refusal():
    from numpower_amd.ndarray import NDArray, Error
    with pytest.raises(Error) as e:
        NDArray.cholesky(NDArray.array([1.0, 2.0]))
    assert str(e.value) == "NDArray_Cholesky: $a must be a square matrix."
    with pytest.raises(Error) as e:
        NDArray.cholesky(NDArray.array(np.ones((2, 3), np.float32)))
    assert str(e.value) == "NDArray_Cholesky: $a must be a square matrix."
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.cholesky(NDArray.array(np.eye(3, dtype=np.float32)))


def test_the_glue_raises_the_reference_messages():
    src = (ROOT / "ext" / "hip_linalg.c").read_text()
    body = src[src.index("NDArray *NPH_Cholesky(NDArray *a) {"):].replace('" "', "")   # adjacent literals are one string
    assert '"Error calculating the cholesky decomposition. (Is $a not positive definite?)"' in body
    assert '"NDArray_Cholesky: $a must be a square matrix."' in body and "np_cholesky(" in body


def test_the_edit_is_a_list_of_its_own_and_passes_the_snippet_check(tmp_path):
    tool = _tool()
    assert len(tool.LINALG_EDITS) == 5
    assert len(tool.CHOLESKY_EDITS) == 1 and all(e in tool.EDITS for e in tool.CHOLESKY_EDITS)
    (edit,) = tool.CHOLESKY_EDITS
    assert edit.what == WHAT and edit.after and edit.context and not edit.guard
    assert edit not in tool.LINALG_EDITS and not any(e is edit for _, e in tool.FAST_BINARY)
    assert "NPH_LINALG_TAKES(a)" in edit.new and "return NPH_Cholesky(a);" in edit.new
    src = tool.snippet_check_source()
    assert "/* %s */" % WHAT in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    bad_src = src.replace("return NPH_Cholesky(a);", "return NPH_Cholesky(a, a);")
    assert bad_src != src
    bad = tmp_path / "bad.c"
    bad.write_text(bad_src)
    assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_cholesky_bodies_cpu_operand_reaches_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "cholesky_bodies"
    tool = _tool()
    gen = tool.cholesky_program_source()
    for line in tool.CHOLESKY_EDITS[0].new.split("\n"):
        assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "cholesky_bodies cpu: 1 calls reached the reference's own code, 0 failures" in proc.stdout


@pytest.mark.skipif(not (REF / "numpower.c").exists(), reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_device_cholesky(tmp_path):
    tool = _tool()
    out = tmp_path / "numpower"
    applied = tool.apply(REF, out)
    assert applied[WHAT] == 1
    assert len(applied) == len(tool.EDITS)
    text = (out / "src" / "ndmath" / "linalg.c").read_text()
    body = _function(text)
    assert body.count("return NPH_Cholesky(a);") == 1
    assert body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_LINALG_TAKES(a)") < body.index("return NPH_Cholesky(a);") < \
        body.index("#endif") < body.index("ndarray::cholesky not implemented for GPU") < body.index("LAPACKE_spotrf")
    before = (REF / "src" / "ndmath" / "linalg.c").read_text()
    ref_body = _function(before)
    inserted = body[body.index("#ifdef HAVE_NP_HIP"):body.index("#endif") + len("#endif\n")]
    assert body.replace(inserted, "") == ref_body                                  # nothing of the reference is replaced
