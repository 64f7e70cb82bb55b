"""CPU-tier checks of the LU's boundary (np_lu.hip, host/numpower_linalg.cpp): the new C-ABI names are declared,
prototyped and exported, the four host functions are declared with the reference's signatures (linalg.h) and
exported, and their argument checks raise the reference's messages without touching a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW_ABI = ["np_getrf", "np_getrs", "np_det", "np_inverse", "np_solve", "np_lu"]
# src/ndmath/linalg.h of the reference
HOST_SIGNATURES = {
    "NDArray_Det": "NDArray *NDArray_Det(NDArray *a);",
    "NDArray_Inverse": "NDArray *NDArray_Inverse(NDArray *target);",
    "NDArray_LU": "NDArray **NDArray_LU(NDArray *target);",
    "NDArray_Solve": "NDArray *NDArray_Solve(NDArray *a, NDArray *b);",
}


def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def test_lu_abi_is_declared_prototyped_and_exported():
    from numpower_amd import _lib
    text = _header("np_hip.h")
    lib = _lib.load()
    for n in NEW_ABI:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in _lib.PROTOTYPES, n
        assert hasattr(lib, n), n


def test_host_functions_have_the_reference_signatures():
    from numpower_amd import ndarray
    text = re.sub(r"\s+", " ", _header("numpower_host.h"))
    h = ndarray._load_host()
    for name, sig in HOST_SIGNATURES.items():
        assert sig in text, sig
        assert hasattr(h, name), name


def test_null_arguments_are_refused_before_any_device_work():
    from numpower_amd import _lib
    lib = _lib.load()
    info = C.c_int()
    # argument checks come after np_init: without a device they report that instead; either way nothing runs
    for rc in (lib.np_getrf(None, 4, None, None), lib.np_getrs(None, None, 4, 1, None), lib.np_det(None, 4, None),
               lib.np_inverse(None, 4, None, C.byref(info)), lib.np_solve(None, None, 4, 1, None, C.byref(info)),
               lib.np_lu(None, 4, None, None, None)):
        assert rc != _lib.NP_OK


@pytest.mark.parametrize("method", ["det", "inv", "lu"])
def test_shape_errors_on_cpu_arrays(method):
    from numpower_amd.ndarray import NDArray, Error
    fn = getattr(NDArray, method)
    with pytest.raises(Error, match="Array must be at least two-dimensional"):
        fn(NDArray.array([1.0, 2.0]))
    with pytest.raises(Error, match="Array must be square"):
        fn(NDArray.array(np.ones((2, 3), np.float32)))
    with pytest.raises(Error, match="only computes on the GPU"):
        fn(NDArray.array(np.eye(3, dtype=np.float32)))


def test_solve_argument_checks_on_cpu_arrays():
    from numpower_amd.ndarray import NDArray, Error
    a = NDArray.array(np.eye(3, dtype=np.float32))
    with pytest.raises(Error, match="Incompatible shapes"):
        NDArray.solve(a, NDArray.array(np.ones((4, 1), np.float32)))
    with pytest.raises(Error, match="Incompatible shapes"):
        NDArray.solve(a, NDArray.array([1.0, 2.0, 3.0]))
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.solve(a, NDArray.array(np.ones((3, 2), np.float32)))


def test_cuda_stubs_still_raise():
    C.CDLL(str(ROOT / "numpower_amd" / "lib" / "libnp_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(str(ROOT / "numpower_amd" / "lib" / "libnp_hipmath.so"))
    lib.np_ext_last_error.restype = C.c_char_p
    lib.np_ext_clear_error()
    assert lib.cuda_det_float(None, None, 3) == 0
    assert b"not available" in lib.np_ext_last_error()
    lib.np_ext_clear_error()
    lib.cuda_matrix_float_inverse(None, 3)
    assert b"not available" in lib.np_ext_last_error()


# ---- the --with-hip early-outs (tools/apply_with_hip.py section 2b, ext/hip_linalg.c) ---------------------------------

REF = Path("/root/reference")
GCC_CHECK = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-I", str(ROOT / "include"), "-I", str(ROOT / "ext")]


def _tool():
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import apply_with_hip
    return apply_with_hip


def test_linalg_edits_pass_the_snippet_check_and_a_broken_one_is_refused(tmp_path):
    import subprocess
    tool = _tool()
    assert len(tool.LINALG_EDITS) == 5 and all(e in tool.EDITS for e in tool.LINALG_EDITS)
    early = [e for e in tool.LINALG_EDITS if e.what.endswith("GPU early-out")]
    assert len(early) == 4 and all(e.context and e.after for e in early)
    assert not any(e in early for _, e in tool.FAST_BINARY)       # their own program, not fast_path_bodies
    src = tool.snippet_check_source()
    for e in early:
        assert "/* %s */" % e.what in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    bad_src = src.replace("if (!NPH_LU(target, p, l, u)) {", "if (!NPH_LU(p, target, l)) {")
    assert bad_src != src
    bad = tmp_path / "bad.c"
    bad.write_text(bad_src)
    assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_linalg_bodies_cpu_operands_reach_the_reference_code():
    import subprocess
    exe = ROOT / "numpower_amd" / "lib" / "linalg_bodies"
    gen = _tool().linalg_program_source()
    for e in _tool().LINALG_EDITS[1:]:
        assert e.new.strip().split("\n")[-2].strip() in gen, e.what
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "4 calls reached the reference's own code, 0 failures" in proc.stdout


def test_hip_linalg_uses_only_what_the_reference_headers_declare():
    import json
    src = re.sub(r"/\*.*?\*/", "", (ROOT / "ext" / "hip_linalg.c").read_text(), flags=re.S)
    used = sorted(set(re.findall(r"\b(NDArray_\w+|NDARRAY_\w+)\b", src)))
    ref = json.loads((ROOT / "tests" / "golden" / "reference_abi.json").read_text())
    ours = (ROOT / "include" / "numpower_host.h").read_text()
    for name in used:
        assert name in ref["ndarray_header_names"], name
        assert re.search(r"#define\s+%s\b|\b%s\s*\(" % (name, name), ours), name


@pytest.mark.skipif(not (REF / "numpower.c").exists(), reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_lu(tmp_path):
    tool = _tool()
    out = tmp_path / "numpower"
    applied = tool.apply(REF, out)
    for e in tool.LINALG_EDITS:
        assert applied[e.what] == 1, e.what
    text = (out / "src" / "ndmath" / "linalg.c").read_text()
    assert "#include <hip_linalg.h>" in text
    for fn, call in (("NDArray_Det(NDArray *a) {", "return NPH_Det(a);"),
                     ("NDArray_Inverse(NDArray* target) {", "return NPH_Inverse(target);"),
                     ("NDArray_LU(NDArray* target) {", "if (!NPH_LU(target, p, l, u)) {"),
                     ("NDArray_Solve(NDArray *a, NDArray *b) {", "return NPH_Solve(a, b);")):
        body = text[text.index(fn):]
        body = body[:body.index("\n}\n")]
        assert call in body, fn
    solve = text[text.index("NDArray_Solve(NDArray *a, NDArray *b) {"):]
    assert solve.index("Both NDArray must be in the same device.") < solve.index("NPH_Solve") < \
        solve.index("ndarray::solve not implemented for GPU")
    lu = text[text.index("NDArray_LU(NDArray* target) {"):]
    assert lu.index("Array must be square") < lu.index("NPH_LU") < lu.index("matrixFloatLU")
    assert (out / "src" / "hip" / "hip_linalg.c").exists() and "src/hip/hip_linalg.c" in (out / "config.m4").read_text()
