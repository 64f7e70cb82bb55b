"""CPU-tier checks of the symmetric eigensolver's boundary (np_jacobi.hip, ext/hip_linalg.c, host/numpower_linalg.cpp): np_eigh /
np_eigvalsh / np_symmetry_mismatch and the three debug knobs are declared, prototyped and exported and refuse null arguments;
NDArray_Eig has the reference's signature and message; the --with-hip early-out is one edit in a list of its own that is NOT part
of EDITS and reaches a tree only under --eig; eig_bodies shows a CPU operand reaching the reference's own code."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT = "linalg.c:796-799 NDArray_Eig: GPU early-out"
GCC_CHECK = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-I", str(ROOT / "include"), "-I", str(ROOT / "ext")]
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
    assert "int np_eigh(const float *a, size_t n, float *w, float *v, int *info_host);" in text
    assert "int np_eigvalsh(const float *a, size_t n, float *w, int *info_host);" in text
    assert "int np_symmetry_mismatch(const float *a, size_t n, int *host_any);" in text
    debug = _header("np_hip_debug.h")
    for proto in ("int np_debug_eigh_max_sweeps(int sweeps);", "int np_debug_eigh_last_sweeps(int *host_sweeps);",
                  "int np_debug_eigh_small_path(int on);"):
        assert proto in debug, proto
    for n in ("np_eigh", "np_eigvalsh", "np_symmetry_mismatch", "np_debug_eigh_max_sweeps", "np_debug_eigh_last_sweeps",
              "np_debug_eigh_small_path"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert len(_lib.PROTOTYPES["np_eigh"][1]) == 5 and len(_lib.PROTOTYPES["np_eigvalsh"][1]) == 4


def test_the_header_states_the_fine_print():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    block = raw[raw.index("symmetric eigensolver (np_jacobi.hip"):raw.index("int np_eigh(")]
    for phrase in ("only the lower triangle", "ssyevd('L')", "eigenvalues ascending", "ties kept in the order of their diagonal position",
                   "column j is the eigenvector of w[j]", "not renormalised", "the first such in index order, is positive",
                   "same w bit for bit", "the sweep cap (60)", "clipped to INT_MAX", "the largest |entry| of the lower triangle",
                   "accuracy class", "not LAPACK's ssyevd", "non-finite input", "n <= 64 is ONE launch", "n <= 65536", "Scratch:",
                   "bit-identical from run to run", "Outputs must not overlap a", "crossover"):
        assert phrase.lower() in block.lower(), phrase


def test_null_arguments_are_refused_before_any_device_work():
    from numpower_amd import _lib
    lib = _lib.load()
    info = C.c_int()
    # argument checks come after np_init: without a device they report that instead; either way nothing runs
    for rc in (lib.np_eigh(None, 4, None, None, C.byref(info)), lib.np_eigh(None, 4, None, None, None),
               lib.np_eigvalsh(None, 4, None, C.byref(info)), lib.np_eigvalsh(None, 4, None, None),
               lib.np_symmetry_mismatch(None, 4, C.byref(info)), lib.np_symmetry_mismatch(None, 4, None)):
        assert rc != _lib.NP_OK
    assert lib.np_debug_eigh_max_sweeps(-1) != _lib.NP_OK
    assert lib.np_debug_eigh_max_sweeps(0) == _lib.NP_OK
    assert lib.np_debug_eigh_last_sweeps(None) != _lib.NP_OK
    assert lib.np_debug_eigh_small_path(1) == _lib.NP_OK


def test_host_function_has_the_reference_signature():
    from numpower_amd import ndarray
    assert "NDArray **NDArray_Eig(NDArray *a);" in _header("numpower_host.h")      # src/ndmath/linalg.h of the reference
    assert hasattr(ndarray._load_host(), "NDArray_Eig")
    assert "struct NDArray **NPH_Eig(struct NDArray *a);" in _header("hip_linalg.h", "ext")
    assert callable(ndarray.NDArray.eig)


@pytest.mark.skipif(not (REF / "src" / "ndmath" / "linalg.h").exists(), reason="needs a NumPower checkout to compare with")
def test_the_signature_is_the_one_the_reference_declares():
    ref = re.sub(r"\s+", "", (REF / "src" / "ndmath" / "linalg.h").read_text())
    assert "NDArray**NDArray_Eig(NDArray*a);" in ref


def test_shape_errors_and_the_cpu_refusal():
    from numpower_amd.ndarray import NDArray, Error
    for bad in (np.ones(3, np.float32), np.ones((2, 3), np.float32), np.ones((2, 2, 2), np.float32)):
        with pytest.raises(Error) as e:
            NDArray.eig(NDArray.array(bad))
        assert str(e.value) == "Error: Input matrix is not square.\n"
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.eig(NDArray.array(np.eye(3, dtype=np.float32)))


def test_the_glue_raises_the_reference_message_and_declares_the_reference_shapes():
    src = (ROOT / "ext" / "hip_linalg.c").read_text()
    body = src[src.index("NDArray **NPH_Eig(NDArray *a) {"):]
    assert '"Error: Input matrix is not square.\\n"' in body and "np_eigh(" in body and "np_symmetry_mismatch(" in body
    assert body.index("np_symmetry_mismatch(") < body.index("zeros_on_gpu(") < body.index("np_eigh(")
    assert "zeros_on_gpu(1, n, 0)" in body and "zeros_on_gpu(2, n, n)" in body
    assert "symmetric eigensolver" in body and "->cpu()" in body and "sweep cap" in body
    assert body.index("rtns[0] = w;") < body.index("rtns[1] = v;")


def test_the_edit_is_a_list_of_its_own_outside_edits_and_passes_the_snippet_check(tmp_path):
    tool = _tool()
    assert len(tool.EIG_EDITS) == 1 and not any(e in tool.EDITS for e in tool.EIG_EDITS)
    assert not any(e in tool.SIGNAL_EDITS for e in tool.EIG_EDITS)
    assert len(tool.EDITS) == 77
    (edit,) = tool.EIG_EDITS
    assert edit.what == WHAT and edit.after and edit.context and not edit.guard
    assert "NPH_LINALG_TAKES(a)" in edit.new and "return NPH_Eig(a);" in edit.new
    default = tool.snippet_check_source()
    assert "NPH_Eig" not in default and WHAT not in default
    src = tool.snippet_check_source(tool.EIG_EDITS)
    assert "/* %s */" % WHAT in src and "return NPH_Eig(a);" in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    for k, (old, new) in enumerate((("return NPH_Eig(a);", "return NPH_Eig(a, a);"), ("return NPH_Eig(a);", "return NPH_Eigh(a);"))):
        bad_src = src.replace(old, new)
        assert bad_src != src
        bad = tmp_path / ("bad%d.c" % k)
        bad.write_text(bad_src)
        assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_eig_bodies_cpu_operand_reaches_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "eig_bodies"
    tool = _tool()
    gen = tool.eig_program_source()
    for line in tool.EIG_EDITS[0].new.split("\n"):
        assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "eig_bodies cpu: 1 calls reached the reference's own code, 0 failures" in proc.stdout


def test_the_eigensolver_stays_out_of_the_translation_unit_the_null_device_build_compiles():
    """As for the SVD (tests/test_svd_glue_cpu.py): numpower_host.cpp is built against the null device, which has no factorizations."""
    for path in (ROOT / "tests" / "null_device").iterdir():
        if path.is_file():
            text = path.read_text(errors="replace")
            assert "np_eigh" not in text and "np_eigvalsh" not in text and "NDArray_Eig" not in text, path
    host = (ROOT / "numpower_amd" / "host" / "numpower_host.cpp").read_text()
    assert "np_eigh" not in host and "NDArray_Eig" not in host and "np_symmetry_mismatch" not in host
    assert "NDArray_Eig" in (ROOT / "numpower_amd" / "host" / "numpower_linalg.cpp").read_text()


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_device_eigensolver_only_when_asked(tmp_path):
    tool = _tool()
    plain, out = tmp_path / "plain", tmp_path / "numpower"
    before = tool.apply(REF, plain)
    applied = tool.apply(REF, out, extra=tool.EIG_EDITS)
    assert dict(applied) == dict(before) and len(applied) == len(tool.EDITS)
    assert applied.extra == {WHAT: 1}
    text = (out / "src" / "ndmath" / "linalg.c").read_text()
    body = _function(text, "NDArray_Eig(NDArray *a) {")
    assert body.count("return NPH_Eig(a);") == 1
    assert body.index("Input matrix is not square") < body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_LINALG_TAKES(a)") < \
        body.index("return NPH_Eig(a);") < body.index("#endif") < body.index("emalloc(")
    inserted = body[body.index("#ifdef HAVE_NP_HIP"):body.index("#endif") + len("#endif\n")]
    # without the inserted block: the tree the tool makes without `extra`, the other linalg edits applied as before
    assert text.replace(inserted, "", 1) == (plain / "src" / "ndmath" / "linalg.c").read_text()
    assert "NPH_Eig" not in (plain / "src" / "ndmath" / "linalg.c").read_text()


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_command_line_counts(tmp_path, capsys):
    tool = _tool()
    assert tool.main(["apply_with_hip.py", str(REF), str(tmp_path / "a")]) == 0
    assert "79 edits in" in capsys.readouterr().out
    assert tool.main(["apply_with_hip.py", "--eig", str(REF), str(tmp_path / "b")]) == 0
    out = capsys.readouterr().out
    assert "80 edits in" in out and "applied x1  %s" % WHAT in out
    assert "NPH_Eig" in (tmp_path / "b" / "src" / "ndmath" / "linalg.c").read_text()
    assert "NPH_Eig" not in (tmp_path / "a" / "src" / "ndmath" / "linalg.c").read_text()
