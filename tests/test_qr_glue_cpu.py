"""CPU-tier checks of the Householder QR's boundary (np_qr.hip, ext/hip_linalg.c, host/numpower_linalg.cpp): np_geqrf / np_qr /
np_lstsq are declared, prototyped and exported and refuse null and m < n arguments; the header states the convention; NDArray_Qr
and NDArray_Lstsq have the reference's signatures and messages; the --with-hip early-outs are two edits in a list of their own
that is NOT part of EDITS and reaches a tree only under --qr; qr_bodies shows CPU operands reaching the reference's own code."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
WHAT_LSTSQ = "linalg.c:849 NDArray_Lstsq: GPU early-out"
WHAT_QR = "linalg.c:909 NDArray_Qr: GPU early-out"
SHAPE_MESSAGE = ("Invalid dimensions to calculate lstsq, both arrays must have 2 dimensions and $b must contain the same amount "
                 "of rows as $a")
RANK_MESSAGE = "The diagonal element %i of the triangular factor of $a is zero, so that $a does not have full rank."
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
    assert "int np_geqrf(float *a, size_t m, size_t n, float *tau);" in text
    assert "int np_qr(const float *a, size_t m, size_t n, float *q, float *r);" in text
    assert "int np_lstsq(const float *a, const float *b, size_t m, size_t n, size_t nrhs, float *x, int *info_host);" in text
    for n in ("np_geqrf", "np_qr", "np_lstsq"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in ("np_geqrf", "np_qr", "np_lstsq")] == [4, 5, 7]
    assert "np_qr.hip" in (ROOT / "numpower_amd" / "build.py").read_text()


def test_the_header_states_the_convention():
    raw = re.sub(r"\s+", " ", (ROOT / "include" / "np_hip.h").read_text().replace(" * ", " "))
    block = raw[raw.index("Householder QR and least squares (np_qr.hip"):raw.index("int np_geqrf(")]
    for phrase in ("sgeqr2 / slarfg", "sign(+0) = sign(-0) = +", "tau_j = (beta - alpha) / beta", "v_j = x / (alpha - beta)",
                   "A zero sub-column (x == 0 exactly) gives tau_j = 0", "R's diagonal is not normalised", "not made positive",
                   "the reduced factorization", "mode='reduced'", "strict lower triangle of exact +0.0f",
                   "m < n is refused by all three", "minimum-norm branch of sgels for m < n is out of scope",
                   "j + 1 for the first j with R_jj == 0 exactly", "x is not written",
                   "m <= 16777216, n <= 65536", "refused, not truncated", "Scratch", "released on every path",
                   "bit-identical from run to run", "no float atomics", "fp64 and rounds once", "power-of-two scaling",
                   "Non-finite input", "never sorgqr", "packed reflectors", "Different from the reference's CPU qr on purpose"):
        assert phrase.lower() in block.lower(), phrase


def test_null_and_wide_arguments_are_refused_before_any_device_work():
    from numpower_amd import _lib
    lib = _lib.load()
    info = C.c_int(7)
    # argument checks come after np_init: without a device they report that instead; either way nothing runs
    for rc in (lib.np_geqrf(None, 4, 3, None), lib.np_qr(None, 4, 3, None, None), lib.np_lstsq(None, None, 4, 3, 1, None, C.byref(info)),
               lib.np_lstsq(None, None, 4, 3, 1, None, None),
               lib.np_geqrf(None, 3, 4, None), lib.np_qr(None, 3, 4, None, None), lib.np_lstsq(None, None, 3, 4, 1, None, C.byref(info))):
        assert rc != _lib.NP_OK
    assert info.value == 7
    src = (ROOT / "numpower_amd" / "csrc" / "np_qr.hip").read_text()
    for name in ("np_geqrf", "np_qr", "np_lstsq"):     # the order inside each entry point: pointers, then the shape, then work
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        assert body.index("null pointer") < body.index("check_shape(") < body.index(".alloc("), name
    assert "is smaller than n" in src and "NP_ERR_INVALID" in src[src.index("int check_shape("):src.index("}  // namespace")]


def test_host_functions_have_the_reference_signatures():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert "NDArray **NDArray_Qr(NDArray *a);" in host and "NDArray *NDArray_Lstsq(NDArray *a, NDArray *b);" in host
    h = ndarray._load_host()
    assert hasattr(h, "NDArray_Qr") and hasattr(h, "NDArray_Lstsq")
    glue = _header("hip_linalg.h", "ext")
    assert "struct NDArray **NPH_Qr(struct NDArray *a);" in glue
    assert "struct NDArray *NPH_Lstsq(struct NDArray *a, struct NDArray *b);" in glue
    assert callable(ndarray.NDArray.qr) and callable(ndarray.NDArray.lstsq)


@pytest.mark.skipif(not (REF / "src" / "ndmath" / "linalg.h").exists(), reason="needs a NumPower checkout to compare with")
def test_the_signatures_are_the_ones_the_reference_declares():
    ref = re.sub(r"\s+", "", (REF / "src" / "ndmath" / "linalg.h").read_text())
    assert "NDArray**NDArray_Qr(NDArray*a);" in ref and "NDArray*NDArray_Lstsq(NDArray*a,NDArray*b);" in ref


def test_shape_errors_and_the_cpu_refusal():
    from numpower_amd.ndarray import NDArray, Error
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    for bad in (ones(3), ones(2, 2, 2)):
        with pytest.raises(Error, match="qr: the operand must be two-dimensional"):
            NDArray.qr(bad)
    with pytest.raises(Error, match="m >= n"):
        NDArray.qr(ones(2, 3))
    for a, b in ((ones(3), ones(3, 1)), (ones(3, 2), ones(3)), (ones(3, 2), ones(4, 1)), (ones(2, 2, 2), ones(2, 2))):
        with pytest.raises(Error) as e:
            NDArray.lstsq(a, b)
        assert str(e.value) == SHAPE_MESSAGE
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.qr(ones(3, 2))
    with pytest.raises(Error, match="only computes on the GPU"):
        NDArray.lstsq(ones(3, 2), ones(3, 1))


def test_the_glue_raises_the_reference_messages_and_declares_the_reference_shapes():
    src = (ROOT / "ext" / "hip_linalg.c").read_text()
    qr = src[src.index("NDArray **NPH_Qr(NDArray *a) {"):src.index("NDArray *NPH_Lstsq(")]
    assert "zeros_on_gpu(2, m, n)" in qr and "zeros_on_gpu(2, n, n)" in qr and "np_qr(" in qr and "np_ext_throw_last();" in qr
    assert qr.index("rtns[0] = q;") < qr.index("rtns[1] = r;")
    assert qr.index("two-dimensional") < qr.index("m >= n") < qr.index("on_gpu(a)") < qr.index("zeros_on_gpu(") < qr.index("np_qr(")
    lstsq = re.sub(r'"\s*\n\s*"', "", src[src.index("NDArray *NPH_Lstsq("):])
    assert '"%s"' % SHAPE_MESSAGE in lstsq and '"%s"' % RANK_MESSAGE in lstsq
    assert "zeros_on_gpu(2, n, nrhs)" in lstsq and "np_lstsq(" in lstsq and "np_ext_throw_last();" in lstsq
    assert lstsq.index(SHAPE_MESSAGE) < lstsq.index("same device") < lstsq.index("on_gpu(a)") < lstsq.index("zeros_on_gpu(") < \
        lstsq.index("np_lstsq(") < lstsq.index(RANK_MESSAGE)
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "NPH_Qr" in integration and "deliberate difference" in integration


def test_the_edits_are_a_list_of_their_own_outside_edits_and_pass_the_snippet_check(tmp_path):
    tool = _tool()
    assert len(tool.QR_EDITS) == 2
    for other in (tool.EDITS, tool.SIGNAL_EDITS, tool.EIG_EDITS):
        assert not any(e in other for e in tool.QR_EDITS)
    assert len(tool.EDITS) == 77
    lstsq, qr = tool.QR_EDITS
    assert lstsq.what == WHAT_LSTSQ and qr.what == WHAT_QR
    for e in tool.QR_EDITS:
        assert e.after and e.context and not e.guard and "NPH_LINALG_TAKES(a)" in e.new
    assert "return NPH_Lstsq(a, b);" in lstsq.new and "return NPH_Qr(a);" in qr.new
    default = tool.snippet_check_source()
    assert "NPH_Qr" not in default and "NPH_Lstsq" not in default and WHAT_QR not in default
    src = tool.snippet_check_source(tool.QR_EDITS)
    assert "/* %s */" % WHAT_QR in src and "/* %s */" % WHAT_LSTSQ in src
    good = tmp_path / "snippets.c"
    good.write_text(src)
    proc = subprocess.run(GCC_CHECK + [str(good)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    for k, (old, new) in enumerate((("return NPH_Qr(a);", "return NPH_Qr(a, a);"), ("return NPH_Lstsq(a, b);", "return NPH_Lstsq(a);"),
                                    ("return NPH_Qr(a);", "return NPH_QR(a);"))):
        bad_src = src.replace(old, new)
        assert bad_src != src
        bad = tmp_path / ("bad%d.c" % k)
        bad.write_text(bad_src)
        assert subprocess.run(GCC_CHECK + [str(bad)], capture_output=True, text=True).returncode != 0


def test_qr_bodies_cpu_operands_reach_the_reference_code():
    exe = ROOT / "numpower_amd" / "lib" / "qr_bodies"
    tool = _tool()
    gen = tool.qr_program_source()
    for e in tool.QR_EDITS:
        for line in e.new.split("\n"):
            assert line.strip() in gen
    proc = subprocess.run([str(exe), "cpu"], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "qr_bodies cpu: 2 calls reached the reference's own code, 0 failures" in proc.stdout


def test_the_qr_stays_out_of_the_translation_unit_the_null_device_build_compiles():
    """As for the SVD (tests/test_svd_glue_cpu.py): numpower_host.cpp is built against the null device, which has no factorizations."""
    for path in (ROOT / "tests" / "null_device").iterdir():
        if path.is_file():
            text = path.read_text(errors="replace")
            assert "np_geqrf" not in text and "np_lstsq" not in text and "NDArray_Qr" not in text, path
    host = (ROOT / "numpower_amd" / "host" / "numpower_host.cpp").read_text()
    assert "np_lstsq" not in host and "NDArray_Qr" not in host and "NDArray_Lstsq" not in host
    linalg = (ROOT / "numpower_amd" / "host" / "numpower_linalg.cpp").read_text()
    assert "NDArray_Qr" in linalg and "NDArray_Lstsq" in linalg


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_patched_tree_routes_gpu_operands_to_the_device_qr_only_when_asked(tmp_path):
    tool = _tool()
    plain, out = tmp_path / "plain", tmp_path / "numpower"
    before = tool.apply(REF, plain)
    applied = tool.apply(REF, out, extra=tool.QR_EDITS)
    assert dict(applied) == dict(before) and len(applied) == len(tool.EDITS)
    assert applied.extra == {WHAT_LSTSQ: 1, WHAT_QR: 1}
    text = (out / "src" / "ndmath" / "linalg.c").read_text()
    plain_text = (plain / "src" / "ndmath" / "linalg.c").read_text()
    for opening, call, throw in (("NDArray_Lstsq(NDArray *a, NDArray *b) {", "return NPH_Lstsq(a, b);", "ndarray::lstsq not implemented for GPU"),
                                 ("NDArray_Qr(NDArray *a) {", "return NPH_Qr(a);", "ndarray::qr not implemented for GPU")):
        body = _function(text, opening)
        assert body.count(call) == 1
        assert body.index("#ifdef HAVE_NP_HIP") < body.index("NPH_LINALG_TAKES(a)") < body.index(call) < body.index("#endif") < \
            body.index(throw)
        inserted = body[body.index("#ifdef HAVE_NP_HIP"):body.index("#endif") + len("#endif\n")]
        text = text.replace(inserted, "", 1)
    assert text == plain_text                                  # without the two inserted blocks: the tree the tool makes without `extra`
    assert "NPH_Qr" not in plain_text and "NPH_Lstsq" not in plain_text


@pytest.mark.skipif(not HAS_REF, reason="needs a NumPower checkout for tools/apply_with_hip.py to patch")
def test_the_command_line_counts(tmp_path, capsys):
    tool = _tool()
    assert tool.main(["apply_with_hip.py", str(REF), str(tmp_path / "a")]) == 0
    assert "79 edits in" in capsys.readouterr().out
    assert tool.main(["apply_with_hip.py", "--qr", str(REF), str(tmp_path / "b")]) == 0
    out = capsys.readouterr().out
    assert "81 edits in" in out and "applied x1  %s" % WHAT_QR in out and "applied x1  %s" % WHAT_LSTSQ in out
    assert tool.main(["apply_with_hip.py", "--eig", "--qr", str(REF), str(tmp_path / "c")]) == 0
    assert "82 edits in" in capsys.readouterr().out
    b = (tmp_path / "b" / "src" / "ndmath" / "linalg.c").read_text()
    assert "NPH_Qr" in b and "NPH_Lstsq" in b and "NPH_Eig" not in b
    a = (tmp_path / "a" / "src" / "ndmath" / "linalg.c").read_text()
    assert "NPH_Qr" not in a and "NPH_Lstsq" not in a
