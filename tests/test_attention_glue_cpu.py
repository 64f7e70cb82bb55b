"""CPU-tier checks of the boundary of scaled dot-product attention (np_attention.hip, ext/hip_dnn.c, host/numpower_dnn.cpp, ndarray.py):
the two calls are declared below the group-normalization block, prototyped and exported; the probes return zeros before any launch
and report the constants the family restates; the header's comment block states each rule; every refusal comes back on a machine
with no device, so nothing ran; each message of the glue is raised with its text."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import attention_family as A

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_ATTN_MSG_NDIM": "dnn_attention: q, k and v must have at least 2 dimensions (..., S, D) and the same number of them",
    "NPH_ATTN_MSG_LEADING": "dnn_attention: the leading axes of q, k and v must be equal",
    "NPH_ATTN_MSG_D": "dnn_attention: q, k and v must have the same last axis D",
    "NPH_ATTN_MSG_SK": "dnn_attention: k and v must have the same number of rows Sk",
    "NPH_ATTN_MSG_EMPTY": "dnn_attention: an operand has no elements",
    "NPH_ATTN_MSG_DMAX": "dnn_attention: D, the last axis, must not be above 128",
    "NPH_ATTN_MSG_OUTPUT": "dnn_attention_backward: o and dout must have the shape of q",
    "NPH_ATTN_MSG_SAVED": "dnn_attention_backward: save_max and save_sum must have the shape of q without its last axis",
    "NPH_ATTN_MSG_SCALE": "dnn_attention: scale must be finite",
    "NPH_ATTN_MSG_DEVICE": "dnn_attention: the operands must be on the same device",
    "NPH_ATTN_MSG_CPU": "dnn_attention: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
}
UNIT = ROOT / "numpower_amd" / "csrc" / "np_attention.hip"


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def test_abi_is_declared_below_the_groupnorm_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert ("int np_attention_forward(const float *q, const float *k, const float *v, size_t BH, size_t Sq, size_t Sk, size_t D, int causal, "
            "float scale, float *o, float *save_max , float *save_sum );") in text
    assert ("int np_attention_backward(const float *q, const float *k, const float *v, const float *o, const float *dout, const float *save_max, "
            "const float *save_sum, size_t BH, size_t Sq, size_t Sk, size_t D, int causal, float scale, float *dq, float *dk, float *dv);") in text
    order = [text.index(s) for s in ("int np_groupnorm_forward(", "int np_groupnorm_backward(", "int np_attention_forward(", "int np_attention_backward(",
                                     "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_attention_last_path(int *d_class, int *q_tile, int *k_tile, int *launches, size_t *key_tiles, size_t *skipped);" in debug
    assert "int np_debug_attention_bounds(size_t bounds[], int n);" in debug
    order = [debug.index(s) for s in ("int np_debug_groupnorm_bounds(", "int np_debug_attention_last_path(", "int np_debug_attention_bounds(",
                                      "#define NP_REDUCE_PATH_ROWS_BLOCK")]
    assert order == sorted(order)
    names = ("np_attention_forward", "np_attention_backward", "np_debug_attention_last_path", "np_debug_attention_bounds")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [12, 16, 6, 2]
    assert _lib.PROTOTYPES["np_attention_forward"][1][8] == C.c_float and _lib.PROTOTYPES["np_attention_backward"][1][12] == C.c_float
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_attention.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build
    assert "#pragma clang fp contract(off)" in (UNIT.parent / "np_elementwise_ops.h").read_text() and '#include "np_elementwise_ops.h"' in UNIT.read_text()


def test_the_probes_are_zero_before_any_launch_and_report_the_constants():
    from numpower_amd import _lib
    lib = _lib.load()
    vals = [C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_size_t(7), C.c_size_t(7)]
    refs = [C.byref(v) for v in vals]
    for k in range(6):
        assert lib.np_debug_attention_last_path(*[None if j == k else v for j, v in enumerate(refs)]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_attention_last_path(*refs) == _lib.NP_OK
    assert [v.value for v in vals] == [0] * 6
    bounds = (C.c_size_t * 7)()
    assert lib.np_debug_attention_bounds(None, 7) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_attention_bounds(bounds, 6) == NP_ERR_INVALID and b"room for 7" in lib.np_last_error()
    assert lib.np_debug_attention_bounds(bounds, 7) == _lib.NP_OK
    assert tuple(bounds) == A.BOUNDS                         # the family's dispatcher uses the library's constants
    tq, tk, d0, d1, d2, wave, keys = bounds
    assert tq == 4 * wave and tk == wave == 32 and (d0, d1, d2) == (32, 64, 128) and keys % wave == 0
    src = UNIT.read_text()
    for name, value in (("kTQ", tq), ("kTK", tk), ("kWaveRows", wave), ("kKeysPerGroup", keys), ("kMaxD", d2)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert "int d_class_of(size_t D) { return D <= 32 ? 32 : D <= 64 ? 64 : 128; }" in src


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("scaled dot-product attention (np_attention.hip"):raw.index("int np_attention_forward(")]
    for phrase in ("the (Sq x Sk) score matrix is never stored", "q (BH, Sq, D), k (BH, Sk, D), v (BH, Sk, D), o (BH, Sq, D)",
                   "save_max and save_sum (BH, Sq)", "1 <= D <= 128", "or j <= i when causal", "the alignment is top-left",
                   "every row sees at least key 0", "fmaf chain from +0.0f over d ascending", "ONE fp32 multiply of the finished dot product by scale",
                   "a NaN never wins", "e_ij = fast_exp(s_ij - m_i)", "evaluated online over key tiles", "the rescaling of online_add",
                   "always walked from key 0", "a fixed permutation", "ONE correctly rounded division per element, no reciprocal",
                   "save_max = m_i, save_sum = l_i", "what the online evaluation ended with", "p_ij = fast_exp(s_ij - m_i) / l_i",
                   "the same instruction sequence as the forward probability", "delta_i = sum over d of dout_id . o_id", "dp_ij = chain_d(dout_id . v_jd)",
                   "ds_ij = p_ij . (dp_ij - delta_i)", "dv_jd = sum over i of p_ij . dout_id", "dk_jd = (sum over i of ds_ij . q_id) . scale",
                   "dq_id = (sum over j of ds_ij . k_jd) . scale", "Any of dq, dk, dv may be NULL",
                   "a kernel that would only produce NULL outputs is not launched", "no float atomics",
                   "a function of the extents and the compile-time tile constants alone", "bit-identical from run to run",
                   "a slice alone equals the same slice inside a larger batch", "the first n rows of a call equal the call on q[:, :n]",
                   "row i reads the key tiles 0 .. i / T alone", "min(c, i + 1) = min(Sk, i + 1)", "makes row i of o, save_sum and dq NaN, and no other row of o",
                   "makes every row that sees j NaN", "are NOT specified", "0 . NaN on the matrix core is NaN", "skipped tiles never read it",
                   "No other slice b is ever reached", "A row whose visible scores are all -Inf is NaN in o and in save_sum", "The forward pass takes no scratch",
                   "pool scratch for delta (BH.Sq floats)", "nothing proportional to Sq.Sk", "released on every path", "on the library stream",
                   "every offset is formed in size_t, so BH.S.D may pass 2^31", "does not fit the grid arithmetic and is refused",
                   "pointers are checked first, then the extents, the scale, the aliasing, then work begins", "a scale that is not finite"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    p = [C.c_void_p(k << 28) for k in range(1, 11)]      # far apart, never dereferenced
    ok = (2, 5, 7, 8)
    fwd = lambda q, k, v, o, m=None, l=None, shape=ok, scale=0.5, causal=0: lib.np_attention_forward(q, k, v, *shape, causal, scale, o, m, l)
    bwd = lambda ins, outs, shape=ok, scale=0.5: lib.np_attention_backward(*ins, *shape, 1, scale, *outs)
    for k in range(4):
        args = list(p[:4])
        args[k] = None
        assert fwd(*args) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in range(7):
        ins = list(p[:7])
        ins[k] = None
        assert bwd(ins, p[7:10]) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    for k in range(4):
        bad = list(ok)
        bad[k] = 0
        assert fwd(*p[:4], shape=bad) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
        assert bwd(p[:7], p[7:10], bad) == NP_ERR_INVALID and b"at least 1" in lib.np_last_error()
    for D in (129, 256, 1 << 31, 1 << 63):
        assert fwd(*p[:4], shape=(2, 5, 7, D)) == NP_ERR_INVALID and b"is above 128" in lib.np_last_error()
        assert bwd(p[:7], p[7:10], (2, 5, 7, D)) == NP_ERR_INVALID and b"is above 128" in lib.np_last_error()
    for big in (1 << 31, (1 << 31) + 5, 1 << 40, 1 << 63):
        for shape in ((1, big, 7, 8), (1, 5, big, 8)):
            assert fwd(*p[:4], shape=shape) == NP_ERR_INVALID and b"Sq or Sk is 2^31 or more" in lib.np_last_error()
        assert fwd(*p[:4], shape=(big, 5, 7, 8)) == NP_ERR_INVALID and b"tiles of a slice is 2^31 or more" in lib.np_last_error()
    assert fwd(*p[:4], shape=(1 << 24, 1 << 14, 7, 8)) == NP_ERR_INVALID and b"tiles of a slice is 2^31 or more" in lib.np_last_error()
    assert bwd(p[:7], p[7:10], (1 << 24, 7, 1 << 14, 8)) == NP_ERR_INVALID and b"tiles of a slice is 2^31 or more" in lib.np_last_error()
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert fwd(*p[:4], scale=scale) == NP_ERR_INVALID and b"scale must be finite" in lib.np_last_error()
        assert bwd(p[:7], p[7:10], scale=scale) == NP_ERR_INVALID and b"scale must be finite" in lib.np_last_error()
    near = lambda a, k=8: C.c_void_p(a.value + k)
    for args in ((p[0], p[1], p[2], p[0]), (p[0], p[1], p[2], near(p[1])), (p[0], p[1], p[2], p[3], near(p[2], 4)), (p[0], p[1], p[2], p[3], p[4], near(p[4], 4)),
                 (p[0], p[1], p[2], p[3], near(p[3], 16))):
        assert fwd(*args) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    for outs in ((p[0], p[8], p[9]), (p[7], near(p[4]), p[9]), (p[7], p[8], near(p[8], 4)), (None, near(p[6], 4), None), (near(p[5]), None, None)):
        assert bwd(p[:7], outs) == NP_ERR_INVALID and b"overlaps" in lib.np_last_error()
    vals = [C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_size_t(7), C.c_size_t(7)]
    assert lib.np_debug_attention_last_path(*[C.byref(v) for v in vals]) == _lib.NP_OK and vals[0].value == 0      # no device, no launch

    src = UNIT.read_text()
    body = _function(src, "int np_attention_forward(")      # pointers, extents and scale, aliasing, then work
    assert body.index("null pointer") < body.index("check_call(") < body.index("any_overlap(") < body.index("ensure_init()") < body.index("<<<")
    assert "alloc" not in body                                # the forward pass takes no scratch
    body = _function(src, "int np_attention_backward(")
    assert body.index("null pointer") < body.index("check_call(") < body.index("any_overlap(") < body.index("ensure_init()") < body.index("delta.alloc(") \
        < body.index("attn_delta_kernel<<<") < body.index("attn_dkdv_kernel<") < body.index("attn_dq_kernel<")
    assert "np::Scratch delta;" in body and body.count("alloc(") == 1 and "if (dk || dv)" in body and "if (dq)" in body
    body = _function(src, "int check_call(")
    assert body.index("at least 1") < body.index("is above") < body.index("Sq or Sk is 2^31") < body.index("tiles of a slice") < body.index("does not fit") \
        < body.index("scale must be finite")
    assert "ensure_init" not in body and "hip" not in body
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "num_cus" not in code and "__fdividef" not in code and "rcp" not in code and "hipMalloc" not in code and "asm" not in code
    assert code.count("__builtin_amdgcn_mfma_f32_32x32x2f32") == 2 and "__fdiv_rn" in code      # chain_block and accumulate_block: every product


def test_the_family_restates_the_dispatcher():
    """pinned by hand: (Sq, Sk, D, causal) -> (d_class, key tiles of the last workgroup row, skipped pairs)"""
    pins = {(1, 1, 1, False): (32, 1, 0), (1, 257, 32, True): (32, 1, 8), (128, 128, 33, True): (64, 4, 0), (129, 129, 64, True): (64, 5, 1),
            (129, 129, 65, False): (128, 5, 0), (257, 257, 128, True): (128, 9, 6), (257, 32, 4, True): (32, 1, 0), (64, 257, 16, True): (32, 2, 7),
            (256, 64, 64, True): (64, 2, 0), (300, 300, 100, True): (128, 10, 8), (8192, 8192, 64, True): (64, 256, 8064), (33, 31, 31, False): (32, 1, 0)}
    for (Sq, Sk, D, causal), (dc, kt, sk) in pins.items():
        assert A.probe(Sq, Sk, D, causal)[:3] == (dc, 128, 32) and A.probe(Sq, Sk, D, causal)[4:] == (kt, sk), (Sq, Sk, D, causal)
    assert [A.d_class(D) for D in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert A.launches(False) == 1 and A.launches(True) == 3 and A.launches(True, (True, False, False)) == 2
    assert A.launches(True, (False, True, False)) == 2 and A.launches(True, (False, False, False)) == 0
    src = UNIT.read_text()
    fn = _function(src, "__host__ __device__ __forceinline__ unsigned key_tiles_of(")
    assert "const unsigned last = (q0 + kTQ < Sq ? q0 + kTQ : Sq) - 1, need = last / kTK + 1;" in fn and "return need < nkt ? need : nkt;" in fn


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    for text in ("NDArray **NDArrayDNN_Attention_Forward(NDArray *q, NDArray *k, NDArray *v, int causal, float scale);",
                 "NDArray **NDArrayDNN_Attention_Backward(NDArray *q, NDArray *k, NDArray *v, NDArray *o, NDArray *dout, NDArray *save_max, NDArray *save_sum, "
                 "int causal, float scale);"):
        assert text in host, text
    order = [host.index(s) for s in ("NDArrayDNN_GroupNorm_Backward(", "NDArrayDNN_Attention_Forward(", "NDArrayDNN_Attention_Backward(")]
    assert order == sorted(order)
    h = ndarray._load_host()
    assert hasattr(h, "NDArrayDNN_Attention_Forward") and hasattr(h, "NDArrayDNN_Attention_Backward")
    glue = _header("hip_dnn.h", "ext")
    for text in ("struct NDArray **NPH_Attention_Forward(struct NDArray *q, struct NDArray *k, struct NDArray *v, int causal, float scale);",
                 "struct NDArray **NPH_Attention_Backward(struct NDArray *q, struct NDArray *k, struct NDArray *v, struct NDArray *o, struct NDArray *dout, "
                 "struct NDArray *save_max, struct NDArray *save_sum, int causal, float scale);"):
        assert text in glue, text
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    check = _function(src, "static int attention_of(")
    order = [check.index("NPH_ATTN_MSG_" + n) for n in ("NDIM", "LEADING", "D)", "SK", "EMPTY", "DMAX", "OUTPUT", "SAVED", "SCALE", "DEVICE", "CPU")]
    assert order == sorted(order) and "NDArray_Empty" not in check and "np_attention" not in check
    fwd = _function(src, "NDArray **NPH_Attention_Forward(")
    assert fwd.index("attention_of(") < fwd.index("empty_like_on_gpu(") < fwd.index("np_attention_forward(") < fwd.index("batchnorm_drop(rtns, o, smax, ssum);\n    }")
    bwd = _function(src, "NDArray **NPH_Attention_Backward(")
    assert bwd.index("attention_of(") < bwd.index("empty_like_on_gpu(") < bwd.index("np_attention_backward(") and bwd.count("batchnorm_drop(") == 2
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for n in ("Forward", "Backward"):
        body = _function(cpp, "NDArray **NDArrayDNN_Attention_" + n + "(")
        assert "on_contiguous(" in body and "NPH_Attention_" + n + "(" in body
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "Attention" not in tool and "attention" not in tool      # the reference has no attention: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message before them needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    f, b, M = NDArray.dnn_attention_forward, NDArray.dnn_attention_backward, (lambda n: MESSAGES["NPH_ATTN_MSG_" + n])
    q, k, v = ones(2, 5, 8), ones(2, 7, 8), ones(2, 7, 8)
    o, dout, m, l = ones(2, 5, 8), ones(2, 5, 8), ones(2, 5), ones(2, 5)

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    for bad in ((ones(8), ones(8), ones(8)), (q, ones(7, 8), v), (q, k, ones(2, 1, 7, 8)), (ones(1, 2, 5, 8), k, v)):
        assert message(f, *bad) == M("NDIM") and message(b, *bad, o, dout, m, l) == M("NDIM")
    for bad in ((q, ones(3, 7, 8), v), (q, k, ones(1, 7, 8)), (ones(4, 5, 8), k, v)):
        assert message(f, *bad) == M("LEADING") and message(b, *bad, o, dout, m, l) == M("LEADING")
    assert message(f, ones(2, 3, 5, 8), ones(2, 3, 7, 8), ones(2, 4, 7, 8)) == M("LEADING")
    for bad in ((q, ones(2, 7, 9), v), (q, k, ones(2, 7, 4)), (ones(2, 5, 7), k, v)):
        assert message(f, *bad) == M("D") and message(b, *bad, o, dout, m, l) == M("D")
    for bad in ((q, k, ones(2, 6, 8)), (q, ones(2, 8, 8), v)):
        assert message(f, *bad) == M("SK") and message(b, *bad, o, dout, m, l) == M("SK")
    for shape_q, shape_k in (((0, 5, 8), (0, 7, 8)), ((2, 0, 8), (2, 7, 8)), ((2, 5, 8), (2, 0, 8)), ((2, 5, 0), (2, 7, 0))):
        assert message(f, ones(*shape_q), ones(*shape_k), ones(*shape_k)) == M("EMPTY")
    for D in (129, 200):
        assert message(f, ones(2, 5, D), ones(2, 7, D), ones(2, 7, D)) == M("DMAX")
    for bad in (ones(2, 5, 7), ones(2, 4, 8), ones(80), ones(5, 8)):
        assert message(b, q, k, v, bad, dout, m, l) == M("OUTPUT") and message(b, q, k, v, o, bad, m, l) == M("OUTPUT")
    for bad in (ones(2, 4), ones(10), ones(2, 5, 1), ones(5, 2)):
        assert message(b, q, k, v, o, dout, bad, l) == M("SAVED") and message(b, q, k, v, o, dout, m, bad) == M("SAVED")
    assert message(f, q, k, v, scale=float("inf")) == M("SCALE") and message(b, q, k, v, o, dout, m, l, scale=float("inf")) == M("SCALE")
    for args in ((q, k, v), (ones(5, 8), ones(7, 8), ones(7, 8)), (ones(2, 3, 5, 128), ones(2, 3, 1, 128), ones(2, 3, 1, 128))):      # the right operands get as far as the device check
        for kw in ({}, {"causal": True}, {"scale": 0.3}, {"scale": None}):
            assert message(f, *args, **kw) == M("CPU")
    assert message(b, q, k, v, o, dout, m, l) == M("CPU") and message(b, q, k, v, o, dout, m, l, True, 2.0) == M("CPU")
    for bad in (0, -1.0, float("nan")):      # the Python layer keeps "the default" to None
        assert message(f, q, k, v, scale=bad) == "dnn_attention_forward: scale must be greater than zero (None: 1 / sqrt(D))"
    assert message(f, q, k, v, scale="small") == "dnn_attention_forward: scale must be a number or None"
    assert message(b, q, k, v, o, dout, m, l, scale=True) == "dnn_attention_backward: scale must be a number or None"
    assert message(f, q, None, v) == "dnn_attention_forward: q, k and v must be arrays"
    assert message(b, q, k, v, o, None, m, l) == "dnn_attention_backward: q, k, v, o, dout, save_max and save_sum must be arrays"
    assert "scale=None means 1 / sqrt(D)" in " ".join(f.__doc__.split())
