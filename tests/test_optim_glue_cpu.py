"""CPU-tier checks of the boundary of the optimizer steps (np_optim.hip, ext/hip_dnn.c, host/numpower_dnn.cpp, ndarray.py, optim.py):
the three calls are declared below the attention block, prototyped and exported; the probes return zeros before any launch and
report the constants that tests/optim_family.py restates; every refusal comes back on a machine with no device, so nothing ran;
each message of the glue is raised with its text; the header's comment block states each rule; optim.py checks its arguments."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import optim_family as fam

ROOT = Path(__file__).resolve().parent.parent
NP_ERR_INVALID = -1            # np_hip.h: np_status
MESSAGES = {
    "NPH_OPTIM_MSG_LENGTHS": "dnn_optim: the lists of parameters, gradients and states must have the same length",
    "NPH_OPTIM_MSG_NULL": "dnn_optim: a list holds an entry that is not an array",
    "NPH_OPTIM_MSG_EMPTY_LIST": "dnn_optim: the list is empty",
    "NPH_OPTIM_MSG_BUFFERS": "dnn_sgd_step: a momentum needs the list of buffers",
    "NPH_OPTIM_MSG_EMPTY": "dnn_optim: an operand has no elements",
    "NPH_OPTIM_MSG_COUNT": "dnn_optim: a gradient or a state must have as many elements as its parameter",
    "NPH_OPTIM_MSG_SCALE": "dnn_optim: grad_scale must be an array and grad_scale_index an element of it",
    "NPH_OPTIM_MSG_LR": "dnn_optim: lr must be finite and not negative",
    "NPH_OPTIM_MSG_WEIGHT_DECAY": "dnn_optim: weight_decay must be finite and not negative",
    "NPH_OPTIM_MSG_MOMENTUM": "dnn_sgd_step: momentum must lie in [0, 1]",
    "NPH_OPTIM_MSG_DAMPENING": "dnn_sgd_step: dampening must lie in [0, 1]",
    "NPH_OPTIM_MSG_NESTEROV": "dnn_sgd_step: nesterov needs a momentum and zero dampening",
    "NPH_OPTIM_MSG_BETAS": "dnn_adam_step: the betas must lie in [0, 1)",
    "NPH_OPTIM_MSG_EPS": "dnn_adam_step: eps must be finite and not negative",
    "NPH_OPTIM_MSG_STEP": "dnn_adam_step: step must be at least 1",
    "NPH_OPTIM_MSG_MAX_NORM": "dnn_grad_norm: max_norm must not be negative",
    "NPH_OPTIM_MSG_DEVICE": "dnn_optim: the operands must be on the same device",
    "NPH_OPTIM_MSG_CPU": "dnn_optim: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)",
    "NPH_OPTIM_MSG_VIEW": "dnn_optim: parameters and states are updated in place and must be contiguous arrays",
}
INF, NAN = float("inf"), float("nan")


def _header(name, where="include"):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (ROOT / where / name).read_text(), flags=re.S))


def _function(text, opening):
    body = text[text.index(opening):]
    return body[:body.index("\n}\n")]


def _ptrs(*values):
    """a host array of device pointers that are never dereferenced"""
    return (C.c_void_p * len(values))(*values)


def _counts(*values):
    return (C.c_size_t * len(values))(*values)


def test_abi_is_declared_below_the_attention_block_prototyped_and_exported():
    from numpower_amd import _lib
    text, debug, lib = _header("np_hip.h"), _header("np_hip_debug.h"), _lib.load()
    assert ("int np_sgd_step(float *const *params, const float *const *grads, float *const *bufs , const size_t *counts, size_t T, double lr, "
            "double momentum, double dampening, double weight_decay, int nesterov, int first_step, const float *grad_scale );") in text
    assert ("int np_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const size_t *counts, "
            "size_t T, long long step, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, "
            "const float *grad_scale );") in text
    assert "int np_grad_norm(const float *const *grads, const size_t *counts, size_t T, double max_norm, float *dev_out2);" in text
    order = [text.index(s) for s in ("int np_attention_backward(", "int np_sgd_step(", "int np_adam_step(", "int np_grad_norm(", "int np_identity(")]
    assert order == sorted(order)
    assert "int np_debug_optim_last_path(int *launches, size_t *chunks, int *vec_tensors, int *scalar_tensors);" in debug
    assert "int np_debug_optim_bounds(size_t bounds[], int n);" in debug and "int np_debug_optim_force_scalar(int on);" in debug
    names = ("np_sgd_step", "np_adam_step", "np_grad_norm", "np_debug_optim_last_path", "np_debug_optim_bounds", "np_debug_optim_force_scalar")
    for n in names:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [12, 14, 5, 4, 2, 1]
    assert _lib.PROTOTYPES["np_sgd_step"][1][5:9] == [C.c_double] * 4 and _lib.PROTOTYPES["np_adam_step"][1][7:12] == [C.c_double] * 5
    build = (ROOT / "numpower_amd" / "build.py").read_text()
    assert '"np_optim.hip"' in build[build.index("HIP_SOURCES = ["):build.index("HIP_FLAGS")]
    assert "fast-math" not in build and "-ffp-contract" not in build and "unsafe" not in build
    src = (ROOT / "numpower_amd" / "csrc" / "np_optim.hip").read_text()
    assert "#pragma clang fp contract(off)" in src                                          # every fp32 step is rounded on its own
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "hipMalloc" not in code and "hipMemcpy" not in code and "Synchronize" not in code
    assert "__fdividef" not in code and "rcp" not in code and "rsq" not in code and "fmaf" not in code
    assert "sqrt_rn(v)" in code and "__fdiv_rn(r, k.bc2s)" in code and "__fdiv_rn(m, den)" in code
    assert "float sqrt_rn(float x) { return __builtin_sqrtf(x); }" in code and "__fsqrt_rn" not in code      # __fsqrt_rn is the bare 1-ulp estimate
    for step in ("launch_steps<0>", "launch_steps<1>"):                                     # a step takes no scratch at all
        assert step in code
    assert "np::Scratch" not in _function(src, "int launch_steps(") and code.count("np::Scratch") == 1
    assert "np::Scratch partial;" in _function(src, "int np_grad_norm(")


def test_the_probes_are_zero_before_any_launch_and_report_the_constants():
    from numpower_amd import _lib
    lib = _lib.load()
    launches, chunks, vec, scalar = C.c_int(-7), C.c_size_t(7), C.c_int(-7), C.c_int(-7)
    assert lib.np_debug_optim_last_path(None, C.byref(chunks), C.byref(vec), C.byref(scalar)) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_optim_last_path(C.byref(launches), C.byref(chunks), C.byref(vec), C.byref(scalar)) == _lib.NP_OK
    assert (launches.value, chunks.value, vec.value, scalar.value) == (0, 0, 0, 0)
    bounds = (C.c_size_t * 5)()
    assert lib.np_debug_optim_bounds(None, 5) == NP_ERR_INVALID and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_optim_bounds(bounds, 4) == NP_ERR_INVALID and b"room for 5" in lib.np_last_error()
    assert lib.np_debug_optim_bounds(bounds, 5) == _lib.NP_OK
    assert tuple(bounds) == fam.BOUNDS                                                       # the family's dispatcher uses the library's constants
    chunk, most, norm_chunk, per_cu, arg_bytes = bounds
    assert chunk % 1024 == 0 and norm_chunk % 1024 == 0 and most >= 2 and per_cu >= 1
    assert arg_bytes + 64 <= 4096                                                            # the list and the coefficients: one kernel-argument segment
    assert arg_bytes >= most * (4 * 8 + 8) + (most + 1) * 8                                  # Adam's four pointers, a size and the prefix, per tensor
    src = (ROOT / "numpower_amd" / "csrc" / "np_optim.hip").read_text()
    for name, value in (("kChunk", chunk), ("kOptimMaxTensors", most), ("kNormChunk", norm_chunk), ("kWgPerCu", per_cu)):
        assert re.search(r"constexpr unsigned %s = %d;" % (name, value), src), name
    assert lib.np_debug_optim_force_scalar(1) == _lib.NP_OK and lib.np_debug_optim_force_scalar(0) == _lib.NP_OK
    launch = _function(src, "int launch_steps(")            # packed by tensor count alone; the grid from the CU count
    assert "t0 += kOptimMaxTensors" in launch and "grid_of(L.first[L.T])" in launch
    assert "np::num_cus() * kWgPerCu" in _function(src, "unsigned grid_of(")


def test_the_header_states_every_rule():
    raw = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", (ROOT / "include" / "np_hip.h").read_text()))      # the comments' leaders alone
    block = raw[raw.index("optimizer steps (np_optim.hip"):raw.index("int np_grad_norm(")]
    for phrase in ("updates a LIST of T tensors in place", "HOST arrays of device pointers", "travels in the kernel arguments",
                   "copies nothing, takes no scratch and does not synchronise", "may be captured between np_graph_begin and np_graph_end",
                   "ceil(T / 64) launches", "depends on that element's operands and the scalar arguments alone",
                   "the packing into launches, the chunking and the alignment cannot change a bit", "separately rounded fp32 operation, no contraction",
                   "division and square root are correctly rounded", "no reciprocal and no rsqrt", "denormals are kept",
                   "computed in double on the host from the double arguments and rounded to fp32 ONCE", "omd = f32(1 - dampening)",
                   "omb1 = f32(1 - beta1)", "omb2 = f32(1 - beta2)", "lrwd = f32(lr . weight_decay)", "bc2s = f32(sqrt(1 - beta2^step))",
                   "ss = f32(lr / (1 - beta1^step))", "s = *grad_scale is a DEVICE float that the kernel reads",
                   "is SKIPPED, not multiplied through (0 . Inf would otherwise differ)", "weight_decay == 0 skips the decay step",
                   "momentum == 0 skips the buffer", "may be NULL", "a NULL grad_scale skips the scale", "omd . g2 is formed when dampening == 0",
                   "g1 = g . s", "g2 = g1 + (wd . p), a multiply, then an add", "b = g2 when first_step",
                   "b = (mu . b) + (omd . g2), two multiplies, then an add", "d = g2 + (mu . b) with nesterov (the new b), else d = b",
                   "Without momentum d = g2", "p = p - (lr . d), a multiply, then a subtract", "first_step does not read the buffer",
                   "decoupled: p1 = p - (lrwd . p), g2 = g1", "otherwise g2 = g1 + (wd . p), p1 = p", "m = (b1 . m) + (omb1 . g2)",
                   "v = (b2 . v) + ((omb2 . g2) . g2)", "den = (sqrt(v) / bc2s) + eps", "p = p1 - (ss . (m / den))", "step >= 1",
                   "exp_avg and exp_avg_sq are required", "reaches its own element of p and the states, and no other",
                   "weight_decay == 0 with p = +-Inf leaves g untouched", "eps = 0 with v = 0 gives m / 0: NaN for m = 0",
                   "no written range (the parameters and states of ALL tensors) may overlap another written range, a gradient or grad_scale",
                   "by sorting the ranges", "Two gradients may share memory", "all size_t", "beyond 2^31 works",
                   "any 4-byte-aligned pointer is accepted", "congruent mod 16", "16-byte accesses over its aligned middle",
                   "scalar accesses at its head and tail", "the choice is per tensor and both forms give the same bits", "no atomics, no scratch",
                   "bit-identical from run to run", "pointers are checked first, then the extents, the parameters, the aliasing, then work begins",
                   "nesterov with momentum == 0 or dampening != 0", "a beta outside [0, 1)", "step < 1",
                   "each square formed in double from the float (exact), accumulated in fp64 from +0.0", "pool scratch that is released on every path",
                   "one workgroup adds the partials in a fixed order", "depends on (counts, T) alone", "the same at every alignment",
                   "f32(sqrt(S)): ONE rounding of an fp64 value", "f32(min(1, max_norm / ((double) dev_out2[0] + 1e-6)))",
                   "1 when max_norm is +Inf and the norm is finite", "S is NaN exactly when an element is NaN", "norm NaN: the coefficient is NaN",
                   "norm +Inf: the coefficient is 0, or NaN when max_norm is +Inf too", "no host read"):
        assert phrase.lower() in block.lower(), phrase


def test_every_refusal_comes_back_before_any_device_work():
    """No GPU here: a call that got as far as the device would report that instead of NP_ERR_INVALID's message."""
    from numpower_amd import _lib
    lib = _lib.load()
    A = [k << 24 for k in range(1, 9)]                                   # far apart, never dereferenced
    p2, g2, b2, v2, n2 = _ptrs(A[0], A[1]), _ptrs(A[2], A[3]), _ptrs(A[4], A[5]), _ptrs(A[6], A[7]), _counts(5, 9)
    scale = C.c_void_p(9 << 24)
    refused = lambda rc, text: rc == NP_ERR_INVALID and text in lib.np_last_error()

    def sgd(p=p2, g=g2, b=b2, n=n2, T=2, lr=0.1, mu=0.9, damp=0.0, wd=0.0, nest=0, first=0, s=None):
        return lib.np_sgd_step(p, g, b, n, T, lr, mu, damp, wd, nest, first, s)

    def adam(p=p2, g=g2, m=b2, v=v2, n=n2, T=2, step=1, lr=1e-3, b1=0.9, b2_=0.999, eps=1e-8, wd=0.0, dec=0, s=None):
        return lib.np_adam_step(p, g, m, v, n, T, step, lr, b1, b2_, eps, wd, dec, s)

    # pointers: a null list, a null required pointer
    for kw in (dict(p=None), dict(g=None), dict(b=None), dict(n=None)):
        assert refused(sgd(**kw), b"null pointer (a list)")
    assert refused(sgd(p=_ptrs(A[0], None)), b"null pointer (tensor 1)") and refused(sgd(g=_ptrs(None, A[3])), b"null pointer (tensor 0)")
    assert refused(sgd(b=_ptrs(A[4], None)), b"null pointer (tensor 1)")
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=None)):
        assert refused(adam(**kw), b"null pointer (a list)")
    assert refused(adam(m=_ptrs(None, A[5])), b"null pointer (tensor 0)") and refused(adam(v=_ptrs(A[6], None)), b"null pointer (tensor 1)")
    # pointers before extents before parameters
    assert refused(sgd(p=None, T=0, lr=-1.0), b"null pointer") and refused(sgd(T=0, lr=-1.0), b"the list is empty")
    assert refused(adam(T=0, step=0), b"the list is empty")
    assert refused(sgd(n=_counts(5, 0), lr=-1.0), b"tensor 1 has no elements") and refused(adam(n=_counts(0, 5)), b"tensor 0 has no elements")
    assert refused(sgd(n=_counts(5, 1 << 62)), b"does not fit")
    # parameters
    for bad in (-1e-3, -INF, INF, NAN):
        assert refused(sgd(lr=bad), b"lr must be finite and not negative") and refused(adam(lr=bad), b"lr must be finite and not negative")
        assert refused(sgd(wd=bad), b"weight_decay must be finite and not negative") and refused(adam(wd=bad), b"weight_decay must be finite")
        assert refused(adam(eps=bad), b"eps must be finite and not negative")
    for bad in (-0.1, 1.0001, INF, NAN):
        assert refused(sgd(mu=bad), b"momentum must lie in [0, 1]") and refused(sgd(damp=bad), b"dampening must lie in [0, 1]")
    assert refused(sgd(mu=0.0, b=None, nest=1), b"nesterov needs a momentum and zero dampening") and refused(sgd(damp=0.1, nest=1), b"nesterov needs")
    for bad in (-0.1, 1.0, 1.5, NAN):
        assert refused(adam(b1=bad), b"the betas must lie in [0, 1)") and refused(adam(b2_=bad), b"the betas must lie in [0, 1)")
    for bad in (0, -1, -(1 << 40)):
        assert refused(adam(step=bad), b"step must be at least 1")
    assert refused(sgd(lr=-1.0, p=_ptrs(A[0], A[0])), b"lr must be")                       # parameters before aliasing
    # aliasing: no written range may meet another range; two gradients may share memory (that call would go on to the device)
    over = b"overlaps"
    assert refused(sgd(p=_ptrs(A[0], A[0])), over) and refused(sgd(p=_ptrs(A[0], A[0] + 16)), over)          # 5 floats: 20 bytes
    assert refused(sgd(g=_ptrs(A[0], A[3])), over) and refused(sgd(g=_ptrs(A[2], A[1] + 32)), over)          # a gradient inside a parameter
    assert refused(sgd(b=_ptrs(A[0] + 4, A[5])), over) and refused(sgd(b=_ptrs(A[4], A[4] + 16)), over) and refused(sgd(b=_ptrs(A[3], A[5])), over)
    assert refused(sgd(s=C.c_void_p(A[1] + 32)), over) and refused(sgd(s=C.c_void_p(A[4])), over)            # grad_scale inside a written range
    assert refused(adam(v=_ptrs(A[6], A[4])), over) and refused(adam(m=_ptrs(A[4], A[2] + 8)), over) and refused(adam(v=_ptrs(A[1] + 35 , A[7])), over)
    assert refused(adam(p=_ptrs(A[0], A[2])), over) and refused(adam(s=C.c_void_p(A[6] + 16)), over)
    assert refused(sgd(mu=0.0, b=_ptrs(A[0], A[1]), lr=-1.0), b"lr must be")                 # without a momentum the buffers are not looked at ...
    # the norm
    norm = lambda g=g2, n=n2, T=2, mx=1.0, out=scale: lib.np_grad_norm(g, n, T, mx, out)
    assert refused(norm(g=None), b"null pointer") and refused(norm(n=None), b"null pointer") and refused(norm(out=None), b"null pointer")
    assert refused(norm(g=_ptrs(A[2], None)), b"null pointer (tensor 1)") and refused(norm(T=0), b"the list is empty")
    assert refused(norm(n=_counts(0, 1)), b"tensor 0 has no elements")
    for bad in (-1.0, -INF, NAN):
        assert refused(norm(mx=bad), b"max_norm must not be negative")
    assert refused(norm(out=C.c_void_p(A[3] + 32)), b"the result overlaps a gradient") and refused(norm(out=C.c_void_p(A[2] - 4)), b"overlaps")
    launches, chunks, vec, scalar = C.c_int(-7), C.c_size_t(7), C.c_int(-7), C.c_int(-7)
    assert lib.np_debug_optim_last_path(C.byref(launches), C.byref(chunks), C.byref(vec), C.byref(scalar)) == _lib.NP_OK and launches.value == 0

    src = (ROOT / "numpower_amd" / "csrc" / "np_optim.hip").read_text()
    for name, params in (("int np_sgd_step(", ("lr must be", "weight_decay must be", "momentum must lie", "dampening must lie", "nesterov needs")),
                         ("int np_adam_step(", ("lr must be", "weight_decay must be", "eps must be", "the betas must", "step must be"))):
        body = _function(src, name)                   # pointers and extents, parameters, aliasing, then work
        order = [body.index(s) for s in ("check_list(",) + params + ("check_aliasing(", "ensure_init()", "launch_steps<")]
        assert order == sorted(order), name
        assert "<<<" not in body and "alloc" not in body
    body = _function(src, "int check_list(")
    assert body.index("null pointer (a list)") < body.index("null pointer (tensor") < body.index("the list is empty") < body.index("has no elements")
    assert "ensure_init" not in body and "hip" not in body
    body = _function(src, "int np_grad_norm(")
    assert body.index("null pointer") < body.index("the list is empty") < body.index("max_norm must") < body.index("written_overlap(") \
        < body.index("ensure_init()") < body.index("partial.alloc(") < body.index("<<<")
    assert "std::sort" in _function(src, "bool written_overlap(")


def test_the_family_restates_the_dispatcher():
    src = (ROOT / "numpower_amd" / "csrc" / "np_optim.hip").read_text()
    mode = _function(src, "unsigned char mode_of(")
    assert "const uintptr_t r = (uintptr_t)p & 15;" in mode and "return (unsigned char)(r / 4);" in mode and "g_optim_force_scalar ||" in mode
    launch = _function(src, "int launch_steps(")
    for line in ("const size_t o = L.mode[j] == kModeScalar ? 0 : L.mode[j];", "L.first[j + 1] = L.first[j] + ceil_div(o + counts[t], kChunk);"):
        assert line in launch, line
    assert "L.first[j + 1] = L.first[j] + ceil_div(counts[t0 + j], kNormChunk);" in _function(src, "int np_grad_norm(")
    assert "if (wanted <= cap) return wanted < 1 ? 1 : wanted;" in (ROOT / "numpower_amd" / "csrc" / "np_internal.h").read_text()


def test_host_and_glue_declare_the_functions():
    from numpower_amd import ndarray
    host = _header("numpower_host.h")
    assert ("int NDArrayDNN_SGD_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **bufs, int n_bufs, double lr, double momentum, "
            "double dampening, double weight_decay, int nesterov, int first_step, NDArray *grad_scale, int grad_scale_index);") in host
    assert "NDArray *NDArrayDNN_GradNorm(NDArray **grads, int n_grads, double max_norm);" in host and "int NDArrayDNN_Adam_Step(NDArray **params" in host
    h = ndarray._load_host()
    assert all(hasattr(h, n) for n in ("NDArrayDNN_SGD_Step", "NDArrayDNN_Adam_Step", "NDArrayDNN_GradNorm", "NPH_SGD_Step", "NPH_Adam_Step", "NPH_GradNorm"))
    glue = _header("hip_dnn.h", "ext")
    assert "int NPH_SGD_Step(struct NDArray **params, int n_params," in glue and "int NPH_Adam_Step(struct NDArray **params, int n_params," in glue
    assert "struct NDArray *NPH_GradNorm(struct NDArray **grads, int n_grads, double max_norm);" in glue
    src = (ROOT / "ext" / "hip_dnn.c").read_text()
    checks = _function(src, "static int optim_of(")
    order = [checks.index("NPH_OPTIM_MSG_" + n) for n in ("LENGTHS", "NULL", "EMPTY_LIST", "EMPTY", "COUNT", "SCALE", "DEVICE", "CPU")]
    assert order == sorted(order) and checks.index("np_ext_throw(refusal)") < checks.index("NPH_OPTIM_MSG_DEVICE") and "np_sgd_step" not in checks
    for name, call in (("int NPH_SGD_Step(", "np_sgd_step("), ("int NPH_Adam_Step(", "np_adam_step("), ("NDArray *NPH_GradNorm(", "np_grad_norm(")):
        body = _function(src, name)
        assert body.index("optim_of(") < body.index(call) < body.rindex("optim_release(&o);")       # the block is released on every path
    cpp = (ROOT / "numpower_amd" / "host" / "numpower_dnn.cpp").read_text()
    for name, call in (("int NDArrayDNN_SGD_Step(", "NPH_SGD_Step("), ("int NDArrayDNN_Adam_Step(", "NPH_Adam_Step("), ("NDArray *NDArrayDNN_GradNorm(", "NPH_GradNorm(")):
        body = _function(cpp, name)
        assert "OptimLists l;" in body and call in body
    assert "NPH_OPTIM_MSG_VIEW" in _function(cpp, "struct OptimLists {")
    tool = (ROOT / "tools" / "apply_with_hip.py").read_text()
    assert "Optim" not in tool and "optim" not in tool and "SGD" not in tool      # the reference has no optimizer: no anchored edit


def test_each_message_is_raised_with_its_text():
    """CPU operands: the device checks come last, so every message before them needs no device."""
    from numpower_amd.ndarray import NDArray, Error
    raw = re.sub(r'"\s*\n\s*"', "", (ROOT / "ext" / "hip_dnn.h").read_text())
    for name, text in MESSAGES.items():
        assert '#define %s "%s"' % (name, text) in raw, name
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    sgd, adam, norm = NDArray.dnn_sgd_step, NDArray.dnn_adam_step, NDArray.dnn_grad_norm

    def message(fn, *a, **kw):
        with pytest.raises(Error) as e:
            fn(*a, **kw)
        return str(e.value)

    M = lambda n: MESSAGES["NPH_OPTIM_MSG_" + n]
    P, G, S1, S2 = ([ones(3), ones(2, 2)] for _ in range(4))
    assert message(sgd, P, G[:1], 0.1) == M("LENGTHS") and message(sgd, P, G, 0.1, 0.9, buffers=S1[:1]) == M("LENGTHS")
    assert message(adam, P, G, S1[:1], S2, 1) == M("LENGTHS") and message(adam, P, G, S1, S2 + [ones(1)], 1) == M("LENGTHS")
    assert message(sgd, [], [], 0.1) == M("EMPTY_LIST") and message(adam, [], [], [], [], 1) == M("EMPTY_LIST") and message(norm, []) == M("EMPTY_LIST")
    assert message(sgd, P, G, 0.1, 0.9) == M("BUFFERS") and message(sgd, P, G, 0.1, momentum=0.5, nesterov=True) == M("BUFFERS")
    empty = NDArray.array(np.ones((0, 3), np.float32))
    assert message(sgd, [empty], [empty], 0.1) == M("EMPTY") and message(norm, [ones(2), empty]) == M("EMPTY")
    assert message(adam, P, G, [ones(3), empty], S2, 1) == M("EMPTY")
    assert message(sgd, P, [ones(3), ones(5)], 0.1) == M("COUNT") and message(adam, P, G, S1, [ones(4), ones(4)], 1) == M("COUNT")
    assert message(sgd, P, G, 0.1, 0.9, buffers=[ones(3), ones(3)]) == M("COUNT")
    sgd_ok = lambda **kw: message(sgd, P, [ones(3), ones(4)], kw.pop("lr", 0.1), buffers=S1, **kw)          # the shapes are not compared: (2, 2) and (4)
    for idx in (-1, 2, 7):
        assert sgd_ok(grad_scale=(ones(2), idx)) == M("SCALE")
    for bad in (-0.1, INF, NAN):
        assert sgd_ok(lr=bad) == M("LR") and sgd_ok(weight_decay=bad) == M("WEIGHT_DECAY")
        assert message(adam, P, G, S1, S2, 1, lr=bad) == M("LR") and message(adam, P, G, S1, S2, 1, weight_decay=bad) == M("WEIGHT_DECAY")
        assert message(adam, P, G, S1, S2, 1, eps=bad) == M("EPS")
    for bad in (-0.1, 1.5, NAN):
        assert sgd_ok(momentum=bad) == M("MOMENTUM") and sgd_ok(momentum=0.5, dampening=bad) == M("DAMPENING")
        assert message(adam, P, G, S1, S2, 1, betas=(bad, 0.9)) == M("BETAS") and message(adam, P, G, S1, S2, 1, betas=(0.9, bad)) == M("BETAS")
    assert message(adam, P, G, S1, S2, 1, betas=(0.9, 1.0)) == M("BETAS")
    assert sgd_ok(nesterov=True) == M("NESTEROV") and sgd_ok(momentum=0.9, dampening=0.1, nesterov=True) == M("NESTEROV")
    for bad in (0, -3):
        assert message(adam, P, G, S1, S2, bad) == M("STEP")
    for bad in (-1.0, NAN):
        assert message(norm, G, bad) == M("MAX_NORM")
    assert sgd_ok(lr=-1.0, momentum=7.0) == M("LR")                                         # in the order of the header
    # the right operands get as far as the device check
    assert sgd_ok() == M("CPU") and sgd_ok(momentum=0.9, nesterov=True) == M("CPU") and message(sgd, P, G, 0.1) == M("CPU")
    assert message(adam, P, G, S1, S2, 1) == M("CPU") and message(adam, P, G, S1, S2, 3, decoupled=True, weight_decay=0.1, grad_scale=ones(1)) == M("CPU")
    assert message(norm, G) == M("CPU") and message(norm, G, INF) == M("CPU")
    # the binding's own argument checks
    assert message(sgd, P, G, "fast") == "dnn_sgd_step: lr must be a number" and message(sgd, P, G, 0.1, momentum=True) == "dnn_sgd_step: momentum must be a number"
    assert message(sgd, P[0], G, 0.1) == "dnn_sgd_step: params must be a list of arrays" and message(sgd, P, [1.0, 2.0], 0.1) == "dnn_sgd_step: grads must be a list of arrays"
    assert message(sgd, P, G, 0.1, 0.9, buffers=[None, None]) == "dnn_sgd_step: buffers must be a list of arrays"
    assert message(sgd, P, G, 0.1, grad_scale=1.0) == "dnn_sgd_step: grad_scale must be an array, (array, index) or None"
    assert message(adam, P, G, S1, S2, 1.5) == "dnn_adam_step: step must be an int" and message(adam, P, G, S1, S2, 1, betas=0.9) == "dnn_adam_step: betas must be a pair of numbers"
    assert message(adam, P, G, None, S2, 1) == "dnn_adam_step: exp_avg must be a list of arrays"
    assert message(norm, G, "one") == "dnn_grad_norm: max_norm must be a number" and message(norm, G[0]) == "dnn_grad_norm: grads must be a list of arrays"


def test_optim_py_checks_its_arguments():
    from numpower_amd import optim
    from numpower_amd.ndarray import NDArray, Error
    ones = lambda *s: NDArray.array(np.ones(s, np.float32))
    for cls in (optim.SGD, optim.Adam, optim.AdamW):
        for bad in (None, [], ones(3), [ones(3), 1.0]):
            with pytest.raises(Error, match="params must be a non-empty list of arrays"):
                cls(bad)
        with pytest.raises(Error, match="lr must be a number"):
            cls([ones(3)], lr="fast")
    for kw in (dict(lr=-1.0), dict(momentum=1.5), dict(dampening=-0.5), dict(weight_decay=-1.0)):
        with pytest.raises(Error, match="SGD: lr and weight_decay must not be negative"):
            optim.SGD([ones(3)], **kw)
    for kw in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.5)):
        with pytest.raises(Error, match="SGD: nesterov needs a momentum and zero dampening"):
            optim.SGD([ones(3)], **kw)
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(Error, match="betas must be a pair of numbers"):
            cls([ones(3)], betas=0.9)
        for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(weight_decay=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1))):
            with pytest.raises(Error, match="the betas must lie in"):
                cls([ones(3)], **kw)
    s = optim.SGD([ones(3), ones(2, 2)], lr=0.1)                                            # no momentum: no state, no device
    assert s.buffers is None and s.steps == 0 and s.last_norm is None
    for bad in (None, [ones(3)], ones(3)):
        with pytest.raises(Error, match="grads must be a list with one gradient per parameter"):
            s.step(bad)
    with pytest.raises(Error, match="max_norm must be a number"):
        s.step([ones(3), ones(4)], max_norm="one")
    with pytest.raises(Error, match="operands are on the CPU"):                             # a CPU list gets as far as the glue's device check
        s.step([ones(3), ones(4)])
    assert s.steps == 0
    import inspect
    assert list(inspect.signature(optim.SGD.__init__).parameters)[1:] == ["params", "lr", "momentum", "dampening", "weight_decay", "nesterov"]
    assert list(inspect.signature(optim.AdamW.__init__).parameters)[1:] == ["params", "lr", "betas", "eps", "weight_decay"]
    assert inspect.signature(optim.AdamW.__init__).parameters["weight_decay"].default == 1e-2       # torch's defaults
    assert inspect.signature(optim.Adam.__init__).parameters["weight_decay"].default == 0.0
    for name in ("param_groups", "state_dict", "amsgrad", "maximize"):
        assert not hasattr(optim.Adam, name)
