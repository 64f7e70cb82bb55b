"""Python stand-in for the PHP `NDArray` class surface on the hot path.

PHP is not available where this was built, so the Zend glue (numpower.c) cannot be compiled;
this module plays its role for tests and benchmarks: it marshals Python values the way
ZVAL_TO_NDARRAY does (numpower.c:89-117), calls the SAME host entry points the PHP_METHODs call
(libnumpower_host.so: NDArray_Add_Float, reduce, NDArray_Matmul, NDArray_ToGPU ...), frees
temporaries like CHECK_INPUT_AND_FREE (numpower.c:119-135) and converts results like
RETURN_NDARRAY (numpower.c:137-150: ndim > 0 -> NDArray object, ndim == 0 -> float).

    a = NDArray.array([[1, 2], [3, 4]]).gpu()
    c = (a + 2) * a[0]
    NDArray.sum(c, axis=0).cpu().toArray()

All arithmetic runs in the HIP library.  Operating on CPU-resident arrays raises `Error` (the
reference's CPU path is not re-implemented here and nothing falls back to numpy).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import BINARY_OPS, UNARY_OPS

CPU, GPU = 0, 1

# NP_LAZY_BINDING=1 (or NDArray.set_lazy_binding(True)): this stand-in then behaves like a `--with-hip` tree with INTEGRATION.md 2c
# applied — the arithmetic operators / static arithmetic methods / unary methods call the appenders of ext/hip_lazy.c
# (NPH_LazyBinary, NPH_LazyElementWise*), the full reductions NPH_ReduceAll, and EVERY other use of an array's pointer goes through
# the marshalling point (`_p` = buffer_get: NPH_OnBufferGet computes pending values first).  Off by default: the mirror is then the
# 2a + 2b tree (one launch per op) and `$a->lazy()` (numpower_amd/lazy.py) is the explicit form.  Running the whole GPU suite with
# the switch on is the flush-set test of the mirror: every method that is not an appender must see finished values.
import os as _os
_LAZY_BINDING = _os.environ.get("NP_LAZY_BINDING") == "1"
_LAZY_ARITH = ("add", "subtract", "multiply", "divide", "mod", "pow")


_libc_free = C.CDLL(None).free
_libc_free.argtypes = [C.c_void_p]
_libc_free.restype = None


class Error(RuntimeError):
    """PHP `Error` thrown by zend_throw_error in the reference."""


class _CNDArrayDescriptor(C.Structure):
    _fields_ = [("type", C.c_char_p), ("elsize", C.c_int), ("numElements", C.c_long)]


class _CNDArray(C.Structure):
    pass


_CNDArray._fields_ = [
    ("uuid", C.c_int), ("strides", C.POINTER(C.c_int)), ("dimensions", C.POINTER(C.c_int)),
    ("ndim", C.c_int), ("data", C.c_void_p), ("base", C.POINTER(_CNDArray)), ("flags", C.c_int),
    ("descriptor", C.POINTER(_CNDArrayDescriptor)), ("iterator", C.c_void_p),
    ("php_iterator", C.c_void_p), ("refcount", C.c_int), ("device", C.c_int)]

_P = C.POINTER(_CNDArray)
_host = None


class _CDims(C.Structure):   # NDArray_Dims, src/ndarray.h:40-43
    _fields_ = [("ptr", C.POINTER(C.c_int)), ("len", C.c_int)]


def host_lib_path() -> Path:
    return _lib.LIBDIR / "libnumpower_host.so"


def _load_host():
    global _host
    if _host is not None:
        return _host
    _lib.load()   # libnp_hip.so first (RTLD_GLOBAL)
    path = host_lib_path()
    if not path.exists():
        raise Error(f"{path} is missing: run `python -m numpower_amd.build` (no CPU fallback)")
    h = C.CDLL(str(path))
    ip = C.POINTER(C.c_int)
    fp = C.POINTER(C.c_float)
    sig = {
        "numpower_host_last_error": (C.c_char_p, []),
        "numpower_host_clear_error": (None, []),
        "NDArray_Zeros": (_P, [ip, C.c_int, C.c_char_p, C.c_int]),
        "NDArray_Empty": (_P, [ip, C.c_int, C.c_char_p, C.c_int]),
        "NDArray_Copy": (_P, [_P, C.c_int]),
        "NDArray_Fill": (_P, [_P, C.c_float]),
        "NDArray_CreateFromDoubleScalar": (_P, [C.c_double]),
        "NDArray_CreateFromLongScalar": (_P, [C.c_long]),
        "NDArray_FromHostBuffer": (_P, [fp, ip, C.c_int]),
        "NDArray_LeadingSlice": (_P, [_P, C.c_int]),
        "NDArray_FREE": (None, [_P]),
        "NDArray_ToGPU": (_P, [_P]),
        "NDArray_ToCPU": (_P, [_P]),
        "NDArray_GetFloatScalar": (C.c_float, [_P]),
        "NDArray_CopyToHostBuffer": (C.c_int, [_P, fp]),
        "NDArray_LiveDeviceAllocations": (C.c_long, []),
        "NDArray_IsBroadcastable": (C.c_int, [_P, _P]),
        # reference signatures (cuda_math.h:10-15,75-76): the op is a cuda_float_* FUNCTION POINTER
        "NDArrayMathGPU_ElementWise": (_P, [_P, C.c_void_p]),
        "NDArrayMathGPU_ElementWise1F": (_P, [_P, C.c_void_p, C.c_float]),
        "NDArrayMathGPU_ElementWise2F": (_P, [_P, C.c_void_p, C.c_float, C.c_float]),
        "NDArrayMathGPU_ElementWise1N": (_P, [_P, C.c_void_p, _P]),
        "NDArray_Abs": (_P, [_P]),
        "NDArray_Rsqrt": (_P, [_P]),
        "NDArray_Exp2": (_P, [_P]),
        "NDArray_Sum_Float": (C.c_float, [_P]),
        "NDArray_Float_Prod": (C.c_float, [_P]),
        "NDArray_Mean_Float": (C.c_float, [_P]),
        "NDArray_Median_Float": (C.c_float, [_P]),
        "NDArray_Quantile": (_P, [_P, _P]),
        "NDArray_Min": (C.c_float, [_P]),
        "NDArray_Max": (C.c_float, [_P]),
        "NDArray_MinAxis": (_P, [_P, C.c_int]),
        "NDArray_MaxAxis": (_P, [_P, C.c_int]),
        "NDArray_Matmul": (_P, [_P, _P]),
        "NDArray_Dot": (_P, [_P, _P]),
        "NDArray_Outer": (_P, [_P, _P]),
        "NDArray_Inner": (_P, [_P, _P]),
        "NDArray_BatchedMatmul": (_P, [_P, _P]),
        "NDArray_ShardedBatchedMatmul": (_P, [_P, _P, C.c_int, C.c_int]),
        "NDArray_CommInit": (C.c_int, [C.c_int, C.c_int, C.c_char_p]),
        "NDArray_CommDestroy": (C.c_int, []),
        "NDArray_CommRank": (C.c_int, []),
        "NDArray_CommWorld": (C.c_int, []),
    }
    for name in ("Add", "Subtract", "Multiply", "Divide", "Mod", "Pow"):
        sig[f"NDArray_{name}_Float"] = (_P, [_P, _P])
    for name in ("Equal", "NotEqual", "Greater", "GreaterEqual", "Less", "LessEqual", "Maximum", "Minimum"):
        sig[f"NDArray_{name}"] = (_P, [_P, _P])
    sig["NDArray_All"] = (C.c_float, [_P])
    sig["NDArray_Transpose"] = (_P, [_P, C.POINTER(_CDims)])
    sig["NDArray_ArgMinMaxCommon"] = (_P, [_P, C.c_int, C.c_bool, C.c_bool])
    sig["NDArray_Variance"] = (_P, [_P])
    sig["NDArray_Std"] = (_P, [_P])
    sig["NDArray_Average"] = (_P, [_P, _P])
    sig["NDArray_FullOn"] = (_P, [ip, C.c_int, C.c_double, C.c_int])
    sig["NDArray_IdentityOn"] = (_P, [C.c_int, C.c_int])
    sig["NDArray_ArangeOn"] = (_P, [C.c_double, C.c_double, C.c_double, C.c_int])
    sig["NDArray_ArrayEqual"] = (C.c_int, [_P, _P])
    sig["NDArray_AllClose"] = (C.c_int, [_P, _P, C.c_float, C.c_float])
    sig["NDArray_ToContiguous"] = (_P, [_P])
    sig["NDArray_Diagonal"] = (_P, [_P, C.c_int])
    sig["NDArray_Trace"] = (_P, [_P])
    sig["NDArray_Det"] = (_P, [_P])
    sig["NDArray_Inverse"] = (_P, [_P])
    sig["NDArray_LU"] = (C.POINTER(_P), [_P])
    sig["NDArray_Solve"] = (_P, [_P, _P])
    sig["NDArray_Cholesky"] = (_P, [_P])
    sig["NDArray_Correlate2D"] = (_P, [_P, _P, C.c_int, C.c_int, _P, C.c_int])
    sig["NDArrayDNN_Conv2D_Forward"] = (_P, [_P, _P, ip, C.c_char, C.c_int])
    sig["NDArrayDNN_Conv2D_Backward"] = (C.POINTER(_P), [_P, _P, _P, C.c_int, C.c_char, C.c_int])
    sig["NDArrayDNN_Conv2D_ForwardEx"] = (_P, [_P, _P, ip, ip, ip])
    sig["NDArrayDNN_Conv2D_BackwardEx"] = (C.POINTER(_P), [_P, _P, _P, ip, ip, ip])
    sig["NDArrayDNN_Conv2D_LayerForward"] = (_P, [_P, _P, _P, ip, ip, ip, C.c_char])
    sig["NDArrayDNN_Conv2D_LayerBackward"] = (C.POINTER(_P), [_P, _P, _P, _P, ip, ip, ip, C.c_char, C.c_int])
    sig["NDArrayDNN_Pool2D_Forward"] = (_P, [_P, ip, ip, ip, C.c_char])
    sig["NDArrayDNN_Pool2D_Backward"] = (_P, [_P, _P, ip, ip, ip, C.c_char])
    sig["NDArrayDNN_Softmax_Forward"] = (_P, [_P, C.c_int, C.c_char])
    sig["NDArrayDNN_Softmax_Backward"] = (_P, [_P, _P, C.c_int, C.c_char])
    sig["NDArrayDNN_CrossEntropy"] = (_P, [_P, _P, C.c_char, C.c_int, C.POINTER(_P)])
    sig["NDArrayDNN_BatchNorm_Forward"] = (C.POINTER(_P), [_P] * 5 + [C.c_int, C.c_double, C.c_double])
    sig["NDArrayDNN_BatchNorm_Backward"] = (C.POINTER(_P), [_P] * 5)
    sig["NDArrayDNN_LayerNorm_Forward"] = (C.POINTER(_P), [_P, ip, C.c_int, _P, _P, C.c_double])
    sig["NDArrayDNN_LayerNorm_Backward"] = (C.POINTER(_P), [_P, _P, ip, C.c_int, _P, _P, _P])
    sig["NDArrayDNN_GroupNorm_Forward"] = (C.POINTER(_P), [_P, C.c_int, _P, _P, C.c_double])
    sig["NDArrayDNN_GroupNorm_Backward"] = (C.POINTER(_P), [_P, _P, C.c_int, _P, _P, _P])
    sig["NDArrayDNN_Attention_Forward"] = (C.POINTER(_P), [_P, _P, _P, C.c_int, C.c_float])
    sig["NDArrayDNN_Attention_Backward"] = (C.POINTER(_P), [_P] * 7 + [C.c_int, C.c_float])
    pp = C.POINTER(_P)
    sig["NDArrayDNN_SGD_Step"] = (C.c_int, [pp, C.c_int] * 3 + [C.c_double] * 4 + [C.c_int, C.c_int, _P, C.c_int])
    sig["NDArrayDNN_Adam_Step"] = (C.c_int, [pp, C.c_int] * 4 + [C.c_long] + [C.c_double] * 5 + [C.c_int, _P, C.c_int])
    sig["NDArrayDNN_GradNorm"] = (_P, [pp, C.c_int, C.c_double])
    sig["NDArrayDNN_Linear_Forward"] = (_P, [_P, _P, _P, C.c_char])
    sig["NDArrayDNN_Linear_Backward"] = (C.POINTER(_P), [_P, _P, _P, _P, C.c_char, C.c_int, C.c_int])
    sig["NDArray_SVD"] = (C.POINTER(_P), [_P])
    sig["NDArray_Eig"] = (C.POINTER(_P), [_P])
    sig["NDArray_Qr"] = (C.POINTER(_P), [_P])
    sig["NDArray_Lstsq"] = (_P, [_P, _P])
    sig["NDArray_MatrixRank"] = (_P, [_P, fp])
    sig["NDArray_Norm"] = (_P, [_P, C.c_int])
    sig["NDArray_Cond"] = (_P, [_P])
    sig["NDArray_Reshape"] = (_P, [_P, ip, C.c_int])
    sig["NDArray_Flatten"] = (_P, [_P])
    sig["NDArray_ExpandDim"] = (_P, [_P, _P])
    sig["NDArray_Append"] = (_P, [C.POINTER(_P), C.c_int, C.c_int])
    for name in ("NDArray_AtLeast1D", "NDArray_AtLeast2D", "NDArray_AtLeast3D", "NDArray_Diag"):
        sig[name] = (_P, [_P])
    sig["NDArray_Squeeze"] = (_P, [_P, _P])
    sig["NDArray_SwapAxes"] = (_P, [_P, C.c_int, C.c_int])
    sig["NDArray_Rollaxis"] = (_P, [_P, C.c_int, C.c_int])
    sig["NDArray_Moveaxis"] = (_P, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int])
    sig["NDArray_Concatenate"] = (_P, [C.POINTER(_P), C.c_int, C.c_int])
    for name in ("NDArray_VSTACK", "NDArray_HSTACK", "NDArray_DSTACK", "NDArray_ColumnStack"):
        sig[name] = (_P, [C.POINTER(_P), C.c_int])
    sig["NDArray_Slice"] = (_P, [_P, C.POINTER(_P), C.c_int])
    # ext/hip_lazy.c
    sig["NPH_LazyBinary"] = (_P, [C.c_int, C.c_void_p, _P, _P])
    sig["NPH_LazyElementWise"] = (_P, [_P, C.c_void_p])
    sig["NPH_LazyElementWise1F"] = (_P, [_P, C.c_void_p, C.c_float])
    sig["NPH_LazyElementWise2F"] = (_P, [_P, C.c_void_p, C.c_float, C.c_float])
    sig["NPH_ReduceAll"] = (C.c_float, [C.c_int, C.c_void_p, _P])
    sig["NPH_OnBufferGet"] = (None, [_P])
    sig["NPH_Flush"] = (C.c_int, [_P])
    sig["NPH_IsPending"] = (C.c_int, [_P])
    sig["NPH_PendingCount"] = (C.c_int, [])
    for name, (res, args) in sig.items():
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = args
    # reduce(array, int *axis, operation): the operation is passed as the address of the
    # library's own NDArray_Add_Float / NDArray_Multiply_Float, exactly as numpower.c does.
    h.reduce.restype = _P
    h.reduce.argtypes = [_P, C.POINTER(C.c_int), C.c_void_p]
    _host = h
    return h


def _fn(h, symbol):
    """Address of one of the library's own functions, passed where numpower.c passes the function name
    (`NDArrayMathGPU_ElementWise(nda, cuda_float_sin)`, numpower.c:1651)."""
    return C.cast(getattr(h, symbol), C.c_void_p)


def _raise_pending(h, what="call"):
    msg = h.numpower_host_last_error()
    text = msg.decode() if msg else ""
    h.numpower_host_clear_error()
    raise Error(text or f"{what} failed")


_BINARY_FN = {"add": "NDArray_Add_Float", "subtract": "NDArray_Subtract_Float",
              "multiply": "NDArray_Multiply_Float", "divide": "NDArray_Divide_Float",
              "mod": "NDArray_Mod_Float", "pow": "NDArray_Pow_Float",
              # comparison family (src/logic.c), PHP methods equal / not_equal / greater / ...
              "equal": "NDArray_Equal", "not_equal": "NDArray_NotEqual", "greater": "NDArray_Greater",
              "greater_equal": "NDArray_GreaterEqual", "less": "NDArray_Less",
              "less_equal": "NDArray_LessEqual",
              "maximum": "NDArray_Maximum", "minimum": "NDArray_Minimum"}

# PHP method name -> np_unary_op for the plain NDArrayMathGPU_ElementWise family
# (method table numpower.c:5136-5174)
_UNARY_METHODS = [n for n in UNARY_OPS if n not in ("clip", "round")]


class NDArray:
    """Handle on a C `NDArray*` owned by libnumpower_host.so (PHP objects hold a uuid into
    MAIN_MEM_STACK instead, buffer.c:91-120; the ownership rules are the same: the object's
    destructor calls NDArray_FREE, views keep their base alive through the refcount)."""

    __slots__ = ("_ptr", "_h")

    def __init__(self, ptr):
        self._h = _load_host()
        if not ptr:
            _raise_pending(self._h)
        self._ptr = ptr

    @property
    def _p(self):
        """The marshalling point (ZVAL_TO_NDARRAY -> buffer_get, numpower.c:105, src/buffer.c:80): with the lazy binding on, a pending
        value is computed here, and so are the chains that read this array (the consumer may write it).  Appenders use _ptr."""
        p = self._ptr
        if _LAZY_BINDING and p:
            self._h.NPH_OnBufferGet(p)
            if self._h.numpower_host_last_error():
                _raise_pending(self._h)
        return p

    @_p.setter
    def _p(self, value):
        self._ptr = value

    @staticmethod
    def set_lazy_binding(on: bool):
        global _LAZY_BINDING
        _LAZY_BINDING = bool(on)

    def __del__(self):
        try:
            if self._ptr:
                self._h.NDArray_FREE(self._ptr)      # ndarray_destructor -> buffer_ndarray_free: no flush on the way out
                self._ptr = None
        except Exception:
            pass

    # ---- marshalling (ZVAL_TO_NDARRAY, numpower.c:89-117) ---------------------------------
    @staticmethod
    def _coerce(value):
        """-> (NDArray, is_temporary)"""
        if isinstance(value, NDArray):
            return value, False
        h = _load_host()
        if isinstance(value, bool):
            raise Error("argument must be an array, long, double, gdimage or ndarray.")
        if isinstance(value, int):
            return NDArray(h.NDArray_CreateFromLongScalar(value)), True
        if isinstance(value, float):
            return NDArray(h.NDArray_CreateFromDoubleScalar(value)), True
        if isinstance(value, (list, tuple, np.ndarray)):
            return NDArray.array(value), True
        raise Error("argument must be an array, long, double, gdimage or ndarray.")

    @staticmethod
    def _wrap(ptr):
        """RETURN_NDARRAY (numpower.c:137-150)."""
        h = _load_host()
        if not ptr:
            _raise_pending(h)
        if ptr.contents.ndim > 0:
            return NDArray(ptr)
        v = h.NDArray_GetFloatScalar(ptr)
        h.NDArray_FREE(ptr)
        return float(v)

    # ---- construction -----------------------------------------------------------------------
    @staticmethod
    def array(values) -> "NDArray":
        """NDArray::array — CPU array from a nested list (fp32)."""
        a = np.asarray(values, dtype=np.float32, order="C")
        h = _load_host()
        shape = (C.c_int * max(a.ndim, 1))(*a.shape)
        return NDArray(h.NDArray_FromHostBuffer(a.ctypes.data_as(C.POINTER(C.c_float)), shape, a.ndim))

    @staticmethod
    def zeros(shape, device=CPU) -> "NDArray":
        h = _load_host()
        s = (C.c_int * max(len(shape), 1))(*shape)
        return NDArray(h.NDArray_Zeros(s, len(shape), b"float32", device))

    # ---- placement ---------------------------------------------------------------------------
    @staticmethod
    def full(shape, fill_value, device=CPU) -> "NDArray":      # PHP_METHOD full, numpower.c:1214
        h = _load_host()
        arr = (C.c_int * max(len(shape), 1))(*[int(v) for v in shape])
        return NDArray(h.NDArray_FullOn(arr, len(shape), float(fill_value), device))

    @staticmethod
    def ones(shape, device=CPU) -> "NDArray":                  # numpower.c:1261
        return NDArray.full(shape, 1.0, device)

    @staticmethod
    def identity(size: int, device=CPU) -> "NDArray":          # numpower.c:940
        return NDArray(_load_host().NDArray_IdentityOn(int(size), device))

    @staticmethod
    def arange(stop, start=0.0, step=1.0, device=GPU) -> "NDArray":   # numpower.c:1284-1302: (stop, start, step)
        return NDArray(_load_host().NDArray_ArangeOn(float(start), float(stop), float(step), device))

    def gpu(self) -> "NDArray":
        """$a->gpu(): always a new array (NDArray_ToGPU, ndarray.c:1037-1068)."""
        return NDArray(self._h.NDArray_ToGPU(self._p))

    def cpu(self) -> "NDArray":
        return NDArray(self._h.NDArray_ToCPU(self._p))

    @staticmethod
    def setDevice(device_id: int) -> None:
        """NDArray::setDevice -> cudaSetDevice in the reference (numpower.c:615-635)."""
        _lib.check(_lib.load().np_set_device(int(device_id)))

    def isGPU(self) -> bool:
        return self._p.contents.device == GPU

    # ---- introspection -------------------------------------------------------------------------
    def shape(self):
        c = self._p.contents
        return [c.dimensions[i] for i in range(c.ndim)]

    def size(self) -> int:
        return int(self._p.contents.descriptor.contents.numElements)

    def ndim(self) -> int:
        return int(self._p.contents.ndim)

    def toArray(self):
        """toArray(): nested list of floats; throws for GPU arrays (numpower.c:456-477)."""
        return self.numpy().astype(np.float64).tolist()

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape(), dtype=np.float32)
        if self._h.NDArray_CopyToHostBuffer(self._p, out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            _raise_pending(self._h)
        return out

    def fill(self, value: float) -> "NDArray":
        if not self._h.NDArray_Fill(self._p, value):
            _raise_pending(self._h)
        return self

    def __getitem__(self, index: int) -> "NDArray":
        """$a[i]: view of slice i of the leading axis."""
        return NDArray._wrap(self._h.NDArray_LeadingSlice(self._p, int(index)))

    def __len__(self):
        return self.shape()[0]

    # ---- binary ops ------------------------------------------------------------------------------
    @staticmethod
    def _binary(name, a, b):
        h = _load_host()
        x, _tx = NDArray._coerce(a)
        y, _ty = NDArray._coerce(b)
        if _LAZY_BINDING and name in _LAZY_ARITH:     # ndarray_do_operation_ex / PHP_METHOD(add ...) as section 2c edits them
            return NDArray._wrap(h.NPH_LazyBinary(BINARY_OPS[name], _fn(h, _BINARY_FN[name]), x._ptr, y._ptr))
        return NDArray._wrap(getattr(h, _BINARY_FN[name])(x._p, y._p))

    add = staticmethod(lambda a, b: NDArray._binary("add", a, b))
    subtract = staticmethod(lambda a, b: NDArray._binary("subtract", a, b))
    multiply = staticmethod(lambda a, b: NDArray._binary("multiply", a, b))
    divide = staticmethod(lambda a, b: NDArray._binary("divide", a, b))
    mod = staticmethod(lambda a, b: NDArray._binary("mod", a, b))
    pow = staticmethod(lambda a, b: NDArray._binary("pow", a, b))
    equal = staticmethod(lambda a, b: NDArray._binary("equal", a, b))
    not_equal = staticmethod(lambda a, b: NDArray._binary("not_equal", a, b))
    greater = staticmethod(lambda a, b: NDArray._binary("greater", a, b))
    greater_equal = staticmethod(lambda a, b: NDArray._binary("greater_equal", a, b))
    less = staticmethod(lambda a, b: NDArray._binary("less", a, b))
    less_equal = staticmethod(lambda a, b: NDArray._binary("less_equal", a, b))
    maximum = staticmethod(lambda a, b: NDArray._binary("maximum", a, b))
    minimum = staticmethod(lambda a, b: NDArray._binary("minimum", a, b))

    @staticmethod
    def all(a) -> int:
        """PHP_METHOD(NDArray, all) without axis: RETURN_LONG(NDArray_All(nda)) (numpower.c:1330)."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        h.numpower_host_clear_error()
        v = h.NDArray_All(x._p)
        if h.numpower_host_last_error():
            _raise_pending(h)
        return int(v)

    def __add__(self, o): return NDArray._binary("add", self, o)
    def __radd__(self, o): return NDArray._binary("add", o, self)
    def __sub__(self, o): return NDArray._binary("subtract", self, o)
    def __rsub__(self, o): return NDArray._binary("subtract", o, self)
    def __mul__(self, o): return NDArray._binary("multiply", self, o)
    def __rmul__(self, o): return NDArray._binary("multiply", o, self)
    def __truediv__(self, o): return NDArray._binary("divide", self, o)
    def __rtruediv__(self, o): return NDArray._binary("divide", o, self)
    def __mod__(self, o): return NDArray._binary("mod", self, o)
    def __pow__(self, o): return NDArray._binary("pow", self, o)

    @staticmethod
    def square(a):   # PHP_METHOD(NDArray, square): Multiply_Float(nda, nda), numpower.c:3093
        x, _ = NDArray._coerce(a)
        return NDArray._binary("multiply", x, x)

    @staticmethod
    def arctan2(x, y):
        h = _load_host()
        a, _ = NDArray._coerce(x)
        b, _ = NDArray._coerce(y)
        return NDArray._wrap(h.NDArrayMathGPU_ElementWise1N(a._p, _fn(h, "cuda_float_arctan2"), b._p))

    # ---- unary ops ---------------------------------------------------------------------------------
    @staticmethod
    def _unary(name, a):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if name == "rsqrt":
            # numpower.c:1791 passes cuda_float_arccos for rsqrt on the GPU (a copy-paste slip: the reference has
            # no cuda_float_rsqrt); the stand-in asks for the CPU definition (float_rsqrt, double_math.c:111-126)
            # through NDArray_Rsqrt instead of reproducing the slip.
            return NDArray._wrap(h.NDArray_Rsqrt(x._p))
        if name == "exp2":    # no cuda_float_exp2 in the reference (numpower.c:3153 is CPU-only): own entry point
            return NDArray._wrap(h.NDArray_Exp2(x._p))
        if name == "abs":     # PHP_METHOD(NDArray, abs) calls NDArray_Abs (numpower.c:1619)
            return NDArray._wrap(h.NDArray_Abs(x._p))
        if _LAZY_BINDING and x._ptr.contents.device == GPU:      # the method's device branch, as section 2c edits it
            return NDArray._wrap(h.NPH_LazyElementWise(x._ptr, _fn(h, "cuda_float_" + name)))
        return NDArray._wrap(h.NDArrayMathGPU_ElementWise(x._p, _fn(h, "cuda_float_" + name)))

    @staticmethod
    def clip(a, min, max):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if _LAZY_BINDING and x._ptr.contents.device == GPU:
            return NDArray._wrap(h.NPH_LazyElementWise2F(x._ptr, _fn(h, "cuda_float_clip"), float(min), float(max)))
        return NDArray._wrap(h.NDArrayMathGPU_ElementWise2F(x._p, _fn(h, "cuda_float_clip"), float(min), float(max)))

    @staticmethod
    def round(a, precision=0):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if _LAZY_BINDING and x._ptr.contents.device == GPU:
            return NDArray._wrap(h.NPH_LazyElementWise1F(x._ptr, _fn(h, "cuda_float_round"), float(precision)))
        return NDArray._wrap(h.NDArrayMathGPU_ElementWise1F(x._p, _fn(h, "cuda_float_round"), float(precision)))

    # ---- reductions -----------------------------------------------------------------------------------
    @staticmethod
    def _reduce(op, a, axis):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if axis is None:
            fn = {"sum": h.NDArray_Sum_Float, "prod": h.NDArray_Float_Prod, "min": h.NDArray_Min,
                  "max": h.NDArray_Max}[op]
            h.numpower_host_clear_error()
            if _LAZY_BINDING:     # PHP_METHOD(sum ...) as section 2c edits it: a pending operand is reduced inside its chain's kernel
                from ._lib import REDUCE_OPS
                v = h.NPH_ReduceAll(REDUCE_OPS[op], C.cast(fn, C.c_void_p), x._ptr)
            else:
                v = fn(x._p)
            if h.numpower_host_last_error():
                _raise_pending(h)
            return float(v)
        ax = C.c_int(int(axis))
        if op == "sum":    # numpower.c:4637
            return NDArray._wrap(h.reduce(x._p, C.byref(ax), C.cast(h.NDArray_Add_Float, C.c_void_p)))
        if op == "prod":   # numpower.c:4742
            return NDArray._wrap(h.reduce(x._p, C.byref(ax), C.cast(h.NDArray_Multiply_Float, C.c_void_p)))
        if op == "min":
            return NDArray._wrap(h.NDArray_MinAxis(x._p, int(axis)))
        return NDArray._wrap(h.NDArray_MaxAxis(x._p, int(axis)))

    sum = staticmethod(lambda a, axis=None: NDArray._reduce("sum", a, axis))
    prod = staticmethod(lambda a, axis=None: NDArray._reduce("prod", a, axis))
    min = staticmethod(lambda a, axis=None: NDArray._reduce("min", a, axis))
    max = staticmethod(lambda a, axis=None: NDArray._reduce("max", a, axis))

    @staticmethod
    def mean(a, axis=None):
        """PHP_METHOD(NDArray, mean) (numpower.c:2642-2688)."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if axis is None:
            # NDArray_Sum_Float(nda) / NDArray_NUMELEMENTS(nda): float / long in C
            s = NDArray._reduce("sum", x, None)
            return float(np.float32(s) / np.float32(x.size()))
        total = NDArray._reduce("sum", x, axis)
        count = NDArray(h.NDArray_CreateFromLongScalar(x.shape()[int(axis)]))
        if isinstance(total, float):   # 1-D input: 0-d sum
            return float(np.float32(total) / np.float32(x.shape()[int(axis)]))
        return NDArray._binary("divide", total, count)

    @staticmethod
    def median(a):
        """PHP_METHOD(NDArray, median) (numpower.c:2700-2731) -> float; on the device (radix select)."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        h.numpower_host_clear_error()
        v = h.NDArray_Median_Float(x._p)
        if h.numpower_host_last_error():
            _raise_pending(h)
        return float(v)

    @staticmethod
    def quantile(a, q):
        """PHP_METHOD(NDArray, quantile) (numpower.c:2788): q a scalar in [0, 1] -> float."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        qq, _ = NDArray._coerce(q)
        return NDArray._wrap(h.NDArray_Quantile(x._p, qq._p))

    # ---- layout (PHP_METHOD transpose, numpower.c:1404-1450) ----
    @staticmethod
    def transpose(a, axes=None):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if axes is None:
            return NDArray._wrap(h.NDArray_Transpose(x._p, None))
        arr = (C.c_int * max(len(axes), 1))(*[int(v) for v in axes])
        dims = _CDims(arr, len(axes))
        return NDArray._wrap(h.NDArray_Transpose(x._p, C.byref(dims)))

    # ---- views / layout / equality around the path ----
    @staticmethod
    def reshape(a, shape):   # PHP_METHOD reshape, numpower.c:644: a view sharing the buffer
        h = _load_host()
        x, _ = NDArray._coerce(a)
        arr = (C.c_int * max(len(shape), 1))(*[int(v) for v in shape])
        return NDArray._wrap(h.NDArray_Reshape(x._p, arr, len(shape)))

    @staticmethod
    def flatten(a):          # numpower.c:1584
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Flatten(x._p))

    @staticmethod
    def expand_dims(a, axis):   # numpower.c:3563: axis int or list of ints
        h = _load_host()
        x, _ = NDArray._coerce(a)
        ax, _ = NDArray._coerce(axis)
        return NDArray._wrap(h.NDArray_ExpandDim(x._p, ax._p))

    @staticmethod
    def append(a, b):        # numpower.c:3908: flat concatenation (axis = -1)
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        arr = (_P * 2)(x._p, y._p)
        return NDArray._wrap(h.NDArray_Append(arr, -1, 2))

    # ---- manipulation wrappers (PHP_METHODs atleast_1d … column_stack, numpower.c:1480-1570, 3590-3900) ----
    @staticmethod
    def _unary_host(name, a):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(getattr(h, name)(x._p))

    atleast_1d = staticmethod(lambda a: NDArray._unary_host("NDArray_AtLeast1D", a))
    atleast_2d = staticmethod(lambda a: NDArray._unary_host("NDArray_AtLeast2D", a))
    atleast_3d = staticmethod(lambda a: NDArray._unary_host("NDArray_AtLeast3D", a))
    diag = staticmethod(lambda a: NDArray._unary_host("NDArray_Diag", a))

    @staticmethod
    def squeeze(a, axis=None):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if axis is None:
            return NDArray._wrap(h.NDArray_Squeeze(x._p, None))
        ax, _ = NDArray._coerce(axis)
        return NDArray._wrap(h.NDArray_Squeeze(x._p, ax._p))

    @staticmethod
    def swapaxes(a, axis1, axis2):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_SwapAxes(x._p, int(axis1), int(axis2)))

    @staticmethod
    def rollaxis(a, axis, start=0):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Rollaxis(x._p, int(axis), int(start)))

    @staticmethod
    def moveaxis(a, source, destination):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        src = [int(v) for v in (source if isinstance(source, (list, tuple)) else [source])]
        dst = [int(v) for v in (destination if isinstance(destination, (list, tuple)) else [destination])]
        s = (C.c_int * max(len(src), 1))(*src)
        d = (C.c_int * max(len(dst), 1))(*dst)
        return NDArray._wrap(h.NDArray_Moveaxis(x._p, s, d, len(src), len(dst)))

    @staticmethod
    def _stack(name, arrays, *extra):
        h = _load_host()
        xs = [NDArray._coerce(a)[0] for a in arrays]
        arr = (_P * max(len(xs), 1))(*[x._p for x in xs])
        return NDArray._wrap(getattr(h, name)(arr, len(xs), *extra))

    concatenate = staticmethod(lambda arrays, axis=0: NDArray._stack("NDArray_Concatenate", arrays, int(axis)))
    vstack = staticmethod(lambda arrays: NDArray._stack("NDArray_VSTACK", arrays))
    hstack = staticmethod(lambda arrays: NDArray._stack("NDArray_HSTACK", arrays))
    dstack = staticmethod(lambda arrays: NDArray._stack("NDArray_DSTACK", arrays))
    column_stack = staticmethod(lambda arrays: NDArray._stack("NDArray_ColumnStack", arrays))

    @staticmethod
    def diagonal(a):         # numpower.c:1179
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Diagonal(x._p, 0))

    @staticmethod
    def trace(a):            # numpower.c:4067
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Trace(x._p))

    @staticmethod
    def array_equal(a, b) -> bool:   # the `==` handler of the PHP object, numpower.c:175-186
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        h.numpower_host_clear_error()
        r = h.NDArray_ArrayEqual(x._p, y._p)
        if h.numpower_host_last_error():
            _raise_pending(h)
        return bool(r)

    @staticmethod
    def allclose(a, b, rtol=1e-05, atol=1e-08) -> bool:   # numpower.c:1358-1391
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        if x is y:
            return True
        r = h.NDArray_AllClose(x._p, y._p, float(rtol), float(atol))
        if r == -1:
            _raise_pending(h)
        return bool(r)

    def slice(self, *indices):   # PHP_METHOD slice, numpower.c:4773: each index [start(,stop(,step))]
        h = _load_host()
        idx = [NDArray._coerce(list(i) if isinstance(i, (list, tuple)) else [i])[0] for i in indices]
        arr = (_P * max(len(idx), 1))(*[i._p for i in idx])
        return NDArray._wrap(h.NDArray_Slice(self._p, arr, len(idx)))

    def contiguous(self):        # NDArray_ToContiguous
        return NDArray._wrap(_load_host().NDArray_ToContiguous(self._p))

    # ---- argmax / argmin (PHP_METHOD argmax / argmin, numpower.c:2570-2630) ----
    @staticmethod
    def _arg(a, axis, keepdims, is_max):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        ax = 128 if axis is None else int(axis)   # ZEND_NUM_ARGS() == 1 -> axis = 128 (flattened)
        return NDArray._wrap(h.NDArray_ArgMinMaxCommon(x._p, ax, bool(keepdims), bool(is_max)))

    argmax = staticmethod(lambda a, axis=None, keepdims=False: NDArray._arg(a, axis, keepdims, True))
    argmin = staticmethod(lambda a, axis=None, keepdims=False: NDArray._arg(a, axis, keepdims, False))

    # ---- statistics (PHP_METHOD variance / std / average, numpower.c:2743-2900) ----
    @staticmethod
    def variance(a):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Variance(x._p))

    @staticmethod
    def std(a):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Std(x._p))

    @staticmethod
    def average(a, weights=None):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        if weights is None:
            return NDArray._wrap(h.NDArray_Average(x._p, None))
        w, _ = NDArray._coerce(weights)
        return NDArray._wrap(h.NDArray_Average(x._p, w._p))

    # ---- linear algebra -----------------------------------------------------------------------------------
    @staticmethod
    def matmul(a, b):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Matmul(x._p, y._p))

    @staticmethod
    def dot(a, b):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Dot(x._p, y._p))

    @staticmethod
    def inner(a, b):         # PHP_METHOD inner
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Inner(x._p, y._p))

    @staticmethod
    def det(a):              # numpower.c:4598: a 0-d GPU array, RETURN_NDARRAY turns it into a float
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Det(x._p))

    @staticmethod
    def inv(a):              # numpower.c:4548
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Inverse(x._p))

    @staticmethod
    def solve(a, b):         # numpower.c:4145
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Solve(x._p, y._p))

    @staticmethod
    def lu(a):               # numpower.c:4231-4253: RETURN_3NDARRAY -> (P, L, U)
        h = _load_host()
        x, _ = NDArray._coerce(a)
        rtns = h.NDArray_LU(x._p)
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3))
        _libc_free(C.cast(rtns, C.c_void_p))   # the vector itself (the reference efree()s it)
        return out

    @staticmethod
    def cholesky(a):         # numpower.c:4119: lower-triangular L with a = L L^T, from a's lower triangle alone
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Cholesky(x._p))

    @staticmethod
    def svd(a):              # numpower.c PHP_METHOD(svd): RETURN_3NDARRAY -> (U (m, m), S (k), V (n, n)); rows of V are right singular vectors
        h = _load_host()
        x, _ = NDArray._coerce(a)
        rtns = h.NDArray_SVD(x._p)
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out

    @staticmethod
    def eig(a):              # numpower.c PHP_METHOD(eig): RETURN_2NDARRAY -> (values (n) ascending, vectors (n, n), vector j in column j); symmetric a only
        h = _load_host()
        x, _ = NDArray._coerce(a)
        rtns = h.NDArray_Eig(x._p)
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(2))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out

    @staticmethod
    def qr(a):               # numpower.c PHP_METHOD(qr): RETURN_2NDARRAY -> (Q (m, n) with orthonormal columns, R (n, n) upper triangular); m >= n
        h = _load_host()
        x, _ = NDArray._coerce(a)
        rtns = h.NDArray_Qr(x._p)
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(2))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out

    @staticmethod
    def lstsq(a, b):         # numpower.c PHP_METHOD(lstsq): x (n, nrhs) minimising ||a x - b||; m >= n
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Lstsq(x._p, y._p))

    @staticmethod
    def matrix_rank(a, tol=None):   # PHP_METHOD(matrix_rank): singular values > tol (default s_max * max(m, n) * FLT_EPSILON)
        h = _load_host()
        x, _ = NDArray._coerce(a)
        t = None if tol is None else C.byref(C.c_float(tol))
        return NDArray._wrap(h.NDArray_MatrixRank(x._p, t))

    @staticmethod
    def norm(a, order=2):    # PHP_METHOD(norm): order 2 = the largest singular value
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Norm(x._p, int(order)))

    @staticmethod
    def cond(a):             # PHP_METHOD(cond): norm2(a) * norm2(inv(a))
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArray_Cond(x._p))

    @staticmethod
    def _signal2d(a, b, mode, boundary, fill_value, flip):
        """PHP_METHOD(convolve2d) / (correlate2d), numpower.c:4399-4420 / 4460-4481: the first letter of `mode` (valid / same / full)
        and of `boundary` (fill / wrap / symm) picks the flag.  A deviation: the PHP methods leave the flag at 0 (valid, fill)
        for an empty string or an unknown letter; here that is an Error.  And fill_value is passed on (PHP parses it and passes
        NULL)."""
        h = _load_host()
        modes, boundaries = {"v": 0, "s": 1, "f": 2}, {"f": 0, "s": 4, "w": 8}
        if not isinstance(mode, str) or mode[:1] not in modes:
            raise Error("mode must begin with 'v' (valid), 's' (same) or 'f' (full), not %r" % (mode,))
        if not isinstance(boundary, str) or boundary[:1] not in boundaries:
            raise Error("boundary must begin with 'f' (fill), 'w' (wrap) or 's' (symm), not %r" % (boundary,))
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        f, _ = NDArray._coerce(float(fill_value) if isinstance(fill_value, (int, float)) and not isinstance(fill_value, bool) else fill_value)
        return NDArray._wrap(h.NDArray_Correlate2D(x._p, y._p, modes[mode[0]], boundaries[boundary[0]], f._p, flip))

    @staticmethod
    def convolve2d(a, b, mode, boundary, fill_value=0.0):    # numpower.c:4379: scipy.signal.convolve2d
        return NDArray._signal2d(a, b, mode, boundary, fill_value, 1)

    @staticmethod
    def correlate2d(a, b, mode, boundary, fill_value=0.0):   # numpower.c:4440: scipy.signal.correlate2d
        return NDArray._signal2d(a, b, mode, boundary, fill_value, 0)

    @staticmethod
    def _dnn_geometry(filters, stride, padding, dilation):
        """-> None for the defaults (the reference-signature host functions), else three C int pairs (stride, padding, dilation)"""
        def pair(v, what):
            if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
                return int(v), int(v)
            if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in v):
                return int(v[0]), int(v[1])
            raise Error("dnn_conv2d: %s must be an int or a pair of ints" % what)

        s, d = pair(stride, "stride"), pair(dilation, "dilation")
        if isinstance(padding, str):
            if padding not in ("valid", "same"):
                raise Error("dnn_conv2d: padding must be an int, a pair of ints, 'valid' or 'same'")
            if padding == "valid":
                p = (0, 0)
            else:
                shape = tuple(np.shape(filters)) if not isinstance(filters, NDArray) else tuple(filters.shape())
                if len(shape) != 4:
                    raise Error("dnn_conv2d: padding 'same' needs 4-dimensional filters (F, C, kh, kw)")
                ke = tuple(d[i] * (shape[2 + i] - 1) + 1 for i in range(2))
                if s != (1, 1) or min(d) < 1 or ke[0] % 2 == 0 or ke[1] % 2 == 0:
                    raise Error("dnn_conv2d: padding 'same' needs stride 1 and an odd effective window, dilation . (k - 1) + 1, along both axes")
                p = ((ke[0] - 1) // 2, (ke[1] - 1) // 2)
        else:
            p = pair(padding, "padding")
        if (s, p, d) == ((1, 1), (0, 0), (1, 1)):
            return None
        return tuple((C.c_int * 2)(*v) for v in (s, p, d))

    _DNN_ACTIVATIONS = {None: b"n", "relu": b"r", "tanh": b"t", "sigmoid": b"s"}

    @staticmethod
    def _dnn_activation(activation, who="dnn_conv2d"):
        if not (activation is None or isinstance(activation, str)) or activation not in NDArray._DNN_ACTIVATIONS:
            raise Error("%s: activation must be None, 'relu', 'tanh' or 'sigmoid', not %r" % (who, activation))
        return NDArray._DNN_ACTIVATIONS[activation]

    @staticmethod
    def dnn_conv2d_forward(x, filters, stride=1, padding=0, dilation=1, bias=None, activation=None):   # numpower.c:4293: NDArrayDNN_Conv2D_Forward(x, filters, NULL, 'r', 1)
        """y (N, F, oh, ow) of x (N, C, H, W) and filters (F, C, kh, kw): cross-correlation, no bias, no activation (DESIGN.md
        §3.14).  stride, padding and dilation take an int or a (rows, columns) pair; padding also 'valid' (0) and 'same'
        ((keh - 1) / 2 of the effective window keh = dilation . (kh - 1) + 1, for stride 1 and odd keh, kew).
        oh = floor((H + 2 ph - keh) / sh) + 1.  With the defaults: the reference's call, y (N, F, H - kh + 1, W - kw + 1).
        bias: a 1-D array (F,) added to every output of its filter, ONE fp32 add after the reduction; activation: None, 'relu',
        'tanh' or 'sigmoid', applied in the same kernel: y = act(conv + bias).  With both at None: the code path above."""
        h = _load_host()
        geometry = NDArray._dnn_geometry(filters, stride, padding, dilation)
        act = NDArray._dnn_activation(activation)
        a, _ = NDArray._coerce(x)
        w, _ = NDArray._coerce(filters)
        if geometry is None and bias is None and activation is None:       # every keyword at its default: the call the PHP method makes
            return NDArray._wrap(h.NDArrayDNN_Conv2D_Forward(a._p, w._p, None, b"r", 1))
        b = None if bias is None else NDArray._coerce(bias)[0]
        return NDArray._wrap(h.NDArrayDNN_Conv2D_LayerForward(a._p, w._p, None if b is None else b._p, *(geometry or (None, None, None)), act))

    @staticmethod
    def dnn_conv2d_backward(x, y, filters, stride=1, padding=0, dilation=1, out=None, activation=None, bias=False):   # numpower.c:4348: NDArrayDNN_Conv2D_Backward(x, y, filters, 3, 'r', 1) -> RETURN_2NDARRAY
        """(dW (F, C, kh, kw), dX (N, C, H, W)) for y = the gradient of dnn_conv2d_forward(x, filters, stride, padding, dilation),
        the reference's order.  Rows and columns of x that no window reads get dX = 0.
        For a layer with an activation pass it and `out`, the forward RESULT: the gradient goes through act'(out) first (relu: a
        select on out <= 0; tanh: 1 - out^2; sigmoid: (1 - out) out).  bias=True: (dW, dX, db) with db (F,) the gradient of the
        bias.  With the three at their defaults: the code path above and its 2-tuple."""
        h = _load_host()
        geometry = NDArray._dnn_geometry(filters, stride, padding, dilation)
        act = NDArray._dnn_activation(activation)
        if activation is not None and out is None:
            raise Error("dnn_conv2d_backward: an activation needs out, the forward result (gradients are expressed through the output)")
        a, _ = NDArray._coerce(x)
        g, _ = NDArray._coerce(y)
        w, _ = NDArray._coerce(filters)
        if geometry is None and out is None and activation is None and not bias:      # every keyword at its default: the PHP method's call
            rtns = h.NDArrayDNN_Conv2D_Backward(a._p, g._p, w._p, 3, b"r", 1)
        else:
            o = None if out is None else NDArray._coerce(out)[0]
            rtns = h.NDArrayDNN_Conv2D_LayerBackward(a._p, None if o is None else o._p, g._p, w._p, *(geometry or (None, None, None)), act, 1 if bias else 0)
        if not rtns:
            _raise_pending(h)
        out_arrays = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3 if bias else 2))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out_arrays

    _DNN_POOL_MODES = {"max": b"m", "avg": b"a", "avg_valid": b"v"}

    @staticmethod
    def _dnn_pool_geometry(kernel_size, stride, padding, mode):
        """-> (kernel, stride or None, padding, mode's code): C int pairs; stride None means the window"""
        def pair(v, what):
            if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
                return int(v), int(v)
            if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in v):
                return int(v[0]), int(v[1])
            raise Error("dnn_pool2d: %s must be an int or a pair of ints" % what)

        if not isinstance(mode, str) or mode not in NDArray._DNN_POOL_MODES:
            raise Error("dnn_pool2d: mode must be 'max', 'avg' or 'avg_valid', not %r" % (mode,))
        k, p = pair(kernel_size, "kernel_size"), pair(padding, "padding")
        s = None if stride is None else pair(stride, "stride")
        return (C.c_int * 2)(*k), None if s is None else (C.c_int * 2)(*s), (C.c_int * 2)(*p), NDArray._DNN_POOL_MODES[mode]

    @staticmethod
    def dnn_pool2d_forward(x, kernel_size, stride=None, padding=0, mode="max"):      # the reference has no pooling
        """y (N, C, oh, ow) of x (N, C, H, W), each (n, c) plane pooled on its own.  kernel_size, stride and
        padding take an int or a (rows, columns) pair; stride None means the window; 2 . padding <= kernel_size.
        oh = floor((H + 2 ph - kh) / sh) + 1: no dilation, no ceil mode.  mode 'max': the first of equal maxima, a NaN in the
        window gives NaN, padding is never a candidate; 'avg': the sum of the real cells / (kh . kw), padding counts; 'avg_valid':
        / the number of real cells.  One chain of fp32 adds in row-major order and one correctly rounded division."""
        h = _load_host()
        k, s, p, code = NDArray._dnn_pool_geometry(kernel_size, stride, padding, mode)
        a, _ = NDArray._coerce(x)
        return NDArray._wrap(h.NDArrayDNN_Pool2D_Forward(a._p, k, s, p, code))

    @staticmethod
    def dnn_pool2d_backward(x, dy, kernel_size, stride=None, padding=0, mode="max"):
        """dx (N, C, H, W) for dy = the gradient of dnn_pool2d_forward(x, kernel_size, stride, padding, mode).  x is the layer's
        INPUT: 'max' finds the maxima again (no state is kept between the calls), the averages take its shape only.  A gather in
        a fixed order, windows by rows then columns: bit-identical from run to run.  Cells that no window covers get 0."""
        h = _load_host()
        k, s, p, code = NDArray._dnn_pool_geometry(kernel_size, stride, padding, mode)
        a, _ = NDArray._coerce(x)
        g, _ = NDArray._coerce(dy)
        return NDArray._wrap(h.NDArrayDNN_Pool2D_Backward(a._p, g._p, k, s, p, code))

    @staticmethod
    def _softmax_axis(axis, who):
        if not isinstance(axis, (int, np.integer)) or isinstance(axis, bool):
            raise Error("%s: axis must be an int" % who)
        return int(axis)

    @staticmethod
    def softmax(a, axis=-1):      # the reference has no softmax
        """softmax of a GPU array along `axis` (any ndim >= 1, negative axes count from the end):
        exp(x - max) / sum, one read and one write, a correctly rounded division.  A row with a NaN, a +Inf, or nothing but
        -Inf is NaN throughout; a -Inf among finite values gives +0."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArrayDNN_Softmax_Forward(x._p, NDArray._softmax_axis(axis, "softmax"), b"s"))

    @staticmethod
    def log_softmax(a, axis=-1):
        """(x - max) - log(sum exp(x - max)) along `axis`: finite where log(softmax(x)) is -Inf or NaN."""
        h = _load_host()
        x, _ = NDArray._coerce(a)
        return NDArray._wrap(h.NDArrayDNN_Softmax_Forward(x._p, NDArray._softmax_axis(axis, "log_softmax"), b"l"))

    @staticmethod
    def softmax_backward(y, dy, axis=-1, log=False):
        """dx for y = softmax(x, axis) (log=False: y . (dy - sum(dy . y))) or y = log_softmax(x, axis) (log=True:
        dy - exp(y) . sum(dy)): from the forward OUTPUT, fixed-order sums, bit-identical from run to run."""
        h = _load_host()
        out, _ = NDArray._coerce(y)
        g, _ = NDArray._coerce(dy)
        return NDArray._wrap(h.NDArrayDNN_Softmax_Backward(out._p, g._p, NDArray._softmax_axis(axis, "softmax_backward"), b"l" if log else b"s"))

    _DNN_XENT_REDUCTIONS = {"none": b"n", "sum": b"s", "mean": b"m"}

    @staticmethod
    def dnn_cross_entropy(logits, target, reduction="mean", with_grad=False):
        """The cross-entropy of logits (rows, classes) against a target of (rows) class indices (stored as fp32) or
        (rows, classes) probabilities, computed from the logits: log(sum exp(l - max)) - (l - max)[label], finite where
        -log(softmax) overflows.  reduction 'none' returns the (rows) losses, 'sum' and 'mean' a float.  with_grad=True returns
        (loss, dlogits) with dlogits = (softmax(logits) - target) . scale from the same launch, scale = 1 / rows for 'mean' and 1
        otherwise.  A label that is not an integer in [0, classes) gives NaN for its row's loss and gradient."""
        h = _load_host()
        if not isinstance(reduction, str) or reduction not in NDArray._DNN_XENT_REDUCTIONS:
            raise Error("dnn_cross_entropy: reduction must be 'none', 'sum' or 'mean', not %r" % (reduction,))
        l, _ = NDArray._coerce(logits)
        t, _ = NDArray._coerce(target)
        grad = _P()
        loss = h.NDArrayDNN_CrossEntropy(l._p, t._p, NDArray._DNN_XENT_REDUCTIONS[reduction], 1 if with_grad else 0,
                                         C.byref(grad) if with_grad else None)
        loss = NDArray._wrap(loss)
        return (loss, NDArray._wrap(grad)) if with_grad else loss

    @staticmethod
    def _bn_operand(value):
        return None if value is None else NDArray._coerce(value)[0]

    @staticmethod
    def dnn_batch_norm_forward(x, gamma=None, beta=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5):
        """Batch normalization of a GPU array of ndim >= 2 with the channel on axis 1: per channel the mean and
        the biased variance over every other axis, carried in fp64 from shifted sums, then y = (x - mean) . invstd . gamma + beta.
        training=True returns (y, save_mean, save_invstd) and updates running_mean / running_var in place when given
        (r = (1 - momentum) . r + momentum . s, the unbiased variance for running_var); training=False needs both running
        arrays and returns y.  gamma and beta are (C) arrays or None (1 and 0)."""
        h = _load_host()
        if isinstance(momentum, bool) or isinstance(eps, bool) or not isinstance(momentum, (int, float, np.floating, np.integer)) \
                or not isinstance(eps, (int, float, np.floating, np.integer)):
            raise Error("dnn_batch_norm_forward: momentum and eps must be numbers")
        ops = [NDArray._bn_operand(v) for v in (x, gamma, beta, running_mean, running_var)]
        if ops[0] is None:
            raise Error("dnn_batch_norm_forward: x must be an array")
        rtns = h.NDArrayDNN_BatchNorm_Forward(*[None if o is None else o._p for o in ops], 1 if training else 0, float(momentum), float(eps))
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3 if training else 1))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out if training else out[0]

    @staticmethod
    def dnn_batch_norm_backward(x, dy, gamma, save_mean, save_invstd):
        """(dx, dgamma, dbeta) of training-mode batch normalization from the layer's input x, the gradient dy of its output, gamma
        (or None) and the statistics the forward pass saved: fp64 sums of dy and dy . xhat, then
        dx = (gamma . invstd) . ((dy - mean(dy)) - xhat . mean(dy . xhat))."""
        h = _load_host()
        ops = [NDArray._bn_operand(v) for v in (x, dy, gamma, save_mean, save_invstd)]
        if any(ops[i] is None for i in (0, 1, 3, 4)):
            raise Error("dnn_batch_norm_backward: x, dy, save_mean and save_invstd must be arrays")
        rtns = h.NDArrayDNN_BatchNorm_Backward(*[None if o is None else o._p for o in ops])
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out

    @staticmethod
    def _norm_results(h, rtns):
        if not rtns:
            _raise_pending(h)
        out = tuple(NDArray(C.cast(rtns[i], _P)) for i in range(3))
        _libc_free(C.cast(rtns, C.c_void_p))
        return out

    @staticmethod
    def _normalized_shape(who, normalized_shape):
        """-> (int array, ndim) for an int or a tuple of ints"""
        dims = (normalized_shape,) if isinstance(normalized_shape, (int, np.integer)) and not isinstance(normalized_shape, bool) else normalized_shape
        if not isinstance(dims, (tuple, list)) or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in dims):
            raise Error(who + ": normalized_shape must be an int or a tuple of ints")
        return (C.c_int * max(1, len(dims)))(*[int(v) for v in dims]), len(dims)

    @staticmethod
    def dnn_layer_norm_forward(x, normalized_shape, gamma=None, beta=None, eps=1e-5):
        """Layer normalization of a GPU array over its trailing axes: normalized_shape, an int or a tuple, must
        equal those axes.  Per row (one per index of the leading axes) the mean and the biased variance, carried in fp64 from
        shifted sums, then y = (x - mean) . invstd . gamma + beta with gamma and beta of the normalized shape, or None (1 and 0).
        Returns (y, save_mean, save_invstd), the statistics in the shape of the leading axes."""
        h = _load_host()
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.floating, np.integer)):
            raise Error("dnn_layer_norm_forward: eps must be a number")
        dims, ndim = NDArray._normalized_shape("dnn_layer_norm_forward", normalized_shape)
        ops = [NDArray._bn_operand(v) for v in (x, gamma, beta)]
        if ops[0] is None:
            raise Error("dnn_layer_norm_forward: x must be an array")
        p = [None if o is None else o._p for o in ops]
        return NDArray._norm_results(h, h.NDArrayDNN_LayerNorm_Forward(p[0], dims, ndim, p[1], p[2], float(eps)))

    @staticmethod
    def dnn_layer_norm_backward(x, dy, normalized_shape, gamma, save_mean, save_invstd):
        """(dx, dgamma, dbeta) of layer normalization from the layer's input x, the gradient dy of its output, gamma (or None) and
        the statistics the forward pass saved: per row g = dy . gamma, fp64 sums of g and g . xhat, then
        dx = invstd . ((g - mean(g)) - xhat . mean(g . xhat)); per parameter dbeta = sum dy and dgamma = sum dy . xhat."""
        h = _load_host()
        dims, ndim = NDArray._normalized_shape("dnn_layer_norm_backward", normalized_shape)
        ops = [NDArray._bn_operand(v) for v in (x, dy, gamma, save_mean, save_invstd)]
        if any(ops[i] is None for i in (0, 1, 3, 4)):
            raise Error("dnn_layer_norm_backward: x, dy, save_mean and save_invstd must be arrays")
        p = [None if o is None else o._p for o in ops]
        return NDArray._norm_results(h, h.NDArrayDNN_LayerNorm_Backward(p[0], p[1], dims, ndim, p[2], p[3], p[4]))

    @staticmethod
    def dnn_group_norm_forward(x, num_groups, gamma=None, beta=None, eps=1e-5):
        """Group normalization of a GPU array of ndim >= 2 with the channel on axis 1: the C channels form
        num_groups groups of C / num_groups, and each (sample, group) is normalized over its channels and every later axis, with
        statistics carried in fp64 from shifted sums; then y = (x - mean) . invstd . gamma + beta with gamma and beta (C) arrays
        or None (1 and 0).  Instance normalization is num_groups = C; num_groups = 1 normalizes each sample as a whole.
        Returns (y, save_mean, save_invstd), the statistics of shape (N, num_groups)."""
        h = _load_host()
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.floating, np.integer)):
            raise Error("dnn_group_norm_forward: eps must be a number")
        if isinstance(num_groups, bool) or not isinstance(num_groups, (int, np.integer)):
            raise Error("dnn_group_norm_forward: num_groups must be an int")
        ops = [NDArray._bn_operand(v) for v in (x, gamma, beta)]
        if ops[0] is None:
            raise Error("dnn_group_norm_forward: x must be an array")
        p = [None if o is None else o._p for o in ops]
        return NDArray._norm_results(h, h.NDArrayDNN_GroupNorm_Forward(p[0], int(num_groups), p[1], p[2], float(eps)))

    @staticmethod
    def dnn_group_norm_backward(x, dy, num_groups, gamma, save_mean, save_invstd):
        """(dx, dgamma, dbeta) of group normalization (instance normalization: num_groups = C) from the layer's input x, the
        gradient dy of its output, gamma (or None) and the statistics the forward pass saved."""
        h = _load_host()
        if isinstance(num_groups, bool) or not isinstance(num_groups, (int, np.integer)):
            raise Error("dnn_group_norm_backward: num_groups must be an int")
        ops = [NDArray._bn_operand(v) for v in (x, dy, gamma, save_mean, save_invstd)]
        if any(ops[i] is None for i in (0, 1, 3, 4)):
            raise Error("dnn_group_norm_backward: x, dy, save_mean and save_invstd must be arrays")
        p = [None if o is None else o._p for o in ops]
        return NDArray._norm_results(h, h.NDArrayDNN_GroupNorm_Backward(p[0], p[1], int(num_groups), p[2], p[3], p[4]))

    @staticmethod
    def _attention_scale(who, scale):
        """None -> 0.0, which the layers below read as the default 1 / sqrt(D)"""
        if scale is None:
            return 0.0
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating, np.integer)):
            raise Error(who + ": scale must be a number or None")
        if not float(scale) > 0.0:
            raise Error(who + ": scale must be greater than zero (None: 1 / sqrt(D))")
        return float(scale)

    @staticmethod
    def dnn_attention_forward(q, k, v, causal=False, scale=None):
        """Scaled dot-product attention of GPU arrays: o = softmax(q . k^T . scale) . v per index of the leading
        axes, fused, so the (Sq, Sk) scores are never stored.  q is (..., Sq, D), k and v are (..., Sk, D) with equal leading axes
        and D <= 128.  causal=True lets row i see the keys j <= i (top-left alignment).  scale=None means 1 / sqrt(D).
        Returns (o, save_max, save_sum): the row maximum of the scaled scores and the sum of exp(score - maximum), in q's shape
        without its last axis, which dnn_attention_backward takes."""
        h = _load_host()
        sc = NDArray._attention_scale("dnn_attention_forward", scale)
        ops = [NDArray._bn_operand(a) for a in (q, k, v)]
        if any(o is None for o in ops):
            raise Error("dnn_attention_forward: q, k and v must be arrays")
        return NDArray._norm_results(h, h.NDArrayDNN_Attention_Forward(ops[0]._p, ops[1]._p, ops[2]._p, 1 if causal else 0, sc))

    @staticmethod
    def dnn_attention_backward(q, k, v, o, dout, save_max, save_sum, causal=False, scale=None):
        """(dq, dk, dv) of dnn_attention_forward from its operands, its output o, the gradient dout of o and the statistics it
        saved; causal and scale must be the forward call's.  The probabilities are recomputed tile by tile; the scratch is one
        float per query row."""
        h = _load_host()
        sc = NDArray._attention_scale("dnn_attention_backward", scale)
        ops = [NDArray._bn_operand(a) for a in (q, k, v, o, dout, save_max, save_sum)]
        if any(a is None for a in ops):
            raise Error("dnn_attention_backward: q, k, v, o, dout, save_max and save_sum must be arrays")
        return NDArray._norm_results(h, h.NDArrayDNN_Attention_Backward(*[a._p for a in ops], 1 if causal else 0, sc))

    @staticmethod
    def _optim_list(who, name, values, optional=False):
        """-> (the arrays, which keeps them alive; the C vector of their pointers; its length) for a list or tuple of arrays.  Every
        pointer goes through the marshalling point, so a pending chain on a parameter, a state or a gradient is computed first."""
        if values is None and optional:
            return [], None, 0
        if not isinstance(values, (list, tuple)) or any(not isinstance(v, NDArray) for v in values):
            raise Error("%s: %s must be a list of arrays" % (who, name))
        return list(values), (_P * max(1, len(values)))(*[v._p for v in values]), len(values)

    @staticmethod
    def _optim_number(who, name, value):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.floating, np.integer)):
            raise Error("%s: %s must be a number" % (who, name))
        return float(value)

    @staticmethod
    def _optim_scale(who, grad_scale):
        """None, an array (its element 0) or (array, index) -> (array or None, pointer or None, index)"""
        if grad_scale is None:
            return None, None, 0
        arr, index = grad_scale if isinstance(grad_scale, tuple) and len(grad_scale) == 2 else (grad_scale, 0)
        if not isinstance(arr, NDArray) or isinstance(index, bool) or not isinstance(index, (int, np.integer)):
            raise Error(who + ": grad_scale must be an array, (array, index) or None")
        return arr, arr._p, int(index)

    @staticmethod
    def dnn_sgd_step(params, grads, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, buffers=None, first_step=False,
                     grad_scale=None):
        """One torch.optim.SGD update of a list of GPU arrays, in place, in one launch per 64 tensors:
        g = grad . s + weight_decay . p; with a momentum b = g on the first step, else momentum . b + (1 - dampening) . g, and the
        direction is b, or g + momentum . b with nesterov; p = p - lr . direction.  buffers is the list of momentum buffers (needed
        when momentum != 0); first_step=True sets them instead of reading them.  grad_scale: None, a GPU array whose element 0
        multiplies every gradient on the device, or (array, index): (dnn_grad_norm's result, 1) clips by the norm with no host read.
        Parameters and buffers must be contiguous arrays; gradients may be views.  Returns None."""
        who = "dnn_sgd_step"
        h = _load_host()
        nums = [NDArray._optim_number(who, n, v) for n, v in (("lr", lr), ("momentum", momentum), ("dampening", dampening), ("weight_decay", weight_decay))]
        keep = [NDArray._optim_list(who, "params", params), NDArray._optim_list(who, "grads", grads), NDArray._optim_list(who, "buffers", buffers, True)]
        scale, scale_p, index = NDArray._optim_scale(who, grad_scale)
        args = [x for k in keep for x in k[1:]]
        if not h.NDArrayDNN_SGD_Step(*args, *nums, 1 if nesterov else 0, 1 if first_step else 0, scale_p, index):
            _raise_pending(h)

    @staticmethod
    def dnn_adam_step(params, grads, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                      grad_scale=None):
        """One torch.optim.Adam update of a list of GPU arrays, in place; decoupled=True is AdamW's, whose weight
        decay multiplies p by (1 - lr . weight_decay) instead of joining the gradient.  exp_avg and exp_avg_sq are the lists of the
        two moments, zeros before the first update; step >= 1 is the number of this update, for the bias corrections.  grad_scale
        as in dnn_sgd_step.  Returns None."""
        who = "dnn_adam_step"
        h = _load_host()
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)):
            raise Error(who + ": step must be an int")
        if not isinstance(betas, (tuple, list)) or len(betas) != 2:
            raise Error(who + ": betas must be a pair of numbers")
        nums = [NDArray._optim_number(who, n, v) for n, v in (("lr", lr), ("betas", betas[0]), ("betas", betas[1]), ("eps", eps), ("weight_decay", weight_decay))]
        keep = [NDArray._optim_list(who, n, v) for n, v in (("params", params), ("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq))]
        scale, scale_p, index = NDArray._optim_scale(who, grad_scale)
        args = [x for k in keep for x in k[1:]]
        if not h.NDArrayDNN_Adam_Step(*args, max(-1, min(int(step), 2 ** 62)), *nums, 1 if decoupled else 0, scale_p, index):
            _raise_pending(h)

    @staticmethod
    def dnn_grad_norm(grads, max_norm=float("inf")):
        """-> a (2) GPU array: the 2-norm of all the elements of a list of GPU arrays (an fp64 sum of squares, one rounding) and
        torch's clip_grad_norm_ coefficient min(1, max_norm / (norm + 1e-6)), 1 for max_norm = inf.  Nothing is read back: pass
        (result, 1) as grad_scale of dnn_sgd_step / dnn_adam_step to clip."""
        who = "dnn_grad_norm"
        h = _load_host()
        limit = NDArray._optim_number(who, "max_norm", max_norm)
        keep = NDArray._optim_list(who, "grads", grads)
        return NDArray(h.NDArrayDNN_GradNorm(keep[1], keep[2], limit))

    @staticmethod
    def dnn_linear_forward(x, weight, bias=None, activation=None):      # the reference has no dense layer
        """y (..., N) = act(x . weight^T + bias) of GPU arrays in torch's layout: x (..., K), its leading axes
        flattened to rows; weight (N, K); bias a 1-D array (N,) or None, ONE fp32 add after the reduction; activation None,
        'relu', 'tanh' or 'sigmoid', applied in the same kernel.  Every output is one fp32 fmaf chain over k ascending: a row
        alone gives the bits it gives inside any batch."""
        h = _load_host()
        act = NDArray._dnn_activation(activation, "dnn_linear")
        a, _ = NDArray._coerce(x)
        w, _ = NDArray._coerce(weight)
        b = None if bias is None else NDArray._coerce(bias)[0]
        return NDArray._wrap(h.NDArrayDNN_Linear_Forward(a._p, w._p, None if b is None else b._p, act))

    @staticmethod
    def dnn_linear_backward(x, dy, weight, out=None, activation=None, bias=False, need_dx=True):
        """(dW (N, K), dX in x's shape) for dy = the gradient of dnn_linear_forward(x, weight, ...), the conv layer's order; with
        bias=True (dW, dX, db) with db (N,).  need_dx=False: dX is None and costs no launch (a first layer).  For a layer with
        an activation pass it and `out`, the forward RESULT: the gradient goes through act'(out) first (relu: a select on
        out <= 0; tanh: 1 - out^2; sigmoid: (1 - out) out).  No transposed copy of x, weight or dy is made."""
        h = _load_host()
        act = NDArray._dnn_activation(activation, "dnn_linear")
        if activation is not None and out is None:
            raise Error("dnn_linear_backward: an activation needs out, the forward result (gradients are expressed through the output)")
        a, _ = NDArray._coerce(x)
        g, _ = NDArray._coerce(dy)
        w, _ = NDArray._coerce(weight)
        o = None if out is None or activation is None else NDArray._coerce(out)[0]
        rtns = h.NDArrayDNN_Linear_Backward(a._p, None if o is None else o._p, g._p, w._p, act, 1 if bias else 0, 1 if need_dx else 0)
        if not rtns:
            _raise_pending(h)
        results = tuple(NDArray(C.cast(rtns[i], _P)) if rtns[i] else None for i in range(3 if bias else 2))
        _libc_free(C.cast(rtns, C.c_void_p))
        return results

    def copy(self):          # PHP_METHOD copy: NDArray_Copy on the array's own device
        return NDArray._wrap(_load_host().NDArray_Copy(self._p, C.cast(self._p, _P).contents.device))

    @staticmethod
    def outer(a, b):
        h = _load_host()
        x, _ = NDArray._coerce(a)
        y, _ = NDArray._coerce(b)
        return NDArray._wrap(h.NDArray_Outer(x._p, y._p))

    @staticmethod
    def batched_matmul(a, b):
        h = _load_host()
        return NDArray._wrap(h.NDArray_BatchedMatmul(a._p, b._p))

    @staticmethod
    def comm_init(rank: int, world: int, endpoint: str):
        """Join the node's ranks (one process per GPU); endpoint "tcp://127.0.0.1:port" or a file path."""
        if _load_host().NDArray_CommInit(int(rank), int(world), endpoint.encode()) != 0:
            _raise_pending(_load_host())

    @staticmethod
    def comm_destroy():
        if _load_host().NDArray_CommDestroy() != 0:
            _raise_pending(_load_host())

    @staticmethod
    def sharded_batched_matmul(a_slab, b_slab, batch: int, gather_mode: int = 1):
        """This rank's slab of a batch of `batch` products; gather_mode 0 keeps the result sharded, 1 gathers it
        with one all-gather, k >= 2 overlaps the gather of k pieces with the GEMM (include/numpower_host.h)."""
        h = _load_host()
        return NDArray._wrap(h.NDArray_ShardedBatchedMatmul(a_slab._p, b_slab._p, int(batch), int(gather_mode)))

    @staticmethod
    def live_device_allocations() -> int:
        return int(_load_host().NDArray_LiveDeviceAllocations())


def _install_unary_methods():
    for name in _UNARY_METHODS:
        if hasattr(NDArray, name):
            continue
        setattr(NDArray, name, staticmethod(lambda a, _n=name: NDArray._unary(_n, a)))


_install_unary_methods()
NDArray.negative = NDArray.negate   # PHP method name (numpower.c method table); float_negate underneath
# `abs` goes through NDArray_Abs in the reference (arithmetics.c:934-947); same kernel
nd = NDArray
