"""np_sgd_step on a single tensor of 2^31 + 4099 elements (8.6 GB per buffer): the one case that can catch a 32-bit element index
or chunk offset in the step kernel.  The device fills the operands (np_fill; a varied block is copied over the first and the last
2^16 elements, so that an index that wraps would meet other values), computes the expectation itself with np_binary
(p - lr . g: a multiply by a scalar, then a subtract, the two roundings of the plain step) and compares all the elements with
np_count_mismatch; nothing of that size crosses to the host."""
import ctypes as C

import numpy as np
import pytest

from tests import optim_family as fam

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_plain_sgd_past_2_to_31_elements(hip):
    from numpower_amd import _lib
    from numpower_amd._lib import BINARY_OPS
    lib = _lib.load()
    n = (1 << 31) + 4099
    lr = 0.125
    p, g, want = (_lib.DeviceBuffer(4 * n) for _ in range(3))
    try:
        _lib.check(lib.np_fill(p.ptr, 1.5, n))
        _lib.check(lib.np_fill(g.ptr, -2.0, n))
        rng = np.random.default_rng(80)
        block = 1 << 16
        edges = [fam.gaussian(rng, block) for _ in range(4)]
        for buf, (head, tail) in ((p, edges[:2]), (g, edges[2:])):
            _lib.check(lib.np_memcpy_h2d(buf.ptr, head.ctypes.data, 4 * block))
            _lib.check(lib.np_memcpy_h2d(buf.ptr + 4 * (n - block), tail.ctypes.data, 4 * block))
        rate = np.array([lr], F32)
        _lib.check(lib.np_binary(BINARY_OPS["multiply"], g.ptr, _lib.NP_FULL, rate.ctypes.data, 4, want.ptr, 1, n, 0, 0))      # 4: NP_HOST_SCALAR
        _lib.check(lib.np_binary(BINARY_OPS["subtract"], p.ptr, _lib.NP_FULL, want.ptr, _lib.NP_FULL, want.ptr, 1, n, 0, 0))
        any_ = C.c_int(-1)
        _lib.check(lib.np_count_mismatch(0, p.ptr, want.ptr, n, 0.0, 0.0, C.byref(any_)))
        assert any_.value == 1                                   # the expectation differs from the parameter before the step ...
        params, grads, counts = (C.c_void_p * 1)(p.ptr), (C.c_void_p * 1)(g.ptr), (C.c_size_t * 1)(n)
        _lib.check(lib.np_sgd_step(params, grads, None, counts, 1, lr, 0.0, 0.0, 0.0, 0, 0, None))
        launches, chunks, vec, scalar = C.c_int(), C.c_size_t(), C.c_int(), C.c_int()
        _lib.check(lib.np_debug_optim_last_path(C.byref(launches), C.byref(chunks), C.byref(vec), C.byref(scalar)))
        assert (launches.value, chunks.value, vec.value, scalar.value) == fam.plan([(n, [p.ptr, g.ptr])]) == (1, (1 << 19) + 2, 1, 0)
        _lib.check(lib.np_count_mismatch(0, p.ptr, want.ptr, n, 0.0, 0.0, C.byref(any_)))
        assert any_.value == 0                                   # ... and equals it in every element after
        host = np.empty(block, F32)
        _lib.check(lib.np_memcpy_d2h(host.ctypes.data, p.ptr + 4 * (n - block), 4 * block))
        assert host.tobytes() == fam.sgd_step(edges[1], edges[3], lr=lr)[0].tobytes()      # the far end against the evaluator
    finally:
        for buf in (p, g, want):
            buf.free()
