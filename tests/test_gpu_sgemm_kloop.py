"""The two K loops of the 256 x 128 LDS-DMA kernels (dma_gemm_segment in numpower_amd/csrc/np_sgemm.hip): flat per-lane source
pointers and a run-time LDS buffer index (np_sgemm_set_variant(-31)) against buffer-addressed sources and three K-tiles per trip
(-32, taken only where the launch is eligible).  The order in which every element of C is accumulated is the same in both, so each
case compares them BIT FOR BIT; the new loop's result is also held against fp64 within the bound of tests/test_gpu_streamk.py
(1e-6 of |A|.|B|).  np_sgemm_debug_kloop_stats() = (launches on the buffer-addressed loop, launches on the flat one) says which
loop a launch ran.

The kernel is forced by variant 7, so the shapes stay small: one tile is 256 x 128, a K-tile 16 deep, a trip three K-tiles with
five ahead of it — K = 16 n for n = 1 .. 8 walks through every number of trips from 0 to 2 and every remainder 1 .. 4 behind
them; 17, 31, 32 and 256 K-tiles are deeper mixes, the last one (K = 4096) the instantiation that alternates wave priorities
every 5 trips."""
import ctypes as C

import numpy as np
import pytest

from numpower_amd import synth

pytestmark = pytest.mark.gpu

OLD, NEW = -31, -32
DEFAULT_LOOP = -33  # what np_sgemm_set_variant leaves on when nothing was asked for (include/np_hip_debug.h)


def _stats(lib):
    out = (C.c_ulonglong * 2)()
    assert lib.np_sgemm_debug_kloop_stats(out) == 0, lib.np_last_error()
    return np.array(list(out), dtype=np.int64)


@pytest.fixture
def lib(hip):
    """LDS-DMA kernel forced; everything back to the defaults afterwards."""
    from numpower_amd import _lib
    handle = _lib.load()
    _lib.check(handle.np_sgemm_set_variant(7))
    try:
        yield handle
    finally:
        for v in (0, -2, -28, -30, DEFAULT_LOOP):
            _lib.check(handle.np_sgemm_set_variant(v))
        assert handle.np_sync() == 0, handle.np_last_error()


def _same_bits(x, y):
    return bool((x.view(np.uint32) == y.view(np.uint32)).all())


def _within_fp64(c, A, B):
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    scale = np.abs(A64) @ np.abs(B64)
    return float((np.abs(c - A64 @ B64) / scale).max()) <= 1e-6


def _both_loops(lib, launch, read):
    """launch() under -31 and under -32 -> (C of the flat loop, C of the buffer loop, stats moved by each)."""
    from numpower_amd import _lib
    got, moved = {}, {}
    for loop in (OLD, NEW):
        _lib.check(lib.np_sgemm_set_variant(loop))
        before = _stats(lib)
        launch()
        moved[loop] = (_stats(lib) - before).tolist()
        got[loop] = read()
    return got[OLD], got[NEW], moved[OLD], moved[NEW]


def _dense_case(lib, hip, m, n, k, seed=11):
    from numpower_amd import _lib
    A = synth.uniform((m, k), seed, -1.0, 1.0)
    B = synth.uniform((k, n), seed + 1, -1.0, 1.0)
    dA, dB, dC = hip.DeviceArray.from_host(A), hip.DeviceArray.from_host(B), hip.DeviceArray((m, n))

    def launch():
        hip.fill(dC, float("nan"))
        _lib.check(lib.np_sgemm(m, n, k, dA.ptr, dB.ptr, dC.ptr))

    out = _both_loops(lib, launch, dC.to_host)
    for d in (dA, dB, dC):
        d.free()
    return (A, B) + out


@pytest.mark.parametrize("ktiles", [1, 2, 3, 4, 5, 6, 7, 8, 17, 31, 32, 256])
def test_one_tile_every_head_and_tail_of_the_unroll(ktiles, lib, hip):
    A, B, old, new, moved_old, moved_new = _dense_case(lib, hip, 256, 128, 16 * ktiles)
    assert moved_old == [0, 1] and moved_new == [1, 0], (moved_old, moved_new)
    assert _same_bits(old, new)
    assert _within_fp64(new, A, B)


def test_tile_bases_off_zero(lib, hip):
    A, B, old, new, moved_old, moved_new = _dense_case(lib, hip, 512, 256, 112)
    assert moved_old == [0, 1] and moved_new == [1, 0]
    assert _same_bits(old, new)
    assert _within_fp64(new, A, B)


@pytest.mark.parametrize("shape", [(257, 132, 48), (255, 124, 64), (300, 260, 80)], ids=lambda s: "%dx%dx%d" % s)
def test_edge_tiles_without_a_k_tail(shape, lib, hip):
    m, n, k = shape
    A, B, old, new, moved_old, moved_new = _dense_case(lib, hip, m, n, k)
    assert moved_old == [0, 1] and moved_new == [1, 0]
    assert _same_bits(old, new)
    assert _within_fp64(new, A, B)


def test_padded_leading_dimensions_on_a_window(lib, hip):
    """A 512 x 256 x 96 product on windows of larger buffers, lda = K + 4, ldb = N + 8, ldc = N + 4, one row in front of each window
    and one behind it.  Everything of A and B outside the windows is NaN: nothing of it may reach C.  C's buffer holds a pattern:
    every byte outside the window must still hold it."""
    from numpower_amd import _lib
    m, n, k = 512, 256, 96
    lda, ldb, ldc = k + 4, n + 8, n + 4
    A = synth.uniform((m, k), 21, -1.0, 1.0)
    B = synth.uniform((k, n), 22, -1.0, 1.0)
    bufA = np.full((m + 2, lda), np.nan, dtype=np.float32)
    bufA[1:m + 1, :k] = A
    bufB = np.full((k + 2, ldb), np.nan, dtype=np.float32)
    bufB[1:k + 1, :n] = B
    pattern = synth.uniform((m + 2, ldc), 23, 100.0, 200.0)
    dA, dB, dC = hip.DeviceArray.from_host(bufA), hip.DeviceArray.from_host(bufB), hip.DeviceArray((m + 2, ldc))

    def launch():
        _lib.check(lib.np_memcpy_h2d(dC.ptr, pattern.ctypes.data, pattern.nbytes))
        _lib.check(lib.np_sgemm_debug_ld(m, n, k, dA.ptr + 4 * lda, lda, dB.ptr + 4 * ldb, ldb, dC.ptr + 4 * ldc, ldc))

    old, new, moved_old, moved_new = _both_loops(lib, launch, dC.to_host)
    assert moved_old == [0, 1] and moved_new == [1, 0]
    outside = np.ones((m + 2, ldc), dtype=bool)
    outside[1:m + 1, :n] = False
    for got in (old, new):
        assert _same_bits(got[outside], pattern[outside])
    assert _same_bits(old, new)
    window = np.ascontiguousarray(new[1:m + 1, :n])
    assert np.isfinite(window).all()
    assert _within_fp64(window, A, B)
    for d in (dA, dB, dC):
        d.free()


def test_strided_batch_of_three(lib, hip):
    from numpower_amd import _lib
    bt, m, n, k = 3, 256, 256, 80
    A = synth.uniform((bt, m, k), 31, -1.0, 1.0)
    B = synth.uniform((bt, k, n), 32, -1.0, 1.0)
    dA, dB, dC = hip.DeviceArray.from_host(A), hip.DeviceArray.from_host(B), hip.DeviceArray((bt, m, n))

    def launch():
        hip.fill(dC, float("nan"))
        _lib.check(lib.np_sgemm_strided_batched(bt, m, n, k, dA.ptr, m * k, dB.ptr, k * n, dC.ptr, m * n))

    old, new, moved_old, moved_new = _both_loops(lib, launch, dC.to_host)
    assert moved_old == [0, 1] and moved_new == [1, 0]
    assert _same_bits(old, new)
    for b in range(bt):
        assert _within_fp64(new[b], A[b], B[b])
    for d in (dA, dB, dC):
        d.free()


# The stream-K model wants ranges of at least 24 K-tiles on 256 or 512 workgroups: the first two shapes are far below that, the
# planner places them on other kernels even with stream-K forced, and the two knob settings then run the very same launch.  The third
# one — four tiles, 1537 K-tiles each, 25 per workgroup, ranges that straddle tiles — is a shape stream-K really takes.
@pytest.mark.parametrize("shape,takes", [((768, 384, 208), False), ((512, 640, 112), False), ((512, 256, 16 * 1537), True)],
                         ids=["768x384x208", "512x640x112", "512x256x24592"])
def test_stream_k_forced(shape, takes, lib, hip):
    from numpower_amd import _lib
    m, n, k = shape
    for v in (0, -4):
        _lib.check(lib.np_sgemm_set_variant(v))
    plan = (C.c_double * 11)()
    _lib.check(lib.np_sgemm_debug_plan(m, n, k, 1, 0, plan))
    assert bool(plan[4]) == takes
    A, B, old, new, moved_old, moved_new = _dense_case(lib, hip, m, n, k)
    if takes:
        assert moved_old == [0, 1] and moved_new == [1, 0]
    assert _same_bits(old, new)
    assert _within_fp64(new, A, B)


@pytest.mark.parametrize("case", ["K and N tail: 256x130x50", "A 4 bytes off", "B 4 bytes off"])
def test_ineligible_launches_run_the_flat_loop(case, lib, hip):
    from numpower_amd import _lib
    m, n, k = (256, 130, 50) if "tail" in case else (256, 128, 32)
    A = synth.uniform((m, k), 41, -1.0, 1.0)
    B = synth.uniform((k, n), 42, -1.0, 1.0)
    offA, offB = int(case.startswith("A")), int(case.startswith("B"))
    dA, dB, dC = hip.DeviceArray((m * k + 1,)), hip.DeviceArray((k * n + 1,)), hip.DeviceArray((m, n))
    _lib.check(lib.np_memcpy_h2d(dA.ptr + 4 * offA, A.ctypes.data, A.nbytes))
    _lib.check(lib.np_memcpy_h2d(dB.ptr + 4 * offB, B.ctypes.data, B.nbytes))

    def launch():
        hip.fill(dC, float("nan"))
        _lib.check(lib.np_sgemm(m, n, k, dA.ptr + 4 * offA, dB.ptr + 4 * offB, dC.ptr))

    old, new, moved_old, moved_new = _both_loops(lib, launch, dC.to_host)
    assert moved_old == [0, 1] and moved_new == [0, 1], (moved_old, moved_new)   # -32 asked for, the flat loop ran
    assert _same_bits(old, new)
    assert _within_fp64(new, A, B)
    for d in (dA, dB, dC):
        d.free()


def test_sixteen_independent_products_with_the_side_lane(lib, hip):
    from numpower_amd import _lib
    m, n, k, count = 512, 256, 64, 16
    for v in (-28, -29):
        _lib.check(lib.np_sgemm_set_variant(v))
    A = [synth.uniform((m, k), 50 + i, -1.0, 1.0) for i in range(count)]
    B = synth.uniform((k, n), 49, -1.0, 1.0)
    dA = [hip.DeviceArray.from_host(a) for a in A]
    dB = hip.DeviceArray.from_host(B)
    dC = [hip.DeviceArray((m, n)) for _ in range(count)]
    lane = (C.c_ulonglong * 3)()

    def launch():
        for c in dC:
            hip.fill(c, float("nan"))
        _lib.check(lib.np_sync())
        _lib.check(lib.np_sgemm_overlap_stats(lane))
        side = lane[0]
        for a, c in zip(dA, dC):
            _lib.check(lib.np_sgemm(m, n, k, a.ptr, dB.ptr, c.ptr))
        _lib.check(lib.np_sgemm_overlap_stats(lane))
        assert lane[0] - side == count // 2   # every second one went to the lane

    old, new, moved_old, moved_new = _both_loops(lib, launch, lambda: [c.to_host() for c in dC])
    assert moved_old == [0, count] and moved_new == [count, 0]
    assert all(_same_bits(x, y) for x, y in zip(old, new))
    assert _within_fp64(new[-1], A[-1], B)
    for d in dA + dC + [dB]:
        d.free()
