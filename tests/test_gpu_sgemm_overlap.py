"""Consecutive independent np_sgemm launches alternate between the library stream and the runtime's side lane
(numpower_amd/csrc/np_sgemm_lane.h, np_runtime.hip).  Nothing of that may show: every sequence here is run with the overlap off
and on and compared BIT FOR BIT, with np_sgemm_overlap_stats() = (side launches, launches on the library stream next to the
lane, launches ordered behind everything) saying which way each launch went.

The size threshold is lowered to 0 (np_sgemm_set_variant(-29)) and the LDS-DMA kernel forced (variant 7), so the shapes stay
small: 256 x 128 x 32, one tile of that kernel, and 512 x 256 x 48, four.  Where a test must SEE a missing join (a consumer
right behind a side launch), the side launch is 1024 x 1024 x 4096 instead — 32 workgroups walking 256 K-tiles, some hundred
microseconds, against the few microseconds after which a consumer that was not ordered behind it would run; its C is filled
with NaN first, so an early consumer reads NaN.  The timer test has its own shape and says why."""
import ctypes as C

import numpy as np
import pytest

from numpower_amd import synth

pytestmark = pytest.mark.gpu

S1 = (256, 128, 32)
S2 = (512, 256, 48)
LONG = (1024, 1024, 4096)


def _stats(lib):
    out = (C.c_ulonglong * 3)()
    assert lib.np_sgemm_overlap_stats(out) == 0, lib.np_last_error()
    return np.array(list(out), dtype=np.int64)


@pytest.fixture
def lib(hip):
    """LDS-DMA kernel forced, every size qualifies, overlap on; everything back to the defaults afterwards."""
    from numpower_amd import _lib
    handle = _lib.load()
    for v in (7, -28, -29):
        _lib.check(handle.np_sgemm_set_variant(v))
    try:
        yield handle
    finally:
        for v in (0, -28, -30):
            _lib.check(handle.np_sgemm_set_variant(v))
        assert handle.np_sync() == 0, handle.np_last_error()


class Arena:
    """One device buffer; operands are windows of it, given as float offsets (so that ranges can be made to abut or share a float)."""

    def __init__(self, hip, floats, seed=1):
        self.D = hip
        self.host = synth.uniform((floats,), seed, -1.0, 1.0)
        self.dev = hip.DeviceArray((floats,))

    def reset(self):
        from numpower_amd import _lib
        _lib.check(_lib.load().np_memcpy_h2d(self.dev.ptr, self.host.ctypes.data, self.host.nbytes))

    def at(self, offset):
        return self.dev.ptr + 4 * offset

    def read(self, offset, rows, cols):
        return self.dev.view(offset, (rows, cols)).to_host()

    def free(self):
        self.dev.free()


def _run(lib, arena, products, on):
    """products: (M, N, K, offset of A, of B, of C), dense.  -> (every C in order, what the stats moved by)"""
    from numpower_amd import _lib
    _lib.check(lib.np_sgemm_set_variant(-28 if on else -27))
    arena.reset()
    _lib.check(lib.np_sync())
    before = _stats(lib)
    for (m, n, k, a, b, c) in products:
        _lib.check(lib.np_sgemm(m, n, k, arena.at(a), arena.at(b), arena.at(c)))
    moved = _stats(lib) - before
    outs = [arena.read(c, m, n) for (m, n, k, a, b, c) in products]
    _lib.check(lib.np_sgemm_set_variant(-28))
    return outs, moved


def _same_bits(xs, ys):
    return all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(xs, ys))


def _layout(shapes, gap=64):
    """Dense A, B, C for every shape, one behind the other in an arena -> (products, floats)."""
    at, products = 0, []
    for (m, n, k) in shapes:
        a, b, c = at, at + m * k + gap, at + m * k + k * n + 2 * gap
        at = c + m * n + gap
        products.append((m, n, k, a, b, c))
    return products, at


@pytest.mark.parametrize("shapes", [[S1, S1], [S2, S2], [S1, S2], [S1, S2, S1, S2, S1], [S2] * 5],
                         ids=["pair 256x128x32", "pair 512x256x48", "mixed pair", "mixed run of 5", "run of 5"])
def test_independent_products_overlap_and_match(shapes, lib, hip):
    products, floats = _layout(shapes)
    arena = Arena(hip, floats)
    off, moved_off = _run(lib, arena, products, on=False)
    on, moved_on = _run(lib, arena, products, on=True)
    n = len(shapes)
    assert moved_off.tolist() == [0, 0, 0]
    # the first is ordered behind everything, then lane and library stream take turns
    assert moved_on.tolist() == [n // 2, (n - 1) // 2, 1], moved_on
    assert _same_bits(off, on)
    m, nn, k, a, b, c = products[-1]
    ref = arena.host[a:a + m * k].reshape(m, k).astype(np.float64) @ arena.host[b:b + k * nn].reshape(k, nn).astype(np.float64)
    assert np.abs(on[-1] - ref).max() <= 1e-5 * k   # |a|, |b| <= 1: fp32 rounding of k terms is far inside this
    arena.free()


def _hazard_cases():
    m, n, k = S1
    a1, b1, c1 = 0, 40000, 80000            # P1 = 256 x 128 x 32: A1 8192 floats, B1 4096, C1 32768
    a2, b2, c2 = 120000, 160000, 200000     # free space for P2's own operands
    p1 = (m, n, k, a1, b1, c1)
    return {
        "RAW: C1 is A2": [p1, (256, 128, 128, c1, b2, c2)],
        "RAW: C1 is B2": [p1, (256, 128, 256, a2, c1, c2)],
        "WAW: same C": [p1, (m, n, k, a2, b2, c1)],
        "WAR: C2 is A1": [(256, 128, 128, a1, b1, c1), (256, 128, 32, a2, b2, a1)],
        "WAR: C2 is B1": [(256, 128, 256, a1, b1, c1), (256, 128, 32, a2, b2, b1)],
        # C2 starts on the last float of A1 (A1 = 256 x 32 at 0: floats 0 .. 8191)
        "C2 starts inside A1's last row": [p1, (m, n, k, a2, b2, a1 + 8191 - 16)],
        "C2 shares one float with A1": [p1, (m, n, k, a2, b2, a1 + 8191)],
        "C2 ends on C1's first float": [p1, (m, n, k, a2, b2, c1 - m * n + 1)],
    }


@pytest.mark.parametrize("behind_a_side_launch", [False, True], ids=["second of a pair", "behind a side launch"])
@pytest.mark.parametrize("case", list(_hazard_cases()))
def test_dependent_products_join(case, behind_a_side_launch, lib, hip):
    """A product that touches the previous one's bytes is ordered behind it by joining — also when the previous one sits on the lane."""
    products = _hazard_cases()[case]
    if "A1's last row" in case or "one float with A1" in case or "first float" in case:
        # P2's C overlaps P1's B or lies in front of C1: keep B1 clear of it
        products = [(products[0][0], products[0][1], products[0][2], products[0][3], 360000, products[0][5]), products[1]]
    if behind_a_side_launch:   # an independent product in front: P1 goes to the lane, P2 must wait for the LANE
        products = [(256, 128, 32, 300000, 310000, 320000)] + products
    arena = Arena(hip, 400000)
    off, _ = _run(lib, arena, products, on=False)
    on, moved = _run(lib, arena, products, on=True)
    if behind_a_side_launch:
        assert moved.tolist() == [1, 0, 2], moved   # first: joined, P1: lane, P2: joined — no side launch for it
    else:
        assert moved.tolist() == [0, 0, 2], moved
    assert _same_bits(off, on)
    arena.free()


def test_abutting_ranges_are_independent(lib, hip):
    """C2 ends exactly where A1 starts, and C3 starts exactly where C2 ends (over A1, whose reader is two launches back on C3's own
    stream): neighbours share no byte, so they overlap."""
    m, n, k = S1
    a1 = 100000
    products = [(m, n, k, a1, 150000, 160000), (m, n, k, 200000, 210000, a1 - m * n), (m, n, k, 250000, 260000, a1)]
    arena = Arena(hip, 300000)
    off, _ = _run(lib, arena, products, on=False)
    on, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [1, 1, 1], moved
    assert _same_bits(off, on)
    arena.free()


def test_same_stream_dependencies_older_than_the_neighbour(lib, hip):
    """Dependencies two launches back sit on the SAME stream: P2 reads C0 (both on the library stream), P3 reads C1 (both on the lane),
    P4 reads C2.  Stream order keeps them; the cross-stream ones are the next test's."""
    m, n, k = 256, 128, 128   # C (256 x 128) is a valid A of the same shape
    at = lambda i: 40000 * i   # noqa: E731
    products = [(m, n, k, at(0), at(1), at(2)), (m, n, k, at(3), at(4), at(5)), (m, n, k, at(2), at(6), at(7)),
                (m, n, k, at(5), at(8), at(9)), (m, n, k, at(7), at(10), at(11))]
    arena = Arena(hip, at(12))
    off, _ = _run(lib, arena, products, on=False)
    on, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [2, 2, 1], moved
    assert _same_bits(off, on)
    arena.free()


@pytest.mark.parametrize("hazard", ["RAW: A4 is C1", "RAW: B4 is C1", "WAW: C4 lies in C1", "WAR: C4 is A1's head"])
@pytest.mark.parametrize("long_on", ["lane", "library stream"])
def test_cross_stream_dependencies_three_launches_back(hazard, long_on, lib, hip):
    """P0 P1 P2 P3 P4 alternate library stream / lane / ...; a launch is compared with its neighbour only, so P4 — independent of P3 —
    goes to the library stream without joining while P1 sits on the LANE.  P1 is a long product (1024 x 1024 x 16384, C1 full of
    NaN until it is done), every other one takes microseconds: unless the library stream is ordered behind what the lane was given
    before P3 (the mark each stream records in front of its launches), P4 runs while P1 is still computing — a P4 that reads C1
    reads NaN, a P4 that writes into C1 is overwritten by P1, a P4 that overwrites A1 changes what P1 computes.  With one more small
    product in front, the long one sits on the library stream and the dependent one on the lane: the same, mirrored."""
    M, N, K = 1024, 1024, 16384   # four times LONG's depth: a millisecond or so, well beyond the host's time for three more launches
    S = (256, 128, 32)
    a1, b1, c1 = 0, M * K, M * K + K * N                 # the long product's operands
    free = c1 + M * N                                    # small operands from here on, 40000 floats apart
    at = lambda i: free + 40000 * i                      # noqa: E731
    small = lambda i: S + (at(3 * i), at(3 * i + 1), at(3 * i + 2))   # noqa: E731
    if hazard == "RAW: A4 is C1":
        last = (M, 128, N, c1, at(20), at(24))           # A4 = C1 (1024 x 1024), B4 1024 x 128 (131072 floats), C4 1024 x 128
        floats = at(24) + M * 128
    elif hazard == "RAW: B4 is C1":
        last = (256, N, M, at(20), c1, at(27))           # A4 256 x 1024 (262144 floats), B4 = C1, C4 256 x 1024
        floats = at(27) + 256 * N
    elif hazard == "WAW: C4 lies in C1":
        last = S + (at(20), at(21), c1 + 4096)
        floats = at(22)
    else:
        last = S + (at(20), at(21), a1)                  # C4 = the first 32768 floats of A1
        floats = at(22)
    products = [small(0), (M, N, K, a1, b1, c1), small(1), small(2), last]
    if long_on == "library stream":
        products = [small(3)] + products
    arena = Arena(hip, floats)
    nan = np.full((M, N), np.nan, dtype=np.float32)
    arena.host[c1:c1 + M * N] = nan.ravel()              # reset() uploads it: C1 is NaN until P1 has stored it
    off, moved_off = _run(lib, arena, products, on=False)
    on, moved = _run(lib, arena, products, on=True)
    assert moved_off.tolist() == [0, 0, 0]
    n = len(products)
    assert moved.tolist() == [n // 2, (n - 1) // 2, 1], moved   # nobody joins: the marks order the streams
    assert np.isfinite(off[-1]).all() and np.isfinite(off[-4]).all()
    assert _same_bits(off, on)
    # what the memory holds at the end (the WAW / WAR orders), not only what each product's window reads back as
    arena_off = None
    for on_ in (False, True):
        _run(lib, arena, products, on=on_)
        whole = arena.dev.to_host()
        if arena_off is None:
            arena_off = whole
        else:
            assert (whole.view(np.uint32) == arena_off.view(np.uint32)).all()
    arena.free()


def _side_launch_of_a_long_product(lib, hip, seed=5):
    """One small product on the library stream, then LONG on the lane into a C full of NaN -> (its operands, C, what the stats moved by)."""
    from numpower_amd import _lib
    m, n, k = LONG
    a = hip.DeviceArray.from_host(synth.uniform((m, k), seed, -1.0, 1.0))
    b = hip.DeviceArray.from_host(synth.uniform((k, n), seed + 1, -1.0, 1.0))
    c = hip.DeviceArray((m, n))
    hip.fill(c, float("nan"))
    s = [hip.DeviceArray.from_host(synth.uniform(sh, seed + 2 + i, -1.0, 1.0)) for i, sh in enumerate(((256, 32), (32, 128)))]
    s.append(hip.DeviceArray((256, 128)))
    _lib.check(lib.np_sync())
    before = _stats(lib)
    _lib.check(lib.np_sgemm(256, 128, 32, s[0].ptr, s[1].ptr, s[2].ptr))
    _lib.check(lib.np_sgemm(m, n, k, a.ptr, b.ptr, c.ptr))
    return [a, b] + s, c, _stats(lib) - before


@pytest.fixture
def long_reference(lib, hip):
    """LONG's product with the overlap off, once per test."""
    from numpower_amd import _lib
    _lib.check(lib.np_sgemm_set_variant(-27))
    held, c, moved = _side_launch_of_a_long_product(lib, hip)
    assert moved.tolist() == [0, 0, 0]
    ref = c.to_host()
    for d in held + [c]:
        d.free()
    _lib.check(lib.np_sgemm_set_variant(-28))
    assert np.isfinite(ref).all()
    return ref


def _hip_runtime():
    """The HIP runtime the library itself is linked against (already in the process)."""
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64.so" in line}
    assert paths, "libamdhip64.so is not loaded"
    return C.CDLL(sorted(paths)[0])


def _raw_read(ptr, shape):
    """Device memory read by the HIP runtime itself, behind the library's back: no library stream, no join."""
    rt = _hip_runtime()
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(shape, dtype=np.float32)
    assert rt.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0   # 2 = hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("consumer", ["to_host", "elementwise", "reduce_all", "memcpy_d2d", "free_malloc_fill", "sync"])
def test_a_consumer_right_behind_a_side_launch_sees_the_product(consumer, lib, hip, long_reference):
    from numpower_amd import _lib
    ref = long_reference
    held, c, moved = _side_launch_of_a_long_product(lib, hip)
    assert moved.tolist() == [1, 0, 1], moved
    m, n, _ = LONG
    if consumer == "to_host":
        got = c.to_host()
    elif consumer == "elementwise":
        neg = hip.unary("negate", c)
        got = -neg.to_host()
        neg.free()
    elif consumer == "reduce_all":
        total = hip.reduce_all("sum", c)   # NaN if it ran over a C the product had not finished
        assert np.float32(total).view(np.uint32) == np.float32(hip.reduce_all("sum", c)).view(np.uint32)
        assert np.isfinite(total)
        got = c.to_host()
    elif consumer == "memcpy_d2d":
        copy = hip.DeviceArray((m, n))
        _lib.check(lib.np_memcpy_d2d(copy.ptr, c.ptr, 4 * m * n))
        got = copy.to_host()
        copy.free()
    elif consumer == "free_malloc_fill":
        old = c.ptr
        c.free()
        c = hip.DeviceArray((m, n))
        assert c.ptr == old   # the pool hands the block straight back: the fill below lands on the GEMM's C
        hip.fill(c, 7.0)
        got = c.to_host()
        assert (got == 7.0).all()   # a fill that overtook the GEMM would have been overwritten by it
        got = ref
    else:
        _lib.check(lib.np_sync())
        got = _raw_read(c.ptr, (m, n))
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    for d in held + [c]:
        d.free()


@pytest.mark.parametrize("count", [4, 5])
def test_timer_covers_the_lane(count, lib, hip):
    """start, `count` independent products, stop: the stop event must be behind all of them, the lane's too.  The products are
    4096 x 4096 x 1024: 512 workgroups, one full round of the machine like the headline's, so two of them cannot run side by side and
    all the overlap can hide is the store tail (a few per cent; measured on / off = 0.979 for four).  The region with the overlap on
    must take at least the time with it off minus 20 %.  What a stop event recorded on the library stream WITHOUT the join would
    give: with four products the last one is on the lane and the library stream ends with P2, about one product time early — 3 of 4
    product times, 0.75 of the off time, just under the bound; with five the last one is on the library stream behind the lane's
    mark, and an unjoined stop event loses nothing — that count is here for the start of the region and for the odd run itself.
    Medians of 5."""
    from numpower_amd import _lib
    m, n, k = 4096, 4096, 1024
    a = hip.DeviceArray.from_host(synth.uniform((m, k), 20, -1.0, 1.0))
    b = hip.DeviceArray.from_host(synth.uniform((k, n), 21, -1.0, 1.0))
    cs = [hip.DeviceArray((m, n)) for _ in range(count)]

    def elapsed(on):
        _lib.check(lib.np_sgemm_set_variant(-28 if on else -27))
        ms = []
        for _ in range(6):
            t = _lib.Timer()
            _lib.check(lib.np_sync())
            before = _stats(lib)
            t.start()
            for c in cs:
                _lib.check(lib.np_sgemm(m, n, k, a.ptr, b.ptr, c.ptr))
            t.stop()
            ms.append(t.elapsed_ms())
            assert (_stats(lib) - before).tolist() == ([count // 2, (count - 1) // 2, 1] if on else [0, 0, 0])
        return float(np.median(ms[1:]))   # (the first round warms up)

    off = elapsed(False)
    on = elapsed(True)
    print("timer: %d 4096 x 4096 x 1024 products, overlap off %.4f ms, on %.4f ms, on / off = %.3f" % (count, off, on, on / off))
    assert on >= 0.8 * off, (on, off)
    for d in [a, b] + cs:
        d.free()


def test_graph_capture_takes_no_side_launch(lib, hip):
    from numpower_amd import _lib
    products, floats = _layout([S1, S2])
    arena = Arena(hip, floats)
    eager, _ = _run(lib, arena, products, on=False)
    _lib.check(lib.np_sync())
    before = _stats(lib)
    _lib.check(lib.np_graph_begin())
    for (m, n, k, a, b, c) in products:
        _lib.check(lib.np_sgemm(m, n, k, arena.at(a), arena.at(b), arena.at(c)))
    g = C.c_void_p()
    _lib.check(lib.np_graph_end(C.byref(g)))
    assert (_stats(lib) - before).tolist() == [0, 0, 0]   # a capturing stream is outside the gate altogether
    for _ in range(2):
        for (m, n, k, a, b, c) in products:
            hip.fill(arena.dev.view(c, (m, n)), float("nan"))
        _lib.check(lib.np_graph_launch(g))
        assert _same_bits(eager, [arena.read(c, m, n) for (m, n, k, a, b, c) in products])
    _lib.check(lib.np_graph_destroy(g))
    # ... and behind the capture the overlap is back
    on, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [1, 0, 1] and _same_bits(eager, on)
    arena.free()


def test_a_callers_stream_takes_no_side_launch(lib, hip):
    from numpower_amd import _lib
    rt = _hip_runtime()
    rt.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipStreamDestroy.argtypes = [C.c_void_p]
    products, floats = _layout([S1, S2, S1])
    arena = Arena(hip, floats)
    off, _ = _run(lib, arena, products, on=False)
    user = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(user)) == 0
    try:
        _lib.check(lib.np_set_stream(user))
        got, moved = _run(lib, arena, products, on=True)
        assert moved.tolist() == [0, 0, 0], moved
        assert _same_bits(off, got)
    finally:
        _lib.check(lib.np_set_stream(None))
        assert rt.hipStreamDestroy(user) == 0
    got, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [1, 1, 1], moved
    assert _same_bits(off, got)
    arena.free()


def test_off_switch_and_size_threshold(lib, hip):
    from numpower_amd import _lib
    products, floats = _layout([S1, S2, S1, S2])
    arena = Arena(hip, floats)
    _, moved = _run(lib, arena, products, on=False)
    assert moved.tolist() == [0, 0, 0]
    # the default threshold (4e9 flop) leaves products of this size alone, overlap on or not
    _lib.check(lib.np_sgemm_set_variant(-30))
    _, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [0, 0, 0]
    _lib.check(lib.np_sgemm_set_variant(-29))
    _, moved = _run(lib, arena, products, on=True)
    assert moved.tolist() == [2, 1, 1]
    arena.free()
