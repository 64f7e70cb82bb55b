"""The layout kernels (np_layout.hip) against the exact family (tests/layout_family.py), through the C ABI.  Every launch of this
module

  * moves the family's bit patterns (denormals, -0, both infinities, quiet and signalling NaN payloads, every element distinct)
    from an input inside a frame of input canaries to an output inside a frame of output canaries, and the WHOLE output
    allocation is compared bit for bit: one float written outside the output, or read outside the input, fails;
  * asserts the whole record of np_debug_layout_last_record (kernel family, template arguments, tile order, grid, tile counts
    and pitches or the plane kernel's tile) against the dispatcher restated on the host (plan_transpose2d / plan_permute /
    plan_strided_copy / plan_copy2d), exactly one record per call;
  * names the kernel instantiation it was written for; where the plan does not show it the case FAILS, it does not skip.

The size-gated kernels are reached at small shapes with np_debug_set_cus(1) and the np_layout_set_variant knobs, inside state(),
which puts everything back on every way out.  A few cases per family run at the device's own CU count; their names are written
for 256 CUs.

Not here: the 64-bit-index gather (2^31 elements and more).  tests/test_gpu_fullsize.py launches permute_gather_kernel<uint64_t, 1> twice
(a permute and a negative-stride np_strided_copy) without reading the probe; <uint64_t, 4> runs under no test (docs/COVERAGE.md).
Not reachable through the entry points: a transpose that loses its VEC form to a batch stride alone — every batch stride np_permute
and np_transpose2d build is a multiple of rows or cols (tests/test_layout_reference_cpu.py searches for a counterexample).
"Output off by 32 floats" is still 128-byte aligned and is TAKEN by the write-aligned kernel (with 32 canaries in front of it);
the refusals are the offsets 4 and 16.

Each launch prints `LAYOUT-RECORD <what> | <record>` (pytest -s): tools/layout_exact_log.py makes profiles/layout/exact_tests.log
from that output."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from numpower_amd import _lib
from tests import layout_family as lf

pytestmark = pytest.mark.gpu


class Dev:
    def __init__(self):
        self.L = _lib.load()
        cus = C.c_int()
        _lib.check(self.L.np_debug_cus(C.byref(cus)))
        self.cus = cus.value

    def upload(self, image):
        buf = _lib.DeviceBuffer(image.nbytes)
        assert buf.ptr % 128 == 0
        _lib.check(self.L.np_memcpy_h2d(buf.ptr, image.ctypes.data, image.nbytes))
        return buf

    def download(self, buf, count):
        out = np.empty(count, np.uint32)
        _lib.check(self.L.np_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes))
        return out

    def record(self):
        words, count = (C.c_uint * lf.RECORD_WORDS)(*([0xEEEEEEEE] * lf.RECORD_WORDS)), C.c_uint(99)
        _lib.check(self.L.np_debug_layout_last_record(words, 1, C.byref(count)))
        assert count.value <= 1, "np_debug_layout_last_record: %d records for one call" % count.value
        return tuple(words) if count.value else None


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


@contextlib.contextmanager
def state(dev, cus=0, knobs=lf.Knobs()):
    """The CU count the planners assume (0 = the device's own) and the layout knobs, put back on every way out."""
    try:
        _lib.check(dev.L.np_debug_set_cus(cus))
        for code in knobs.codes():
            _lib.check(dev.L.np_layout_set_variant(code))
        yield cus if cus else dev.cus
    finally:
        dev.L.np_debug_set_cus(0)
        for code in lf.DEFAULT_CODES:
            dev.L.np_layout_set_variant(code)


def launch(dev, what, path, payload, in_off, want_of, out_n, out_off, call, plan, salt=0):
    """One call: payload (uint32) framed at in_off -> an output of out_n floats framed at out_off.  call(a_in, a_out) makes the
    C call, plan(a_in, a_out) is the record expected, want_of(out_off) the whole expected allocation, path the instantiation."""
    bin_ = dev.upload(lf.framed_input(payload, in_off))
    bout = dev.upload(lf.blank_output(out_n, out_off))
    try:
        a_in, a_out = bin_.ptr + 4 * in_off, bout.ptr + 4 * out_off
        want_rec = plan(a_in, a_out)
        _lib.check(call(a_in, a_out))
        got_rec = dev.record()
        want = want_of(out_off)
        got = dev.download(bout, want.size)
        back = dev.download(bin_, in_off + payload.size + lf.IN_TAIL)
    finally:
        bin_.free()
        bout.free()
    print("LAYOUT-RECORD %s | %s" % (what, lf.describe(got_rec)))
    assert got_rec == want_rec, "%s: the probe says %s, the plan %s" % (what, lf.describe(got_rec), lf.describe(want_rec))
    assert lf.instantiation(want_rec) == path, "%s was written for %s; the plan shows %s" % (what, path, lf.instantiation(want_rec))
    if not (got == want).all():
        i = int(np.flatnonzero(got != want)[0])
        where = "output element %d" % (i - out_off) if out_off <= i < out_off + out_n else "canary word %d (output at %d .. %d)" % (i, out_off, out_off + out_n)
        raise AssertionError("%s [%s]: %d words differ, first at %s: got 0x%08x (source index %s), want 0x%08x (source index %s)" % (
            what, lf.describe(got_rec), int((got != want).sum()), where, got[i], lf.source_index(got[i], salt), want[i], lf.source_index(want[i], salt)))
    assert (back == lf.framed_input(payload, in_off)).all(), "%s: the input allocation changed" % what


def transpose2d(dev, cus, knobs, batch, rows, cols, in_off, out_off, path, salt=0, tag=""):
    n = batch * rows * cols
    payload = lf.words(n, salt)
    launch(dev, "transpose2d %s(%d, %d, %d) in+%d out+%d cus=%d %s" % (tag, batch, rows, cols, in_off, out_off, cus, knobs.codes()), path,
           payload, in_off, lambda off: lf.expect((batch, rows, cols), (0, 2, 1), salt, off), n, out_off,
           lambda a, b: dev.L.np_transpose2d(a, b, batch, rows, cols),
           lambda a, b: lf.plan_transpose2d(batch, rows, cols, a, b, cus, knobs), salt)


def permute(dev, cus, knobs, shape, perm, in_off, out_off, path, salt=0):
    n = int(np.prod(shape, dtype=np.int64))
    sh, pm = (C.c_int * len(shape))(*shape), (C.c_int * len(shape))(*perm)
    launch(dev, "permute %s %s in+%d out+%d cus=%d %s" % (shape, perm, in_off, out_off, cus, knobs.codes()), path,
           lf.words(n, salt), in_off, lambda off: lf.expect(shape, perm, salt, off), n, out_off,
           lambda a, b: dev.L.np_permute(a, b, len(shape), sh, pm),
           lambda a, b: lf.plan_permute(shape, perm, a, b, cus, knobs), salt)


# ---- the write-aligned transpose ---------------------------------------------------------------------------------------------

def _walign_knobs(tile, order):
    return lf.Knobs(walign64_below=1200 if tile == 64 else 0, walign_order=order)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("r", range(1, 32))
def test_walign_every_shift(r, tile, dev):
    """rows = 256 + r: out_pitch % 32 = r, every per-column shift (o * r) & 31 and both parities of the LDS pitch; cols 129 (ragged),
    130 (in_pitch % 4 != 0) and 192 (vec_in); orders 0, 1, 2; 6 tiles of 128 or 15 of 64 (% 8 != 0), three / five tile rows: the halo
    above row 0 (R < 0), ocol < 0 at the left edge and the last tile's overhang past `rows` all occur.  Output at 0 and at 32
    floats (both on the 128-byte grid; 32 canaries in front)."""
    rows = 256 + r
    for cols in (129, 130, 192):
        for order in (0, 1, 2):
            knobs = _walign_knobs(tile, order)
            with state(dev, 1, knobs) as cus:
                transpose2d(dev, cus, knobs, 1, rows, cols, 0, 0 if order == 1 else 32, "WALIGN<%d> order=%d" % (tile, order), salt=r % 8)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("rows,cols,tiles", [(357, 129, (8, 21)), (449, 192, (8, 24)), (481, 64, (4, 8)), (290, 385, (12, 42)),
                                             (257, 1000, (24, 80))])
def test_walign_tile_counts(rows, cols, tiles, tile, dev):
    """Tile counts that are multiples of 8 (the XCD-run bijection with r = 0) next to those that are not, four tile rows, one tile
    column, in_off 1 (dword-aligned loads), a batch of 1; `tiles` = the counts at tile 128 and 64."""
    for order in (0, 1, 2):
        knobs = _walign_knobs(tile, order)
        with state(dev, 1, knobs) as cus:
            rec = lf.plan_transpose2d(1, rows, cols, 0, 0, cus, knobs)
            assert rec[lf.GRID_X] == tiles[0 if tile == 128 else 1]
            transpose2d(dev, cus, knobs, 1, rows, cols, order % 2, 32, "WALIGN<%d> order=%d" % (tile, order), salt=3)


@pytest.mark.parametrize("case", ["rows255", "cols63", "cols64", "out+4", "out+16", "out+32", "batch3_odd_plane", "batch3_plane%32", "variant1"])
def test_walign_refusals(case, dev):
    """Each condition of the write-aligned form alone — every other condition holds in the case, so deleting the one guard would
    change the record: rows < 256, cols < 64 (513 x 63, one plane, out_pitch % 32 = 1; 513 x 64 is taken), an output off the
    128-byte grid (4 and 16 floats; 32 floats is on it again and is taken), a batch whose planes are not whole lines apart — and
    the same batch taken when they are."""
    knobs = lf.Knobs()
    batch, rows, cols, out_off, path = 1, 259, 130, 0, "TILE<128,VEC=0> order=0"
    if case == "rows255":
        rows, cols = 255, 260
    elif case == "cols63":
        rows, cols = 513, 63           # five tiles of 128 on one CU; no batch stride to refuse it as well
    elif case == "cols64":
        rows, cols, path = 513, 64, "WALIGN<64> order=1"
    elif case.startswith("out+"):
        out_off = int(case[4:])
        path = "WALIGN<64> order=1" if out_off == 32 else path
    elif case == "batch3_odd_plane":
        batch = 3                      # 259 * 130 % 32 = 6
    elif case == "batch3_plane%32":
        batch, rows, cols, path = 3, 259, 128, "WALIGN<64> order=1"       # 259 * 128 % 32 = 0
    elif case == "variant1":
        knobs = lf.Knobs(tile=1)
    with state(dev, 1, knobs) as cus:
        transpose2d(dev, cus, knobs, batch, rows, cols, 0, out_off, path, salt=5)


# ---- the tile kernel ---------------------------------------------------------------------------------------------------------

TILE_SHAPES = [(17, 17), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (191, 257), (257, 191), (17, 257), (257, 17),
               (64, 128), (128, 64), (129, 257), (257, 129), (64, 192)]


@pytest.mark.parametrize("rows,cols", TILE_SHAPES)
def test_tile_shapes(rows, cols, dev):
    """One, two and three tiles each way at both tile sizes, forced (variants 64 / 128) and by the CU rule (one CU: 128 from four
    tiles of 128 up, else 64), batches of 1 and 3, launch order and the forced XCD runs (17011)."""
    vec = 1 if rows % 4 == 0 and cols % 4 == 0 else 0
    for batch in (1, 3):
        for tile_knob in (64, 128, 1):            # 1: the CU rule without the write-aligned form
            for order in (0, 1):
                knobs = lf.Knobs(tile=tile_knob, tile_order=order if order else -1)
                tile = tile_knob if tile_knob > 1 else (128 if lf._ceil(rows, 128) * lf._ceil(cols, 128) * batch >= 4 else 64)
                with state(dev, 1, knobs) as cus:
                    transpose2d(dev, cus, knobs, batch, rows, cols, 0, 0, "TILE<%d,VEC=%d> order=%d" % (tile, vec, order), salt=(rows + cols) % 8)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("reason", ["vec", "rows%4", "cols%4", "in+1", "in+2", "in+3", "out+1", "out+2", "out+3"])
def test_tile_vec_and_each_reason_that_loses_it(reason, tile, dev):
    """128 x 192 is VEC; each reason that loses the float4 form on its own (a batch stride alone cannot: see the module text)."""
    rows, cols, in_off, out_off = 128, 192, 0, 0
    if reason == "rows%4":
        rows = 130
    elif reason == "cols%4":
        cols = 190
    elif reason.startswith("in+"):
        in_off = int(reason[3:])
    elif reason.startswith("out+"):
        out_off = int(reason[4:])
    knobs = lf.Knobs(tile=tile)
    for batch in (1, 3):
        with state(dev, 1, knobs) as cus:
            transpose2d(dev, cus, knobs, batch, rows, cols, in_off, out_off, "TILE<%d,VEC=%d> order=0" % (tile, reason == "vec"), salt=2)


def test_tile_against_skinny_boundary(dev):
    """17 x 17 is the smallest tile transpose, 16 x 17 and 17 x 16 are skinny."""
    knobs = lf.Knobs()
    with state(dev, 0, knobs) as cus:
        transpose2d(dev, cus, knobs, 1, 17, 17, 0, 0, "TILE<64,VEC=0> order=0")
        transpose2d(dev, cus, knobs, 1, 16, 17, 0, 0, "SKINNY<TALL=0>")
        transpose2d(dev, cus, knobs, 1, 17, 16, 0, 0, "SKINNY<TALL=1>")


@pytest.mark.parametrize("rows,cols,in_off,path", [(257, 191, 0, "TILE<64,VEC=0> order=0"), (256, 192, 0, "TILE<64,VEC=1> order=0"),
                                                   (1031, 1033, 0, "TILE<64,VEC=0> order=0"), (4096, 4096, 0, "TILE<128,VEC=1> order=0"),
                                                   (4099, 4099, 0, "WALIGN<64> order=1"), (5000, 4099, 1, "WALIGN<128> order=1")])
def test_transposes_at_the_devices_own_cu_count(rows, cols, in_off, path, dev):
    """The CU rule as the device plans it (names for 256 CUs): 64-tiles below 1024 tiles of 128 — 1031 x 1033 among them, which
    never reaches the write-aligned kernel — 128-tiles from there, write-aligned 64-tiles below 1200 tiles, 128-tiles above."""
    knobs = lf.Knobs()
    with state(dev, 0, knobs) as cus:
        transpose2d(dev, cus, knobs, 1, rows, cols, in_off, 32, path, salt=1)


# ---- skinny and interleave ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("short", range(1, 17))
def test_skinny(short, dev):
    """Short side 1 .. 16 both ways, long sides around the workgroup's 256 lanes, batches of 1 and 2, at the device's own CU count;
    n = 1000 with 2 .. 4 rows stays below the interleave's 1024."""
    knobs = lf.Knobs()
    with state(dev, 0, knobs) as cus:
        for long_ in (1, 17, 255, 256, 257, 1000):
            for rows, cols in ((short, long_), (long_, short)):
                for batch in (1, 2):
                    transpose2d(dev, cus, knobs, batch, rows, cols, batch - 1, 3 - batch, "SKINNY<TALL=%d>" % (cols <= rows), salt=short % 8)


@pytest.mark.parametrize("to_interleaved", [True, False])
@pytest.mark.parametrize("R", [2, 3, 4])
def test_interleave(R, to_interleaved, dev):
    """Every tile boundary of the 2048-position tiles, ragged last tiles, batches of 1 and 3; and each condition that sends the same
    shape to the skinny kernel instead: n below 1024, n % 4 != 0, either pointer off 16 bytes."""
    knobs = lf.Knobs()
    name = "INTERLEAVE<R=%d,%s>" % (R, "to_interleaved" if to_interleaved else "to_planes")
    skinny = "SKINNY<TALL=%d>" % (not to_interleaved)
    shape = (lambda n: (R, n)) if to_interleaved else (lambda n: (n, R))
    with state(dev, 0, knobs) as cus:
        for n in (1024, 1028, 2044, 2048, 2052, 4100):
            for batch in (1, 3):
                transpose2d(dev, cus, knobs, batch, *shape(n), 0, 32, name, salt=R)
        for n, in_off, out_off in ((1020, 0, 0), (1026, 0, 0), (2049, 0, 0), (2048, 1, 0), (2048, 2, 0), (2048, 3, 0), (2048, 0, 1), (2048, 0, 2),
                                   (2048, 0, 3)):
            transpose2d(dev, cus, knobs, 1, *shape(n), in_off, out_off, skinny, salt=R)
    with state(dev, 0, lf.Knobs(tile=5)) as cus:
        transpose2d(dev, cus, lf.Knobs(tile=5), 2, *shape(2048), 0, 0, skinny, salt=R)


# ---- np_permute --------------------------------------------------------------------------------------------------------------

PERMUTE_CASES = [
    # identity after fusion; last_two with batch axes
    ("memcpy", 0, {}, (3, 1, 5, 7), (0, 2, 1, 3), 0, 0, "MEMCPY"),
    ("memcpy_ones", 0, {}, (1, 6, 1, 9), (2, 1, 0, 3), 1, 2, "MEMCPY"),
    ("last_two_batch_axes", 0, {}, (2, 3, 65, 70), (0, 1, 3, 2), 0, 0, "TILE<64,VEC=0> order=0"),
    ("last_two_skinny", 0, {}, (2, 3, 5, 70), (0, 1, 3, 2), 0, 0, "SKINNY<TALL=0>"),
    ("last_two_interleave", 0, {}, (2, 3, 32, 64), (0, 2, 3, 1), 0, 0, "INTERLEAVE<R=3,to_interleaved>"),
    # the pitched plane transposes: E = 1, A and B >= 64
    ("pitched_1_batch_axis", 0, {}, (70, 13, 66), (2, 1, 0), 0, 0, "TILE<64,VEC=0> order=0"),
    ("pitched_1_batch_axis_cu1_tile128", 1, {}, (70, 13, 66), (2, 1, 0), 0, 1, "TILE<128,VEC=0> order=0"),
    ("pitched_1_batch_axis_vec", 1, {}, (64, 5, 128), (2, 1, 0), 0, 0, "TILE<128,VEC=1> order=0"),
    ("pitched_2_batch_axes_tile", 1, {}, (2, 256, 2, 64), (2, 0, 3, 1), 0, 0, "TILE<128,VEC=1> order=0"),
    ("pitched_2_batch_axes_walign64", 1, {}, (2, 257, 2, 64), (2, 0, 3, 1), 0, 0, "WALIGN<64> order=1"),
    ("pitched_2_batch_axes_walign128", 1, {"walign64_below": 0}, (2, 259, 2, 64), (2, 0, 3, 1), 0, 32, "WALIGN<128> order=1"),
    ("pitched_walign128_order2", 1, {"walign64_below": 0, "walign_order": 2}, (3, 271, 2, 96), (2, 0, 3, 1), 1, 32, "WALIGN<128> order=2"),
    ("pitched_walign_refused_batch_stride", 1, {}, (2, 257, 2, 65), (2, 0, 3, 1), 0, 0, "TILE<128,VEC=0> order=0"),
    ("pitched_walign_refused_batch_axis_between", 1, {}, (257, 2, 64), (2, 1, 0), 0, 0, "TILE<128,VEC=0> order=0"),
    ("pitched_3_batch_axes", 1, {}, (2, 66, 2, 3, 65), (3, 2, 0, 4, 1), 0, 0, "TILE<128,VEC=0> order=0"),
    ("pitched_3_batch_axes_order1", 0, {"tile_order": 1}, (2, 66, 2, 3, 65), (3, 2, 0, 4, 1), 2, 3, "TILE<64,VEC=0> order=1"),
    ("pitched_6_batch_axes", 1, {}, (2, 64, 2, 2, 2, 2, 2, 64), (6, 5, 4, 3, 2, 0, 7, 1), 0, 0, "TILE<128,VEC=1> order=0"),
    # permute_plane_kernel<1>
    ("plane_small_a", 0, {}, (30, 7, 200), (2, 1, 0), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_small_b", 0, {}, (200, 7, 30), (2, 1, 0), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_short_a_long_b_run", 0, {}, (5, 3, 1000), (2, 1, 0), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_balanced_100x100_e2", 0, {}, (100, 3, 100, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_50_130", 0, {}, (50, 3, 130), (2, 1, 0), 1, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_e2", 0, {}, (33, 4, 65, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_e3", 0, {}, (129, 257, 3), (1, 0, 2), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_e5", 0, {}, (40, 2, 70, 5), (2, 1, 0, 3), 0, 3, "PLANE<W=1> xcd_runs=1"),
    ("plane_e7", 0, {}, (17, 3, 19, 7), (2, 1, 0, 3), 3, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_e31", 0, {}, (20, 2, 30, 31), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_6_batch_axes", 0, {}, (2, 10, 2, 3, 2, 2, 2, 12), (6, 5, 4, 3, 2, 0, 7, 1), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_xcd_runs0_tiles%8", 0, {"plane_order": 0}, (96, 2, 160, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=0"),
    ("plane_xcd_runs1_tiles%8", 0, {"plane_order": 1}, (96, 2, 160, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_xcd_runs1_tiles_odd", 0, {"plane_order": 1}, (100, 3, 100, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane_xcd_runs0_tiles_odd", 0, {"plane_order": 0}, (100, 3, 100, 2), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=0"),
    # permute_plane_kernel<4>, and the same shapes as W = 1
    ("plane4_e4", 0, {}, (3, 33, 65, 4), (0, 2, 1, 3), 0, 0, "PLANE<W=4> xcd_runs=0"),
    ("plane4_e8", 0, {}, (2, 40, 300, 8), (0, 2, 1, 3), 0, 0, "PLANE<W=4> xcd_runs=0"),
    ("plane4_e12", 0, {}, (5, 17, 19, 12), (2, 1, 0, 3), 0, 0, "PLANE<W=4> xcd_runs=0"),
    ("plane4_e28", 0, {}, (2, 50, 70, 28), (0, 2, 1, 3), 0, 0, "PLANE<W=4> xcd_runs=0"),
    ("plane4_e8_xcd_runs1", 0, {"plane_order": 1}, (2, 40, 300, 8), (0, 2, 1, 3), 0, 0, "PLANE<W=4> xcd_runs=1"),
    ("plane4_e4_in+1", 0, {}, (3, 33, 65, 4), (0, 2, 1, 3), 1, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e8_out+1", 0, {}, (2, 40, 300, 8), (0, 2, 1, 3), 0, 1, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e12_in+1", 0, {}, (5, 17, 19, 12), (2, 1, 0, 3), 1, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e12_in+2", 0, {}, (5, 17, 19, 12), (2, 1, 0, 3), 2, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e28_out+1", 0, {}, (2, 50, 70, 28), (0, 2, 1, 3), 0, 1, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e4_variant6", 0, {"tile": 6}, (3, 33, 65, 4), (0, 2, 1, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e8_variant6", 0, {"tile": 6}, (2, 40, 300, 8), (0, 2, 1, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e12_variant6", 0, {"tile": 6}, (5, 17, 19, 12), (2, 1, 0, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    ("plane4_e28_variant6", 0, {"tile": 6}, (2, 50, 70, 28), (0, 2, 1, 3), 0, 0, "PLANE<W=1> xcd_runs=1"),
    # the gather: a kept innermost axis of 32 floats and more, and the plane path switched off
    ("gather_w4", 0, {}, (9, 11, 32), (1, 0, 2), 0, 0, "GATHER<u32,W=4>"),
    ("gather_w4_unaligned_pointers", 0, {}, (9, 11, 36), (1, 0, 2), 1, 3, "GATHER<u32,W=4>"),
    ("gather_w1_inner%4", 0, {}, (9, 11, 33), (1, 0, 2), 0, 0, "GATHER<u32,W=1>"),
    ("gather_w1_inner34", 0, {}, (7, 5, 3, 34), (2, 0, 1, 3), 0, 0, "GATHER<u32,W=1>"),
    ("gather_w4_more_blocks_than_the_cap", 1, {}, (40, 41, 64), (1, 0, 2), 0, 0, "GATHER<u32,W=4>"),
    ("gather_variant3_reversal", 0, {"tile": 3}, (9, 10, 11, 12), (3, 2, 1, 0), 0, 0, "GATHER<u32,W=1>"),
    ("gather_variant4_short_inner", 0, {"tile": 4}, (6, 40, 30, 8), (0, 2, 1, 3), 0, 0, "GATHER<u32,W=1>"),
]


@pytest.mark.parametrize("case", PERMUTE_CASES, ids=[c[0] for c in PERMUTE_CASES])
def test_permute(case, dev):
    """np_permute: the fusion pass, the two shortcuts, the pitched plane transposes with one to six batch axes (tile and
    write-aligned), permute_plane_kernel<1 | 4> with its balanced tiles, both tile orders, and the gather."""
    name, cus_knob, kn, shape, perm, in_off, out_off, path = case
    knobs = lf.Knobs(**kn)
    with state(dev, cus_knob, knobs) as cus:
        if "tiles" in name:        # the XCD-run bijection with and without a remainder
            assert (lf.plan_permute(shape, perm, 0, 0, cus, knobs)[lf.GRID_X] % 8 == 0) == name.endswith("tiles%8")
        permute(dev, cus, knobs, tuple(shape), tuple(perm), in_off, out_off, path, salt=len(name) % 8)


def test_permute_every_permutation_of_four_axes(dev):
    """All 24 permutations of (6, 7, 8, 9) and of (5, 1, 36, 4): whatever the plan says ran, bits and frame hold."""
    import itertools
    knobs = lf.Knobs()
    with state(dev, 0, knobs) as cus:
        for shape in ((6, 7, 8, 9), (5, 1, 36, 4)):
            for perm in itertools.permutations(range(4)):
                path = lf.instantiation(lf.plan_permute(shape, perm, 0, 0, cus, knobs))
                permute(dev, cus, knobs, shape, perm, 0, 0, path, salt=4)


# ---- np_strided_copy and np_copy2d -------------------------------------------------------------------------------------------

STRIDED_CASES = [
    ("contiguous", (5, 6, 7), (42, 7, 1), 0, "MEMCPY"),
    ("contiguous_with_extent_1", (5, 1, 7), (7, 999, 1), 0, "MEMCPY"),
    ("every_second_column", (30, 50), (100, 2), 0, "GATHER<u32,W=1>"),
    ("negative_stride_axis0", (30, 50), (-50, 1), 29 * 50, "GATHER<u32,W=1>"),
    ("negative_stride_axis1", (30, 50), (50, -1), 49, "GATHER<u32,W=1>"),
    ("negative_stride_axis0_vec4", (30, 64), (-64, 1), 29 * 64, "GATHER<u32,W=4>"),
    ("broadcast_axis0", (30, 50), (0, 1), 0, "GATHER<u32,W=1>"),
    ("broadcast_axis1", (30, 50), (1, 0), 0, "GATHER<u32,W=1>"),
    ("broadcast_axis0_vec4", (30, 64), (0, 1), 0, "GATHER<u32,W=4>"),
    ("vec4_row_slab", (30, 64), (128, 1), 0, "GATHER<u32,W=4>"),
    ("vec4_lost_inner_stride", (30, 64), (128, 2), 0, "GATHER<u32,W=1>"),
    ("vec4_lost_inner%4", (30, 66), (128, 1), 0, "GATHER<u32,W=1>"),
    ("vec4_lost_inner_below_32", (30, 28), (128, 1), 0, "GATHER<u32,W=1>"),
    ("vec4_lost_outer_stride%4", (30, 64), (130, 1), 0, "GATHER<u32,W=1>"),
]


@pytest.mark.parametrize("case", STRIDED_CASES, ids=[c[0] for c in STRIDED_CASES])
def test_strided_copy(case, dev):
    """np_strided_copy: the memcpy shortcut, every second column, a negative stride on each axis, a stride-0 axis, the float4 gather
    and each condition that loses it alone; base pointers at offsets 0 and 1."""
    name, shape, strides, base, path = case
    span = base + sum((e - 1) * s for e, s in zip(shape, strides) if s > 0) + 1
    n = int(np.prod(shape))
    sh, st = (C.c_int * len(shape))(*shape), (C.c_longlong * len(shape))(*strides)
    with state(dev, 0) as cus:
        for in_off, out_off in ((0, 0), (1, 2)):
            buffer = lf.words(span, 6)
            launch(dev, "strided_copy %s %s base=%d in+%d out+%d" % (shape, strides, base, in_off, out_off), path, buffer, in_off,
                   lambda off: lf.expect_strided(buffer, base, shape, strides, off), n, out_off,
                   lambda a, b: dev.L.np_strided_copy(a + 4 * base, b, len(shape), sh, st),
                   lambda a, b: lf.plan_strided_copy(shape, strides, cus), 6)


@pytest.mark.parametrize("width,src_pitch,dst_pitch,path", [(64, 64, 64, "MEMCPY"), (64, 80, 64, "COPY2D<V=4>"), (64, 64, 67, "COPY2D<V=4>"),
                                                            (63, 80, 70, "COPY2D<V=1>"), (1, 3, 2, "COPY2D<V=1>"), (300, 301, 303, "COPY2D<V=4>")])
def test_copy2d(width, src_pitch, dst_pitch, path, dev):
    """np_copy2d: the unpitched memcpy, float4 units at any pitch and base, single floats; the gaps between the destination's rows
    keep their canaries."""
    rows = 37
    src = lf.words(rows * src_pitch, 7)
    with state(dev, 0) as cus:
        for in_off, out_off in ((0, 0), (3, 1)):
            def want_of(off):
                image = lf.blank_output(rows * dst_pitch, off)
                for r in range(rows):
                    image[off + r * dst_pitch:off + r * dst_pitch + width] = src[r * src_pitch:r * src_pitch + width]
                return image
            launch(dev, "copy2d width=%d pitches %d -> %d in+%d out+%d" % (width, src_pitch, dst_pitch, in_off, out_off), path, src, in_off,
                   want_of, rows * dst_pitch, out_off, lambda a, b: dev.L.np_copy2d(b, dst_pitch, a, src_pitch, width, rows),
                   lambda a, b: lf.plan_copy2d(dst_pitch, src_pitch, width, rows, cus), 7)


# ---- the probe itself, and NDArray -------------------------------------------------------------------------------------------

def test_probe_is_cleared_by_calls_that_move_nothing(dev):
    knobs = lf.Knobs()
    with state(dev, 0, knobs) as cus:
        transpose2d(dev, cus, knobs, 1, 20, 30, 0, 0, "TILE<64,VEC=0> order=0")
        assert dev.record() is not None
        _lib.check(dev.L.np_transpose2d(None, None, 0, 4, 4))
        assert dev.record() is None
        transpose2d(dev, cus, knobs, 1, 20, 30, 0, 0, "TILE<64,VEC=0> order=0")
        sh, pm = (C.c_int * 2)(0, 5), (C.c_int * 2)(1, 0)
        _lib.check(dev.L.np_permute(None, None, 2, sh, pm))
        assert dev.record() is None
    count = C.c_uint(7)
    assert dev.L.np_debug_layout_last_record(None, 1, C.byref(count)) != 0 and dev.L.np_debug_layout_last_record(None, 0, None) != 0
    assert dev.L.np_debug_layout_last_record(None, 0, C.byref(count)) == 0 and count.value == 0


@pytest.mark.parametrize("shape,axes,start", [((66, 65), None, 1), ((130, 192), None, 2), ((20, 1024), None, 17), ((9, 11, 32), (1, 0, 2), 3),
                                              ((34, 4, 65, 2), (2, 1, 0, 3), 1), ((71, 13, 66), (2, 1, 0), 1)])
def test_ndarray_transpose_of_a_row_sliced_view_and_of_a_pending_chain(shape, axes, start, dev):
    """NDArray.transpose of rows start .. of an array (a view: the base pointer sits start rows into the block) by bits, with the
    record the plan gives for that address; and of a pending chain (x * 1 under the lazy binding) against the chain computed eagerly."""
    from numpower_amd import ndarray as nd
    from numpower_amd.ndarray import NDArray
    n = int(np.prod(shape))
    x = lf.words(n, 5).reshape(shape)
    g = NDArray.array(x.view(np.float32)).gpu()
    view = g.slice([start, shape[0]])
    vshape = (shape[0] - start,) + tuple(shape[1:])
    perm = tuple(axes) if axes is not None else tuple(reversed(range(len(shape))))
    got = NDArray.transpose(view, axes)
    rec = dev.record()
    plan = lf.plan_permute(vshape, perm, 4 * start * (n // shape[0]), 0, dev.cus)
    print("LAYOUT-RECORD NDArray.transpose %s %s rows %d.. | %s" % (shape, perm, start, lf.describe(rec)))
    want = np.ascontiguousarray(np.transpose(x[start:], perm))
    out = got.cpu().numpy()
    assert out.shape == want.shape and (out.view(np.uint32) == want).all()
    assert rec == plan, "the probe says %s, the plan %s" % (lf.describe(rec), lf.describe(plan))
    eager = (view * 1.0).cpu().numpy().view(np.uint32)
    was = nd._LAZY_BINDING
    NDArray.set_lazy_binding(True)
    try:
        lazy = NDArray.transpose(view * 1.0, axes).cpu().numpy().view(np.uint32)
    finally:
        NDArray.set_lazy_binding(was)
    assert (lazy == np.ascontiguousarray(np.transpose(eager, perm))).all()
