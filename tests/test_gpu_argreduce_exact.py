"""np_argreduce.hip against the exact family (tests/argreduce_family.py), through the C ABI.  Every launch of this module

  * reads its operand at float offset 0, 1, 2 or 3 (the wide-inner cases also 32 and 33) of a larger allocation whose frame WOULD
    WIN IF READ: +Inf all round for argmax, NaN for argmin — a kernel that looks one element in front of a0 or behind a1 answers
    with an index that is wrong or out of range;
  * writes into an output inside a frame of canaries, and the WHOLE allocation is compared: every index with == against the
    family's closed form, every canary against itself;
  * asserts the whole record of np_debug_argreduce_last_record against the planner restated on the host (plan(), at the operand's
    actual address), and that the planned kernel is the one the case was written for: where it is not, the case FAILS.

The planner divides by the CU count: np_debug_set_cus (and the np_reduce_set_variant knobs 4000000 + N, 4100000 + N, 4200001)
inside state(), which puts everything back on every way out, bring every branch down to a few thousand elements.  CASES lists
them per kernel; tests/test_argreduce_reference_cpu.py walks the same list without a device and shows that every kernel, every L,
both FINAL values, every fold and every COLS is reached.  Where np_argreduce's own rules set a floor the case is as small as they
allow: argreduce_rows_group wants 1024 rows, argreduce_rows_wave at 32768 elements 16 of them, a ninth chunk of
argreduce_cols_tile 576 rows of 192 columns or more (chunks <= axis_len / 64), argreduce_fold_cols_kernel<16> and <64> 64
workgroups of columns, argreduce_fold_block_kernel 65 chunks of 4096 elements.

Each case prints `ARG-RECORD <case> | <record>` (pytest -s): tools/argreduce_exact_log.py makes profiles/argreduce/exact_tests.log
from that output."""
import collections
import contextlib
import ctypes as C

import numpy as np
import pytest

from numpower_amd import _lib
from tests import argreduce_family as af

pytestmark = pytest.mark.gpu

FRONT, TAIL = 32, 64          # frame floats in front of offset 0 (128 bytes: the offset alone decides the alignment) and behind
OUT_FRONT, OUT_TAIL = 32, 64
CANARY = np.float32(-7777.0)  # no index is negative
ALL_FAMILIES = ("winner_finite", "winner_identity", "ties", "ties_identity", "constants", "permutation", "nan_rules")
LIGHT = ("winner_finite", "ties_identity", "constants", "permutation", "nan_rules")     # the cases of a megabyte and more
NARROW, WIDE = (0, 1, 2, 3), (0, 1, 2, 3, 32, 33)

Case = collections.namedtuple("Case", "path outer n inner cus knobs offsets families", defaults=(1, af.Knobs(), NARROW, ALL_FAMILIES))
K = af.Knobs


def _group(n, outer=1027):
    L = 1
    while L * 8 < n:
        L *= 2
    return Case("ROWS_GROUP<L=%d>" % L, outer, n, 1, families=ALL_FAMILIES if n <= 64 else LIGHT)


CASES = {
    # L = 1 .. 32 on both sides of each step; 1027 rows: no multiple of 256 / L; 1024 reaches it, 1023 does not
    "rows_group": [_group(n) for n in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)] + [
        _group(10, 1024), Case("ROWS_WAVE", 1023, 10, 1), Case("ROWS_GROUP<L=2>", 2048, 10, 1, cus=0),
        Case("ROWS_GROUP<L=32>", 1024, 129, 1, cus=0, families=LIGHT), Case("ROWS_GROUP<L=1>", 1500, 7, 1, cus=0)],
    # 16 .. 19 rows: the last workgroup holds 4, 1, 2, 3 of them; an odd length rotates the head row by row; nvec = 64, 128, 192
    # (one to three vectors per lane without the main loop), 320 / 384 / 448 (five to seven: the remainder behind it), 8192
    "rows_wave": [Case("ROWS_WAVE", 16 + i % 4, n, 1) for i, n in enumerate((1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 515, 770, 1023, 1024, 1025,
                                                                               1283, 1537, 1795))] + [
        Case("ROWS_WAVE", 16, 257, 1), Case("ROWS_WAVE", 19, 257, 1), Case("ROWS+FOLD_THREAD", 15, 257, 1),
        Case("ROWS_WAVE", 16, 32768, 1, families=LIGHT), Case("ROWS_WAVE", 4096, 257, 1, cus=0, families=("permutation", "nan_rules")),
        Case("ROWS_WAVE", 4100, 300, 1, cus=0, offsets=(1, 2), families=("permutation", "nan_rules", "constants")),
        Case("ROWS+FOLD_THREAD", 4095, 257, 1, cus=0, offsets=(3,), families=("permutation", "nan_rules"))],
    # one CU: 9 workgroups wanted: 9, 5, 3, 2 chunks and 1 (outer >= 9); at most one chunk per 4096 elements.  32769 is odd: the
    # head rotates row by row, so two rows at offsets 0 and 2, three at 0 and 3 and five or more at any offset meet all four heads
    "rows": [Case("ROWS+FOLD_THREAD", 1, 32769, 1)] + [Case("ROWS+FOLD_THREAD", outer, 32769, 1, offsets=offs, families=LIGHT)
                                                       for outer, offs in ((2, (0, 2)), (3, (0, 3)), (5, (1,)), (9, (2,)), (15, (3,)))] + [
        Case("ROWS+FOLD_THREAD", 1, n, 1) for n in (4096, 4097, 8193)] + [
        Case("ROWS+FOLD_BLOCK", 1, 262145, 1, cus=8, offsets=(0, 3), families=LIGHT), Case("ROWS+FOLD_THREAD", 3, 8193, 1, cus=0),
        Case("ROWS+FOLD_THREAD", 1, 8193, 1, cus=0), Case("ROWS+FOLD_BLOCK", 1, 262145, 1, cus=0, offsets=(1, 2), families=LIGHT)],
    # axis_len . inner = 4095 stays out, 4096 is in; one slab, two slabs (outer 1: two workgroups per CU), three (outer 3: eight),
    # five and seven by the knob; slabs of cnt % 4 = 1, 2, 3 elements; last slabs of 1, 2 and 3 rows: a slab holds 4096 elements or
    # more and its rows are rounded up to a multiple of 4, so with at most 63 columns 17 slabs of 72 rows in front of it are the fewest
    "small_inner": [Case("CHUNKS+FOLD_THREAD", 1, 1365, 3), Case("GENERIC", 1, 65, 63), Case("SMALL_INNER+FOLD_THREAD", 1, 2048, 2),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1366, 3), Case("SMALL_INNER+FOLD_THREAD", 1, 2733, 3),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1643, 5), Case("SMALL_INNER+FOLD_THREAD", 3, 1762, 7),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 131, 63), Case("SMALL_INNER+FOLD_THREAD", 3, 197, 63),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 6834, 3, knobs=K(flat_wg_per_cu=5)),
                    Case("SMALL_INNER+FOLD_THREAD", 2, 4102, 7, knobs=K(flat_wg_per_cu=14)),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1225, 63, knobs=K(flat_wg_per_cu=18), offsets=(0, 1), families=LIGHT),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1226, 63, knobs=K(flat_wg_per_cu=18), offsets=(2,), families=LIGHT),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1227, 63, knobs=K(flat_wg_per_cu=18), offsets=(3,), families=LIGHT),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 1366, 3, cus=0), Case("SMALL_INNER+FOLD_THREAD", 3, 1762, 7, cus=0),
                    Case("SMALL_INNER+FOLD_THREAD", 1, 2733, 3, cus=0, offsets=(1, 2))],
    # whole float4 column groups: T = 256 lanes (inner 4, 8, 64, 256) and fewer (inner4 = 3, 25, 63); 260 columns go to the tiles;
    # last slabs of 1, 2 and 3 rows: 256 columns in five slabs of 20 rows (the last holds nvec = 64, 128, 192 < T vectors: lanes that
    # meet nothing, a slab shorter than one trip), 64 columns in 18 slabs of 68
    "small_inner4": [Case("SMALL_INNER4+FOLD_THREAD", 1, 1024, 4), Case("CHUNKS+FOLD_THREAD", 1, 1023, 4), Case("SMALL_INNER4+FOLD_THREAD", 1, 1025, 8),
                     Case("SMALL_INNER4+FOLD_THREAD", 3, 1030, 12), Case("SMALL_INNER4+FOLD_THREAD", 1, 685, 12),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 64, 64), Case("SMALL_INNER4+FOLD_THREAD", 1, 129, 64),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 85, 100), Case("SMALL_INNER4+FOLD_THREAD", 3, 126, 100),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 37, 252), Case("SMALL_INNER4+FOLD_THREAD", 1, 16, 256),
                     Case("SMALL_INNER4+FOLD_THREAD", 2, 67, 256), Case("SMALL_INNER4+FOLD_THREAD", 1, 22, 192),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 4103, 4, knobs=K(flat_wg_per_cu=4)),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 81, 256, knobs=K(flat_wg_per_cu=5)), Case("SMALL_INNER4+FOLD_THREAD", 1, 82, 256, knobs=K(flat_wg_per_cu=5)),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 83, 256, knobs=K(flat_wg_per_cu=5)),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 1157, 64, knobs=K(flat_wg_per_cu=18), offsets=(0, 3)),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 1158, 64, knobs=K(flat_wg_per_cu=18), offsets=(1, 2)),
                     Case("COLS_TILE<FINAL=1>", 1, 16, 260, offsets=WIDE), Case("SMALL_INNER4+FOLD_THREAD", 2, 600, 8, cus=0),
                     Case("SMALL_INNER4+FOLD_THREAD", 1, 129, 64, cus=0), Case("SMALL_INNER4+FOLD_THREAD", 3, 1030, 12, cus=0, offsets=(0, 3))],
    # ncol = 1, 2, 3 in the last lane (193, 194, 195; 257; 513), one, two and three tiles; 15 rows stay out; 16 .. 48 rows: the
    # single-row loop alone, the 4-row loop, the 8-row loop, with wave 3 (and 2) empty or not; partials in 2, 3, 5 and 8 chunks
    # (chunk_len 65, 65, 27, 17: odd); 9 chunks through the column fold with COLS = 4, 16, 64; rows_aligned (260 and 512 columns at
    # offset 0) and not; xcd_runs with 2 . 2 . 2 = 8, 3 and 2 . 3 . 3 = 18 workgroups, and switched off
    "cols_tile": [Case("GENERIC", 1, 15, 193, offsets=WIDE)] + [
        Case("COLS_TILE<FINAL=1>", 1, n, inner, offsets=WIDE) for n, inner in ((16, 193), (17, 194), (18, 195), (19, 192), (20, 257), (21, 260), (29, 513),
                                                                                 (32, 193), (33, 260), (45, 194), (47, 257), (48, 513), (16, 512))] + [
        Case("COLS_TILE<FINAL=1>", 3, 23, 195, offsets=WIDE), Case("COLS_TILE<FINAL=1>", 2, 40, 257, offsets=WIDE, knobs=K(xcd_runs_off=1)),
        Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 128, 193, offsets=WIDE, families=LIGHT), Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 193, 195, offsets=WIDE, families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 2, 129, 257, offsets=WIDE, families=LIGHT), Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 130, 260, offsets=WIDE, knobs=K(cols_wg_per_cu=5), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 3, 200, 513, offsets=(1, 32), knobs=K(cols_wg_per_cu=27)),
        Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 320, 194, offsets=(0, 3), knobs=K(cols_wg_per_cu=5)),
        Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 513, 193, offsets=(0, 1), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<4>", 1, 577, 193, cus=2, offsets=(0, 2), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<4>", 1, 576, 512, cus=9, offsets=(0, 33), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<16>", 5, 576, 193, cus=6, offsets=(1,), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<64>", 16, 579, 193, cus=18, offsets=(3,), families=LIGHT),
        Case("COLS_TILE<FINAL=1>", 1, 40, 513, cus=0, offsets=(0, 33)), Case("COLS_TILE<FINAL=0>+FOLD_THREAD", 1, 128, 193, cus=0, offsets=(0, 1)),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<4>", 1, 577, 193, cus=0, offsets=(1, 32), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<16>", 5, 576, 193, cus=0, offsets=(2,), families=LIGHT),
        Case("COLS_TILE<FINAL=0>+FOLD_COLS<64>", 16, 579, 193, cus=0, offsets=(0,), families=LIGHT)],
    # 127 rows stay out; chunks of 32, 33, 34, 35 rows (129: the last one holds 30); inner 65 .. 191, and a few columns below 4096 elements
    "chunks": [Case("GENERIC", 1, 127, 65)] + [Case("CHUNKS+FOLD_THREAD", 1, n, inner) for n, inner in ((128, 65), (129, 191), (136, 67), (140, 101),
                                                                                                         (131, 3), (1365, 3), (700, 5))] + [
        Case("CHUNKS+FOLD_THREAD", 3, 133, 66), Case("CHUNKS+FOLD_THREAD", 1, 128, 65, cus=0),
        Case("CHUNKS+FOLD_THREAD", 3, 133, 66, cus=0), Case("CHUNKS+FOLD_THREAD", 1, 700, 5, cus=0, offsets=(0, 1))],
    # a thread per output: axes of 1 .. 9; 4550 outputs on the 4096 threads of one CU's grid
    "generic": [Case("GENERIC", 3, n, 7) for n in range(1, 10)] + [Case("GENERIC", 70, 3, 65), Case("GENERIC", 3, 5, 7, cus=0), Case("GENERIC", 70, 3, 65, cus=0),
                                                                Case("GENERIC", 1, 127, 65, cus=0)],
}


class Dev:
    def __init__(self):
        self.L = _lib.load()
        cus = C.c_int()
        _lib.check(self.L.np_debug_cus(C.byref(cus)))
        self.cus = cus.value

    def upload(self, buf, image):
        _lib.check(self.L.np_memcpy_h2d(buf.ptr, image.ctypes.data, image.nbytes))

    def download(self, buf, count):
        out = np.empty(count, np.float32)
        _lib.check(self.L.np_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes))
        return out

    def record(self):
        words, count = (C.c_uint * af.RECORD_WORDS)(*([0xEEEEEEEE] * af.RECORD_WORDS)), C.c_uint(99)
        _lib.check(self.L.np_debug_argreduce_last_record(words, 1, C.byref(count)))
        assert count.value <= 1, "np_debug_argreduce_last_record: %d records for one call" % count.value
        return tuple(words) if count.value else None


@pytest.fixture(scope="module")
def dev(hip):
    return Dev()


@contextlib.contextmanager
def state(dev, cus=0, knobs=af.Knobs()):
    """The CU count the planner assumes (0 = the device's own) and the argmax / argmin knobs, put back on every way out."""
    try:
        _lib.check(dev.L.np_debug_set_cus(cus))
        for code in af.codes(knobs):
            _lib.check(dev.L.np_reduce_set_variant(code))
        yield cus if cus else dev.cus
    finally:
        dev.L.np_debug_set_cus(0)
        for code in af.DEFAULT_CODES:
            dev.L.np_reduce_set_variant(code)


def launch(dev, what, bin_, bout, off, is_max, x, want, want_rec):
    """One np_argreduce call on x (outer, n, inner) at float offset `off` of its frame; the whole output allocation and the whole
    record are compared."""
    outer, n, inner = x.shape
    outputs = outer * inner
    image = np.full(FRONT + off + x.size + TAIL, np.inf if is_max else np.nan, np.float32)
    image[FRONT + off:FRONT + off + x.size] = x.reshape(-1)
    blank = np.full(OUT_FRONT + outputs + OUT_TAIL, CANARY, np.float32)
    dev.upload(bin_, image)
    dev.upload(bout, blank)
    _lib.check(dev.L.np_argreduce(1 if is_max else 0, bin_.ptr + 4 * (FRONT + off), outer, n, inner, bout.ptr + 4 * OUT_FRONT))
    got_rec = dev.record()
    got = dev.download(bout, blank.size)
    assert got_rec == want_rec, "%s: the probe says %s, the plan %s" % (what, af.describe(got_rec), af.describe(want_rec))
    blank[OUT_FRONT:OUT_FRONT + outputs] = want
    bad = np.flatnonzero(~(got == blank))
    if bad.size:
        triples = ["(%s, %r, %r)" % ("output %d" % (i - OUT_FRONT) if OUT_FRONT <= i < OUT_FRONT + outputs else "canary word %d" % i,
                                     float(got[i]), float(blank[i])) for i in bad[:6]]
        raise AssertionError("%s [%s]: %d of %d words differ; (where, got, want): %s" % (what, af.describe(got_rec), bad.size, blank.size, ", ".join(triples)))


def run_case(dev, name, case):
    """Every family of the case at every offset, argmax and argmin."""
    outer, n, inner = case.outer, case.n, case.inner
    size = outer * n * inner
    bin_ = _lib.DeviceBuffer(4 * (FRONT + max(case.offsets) + size + TAIL))
    bout = _lib.DeviceBuffer(4 * (OUT_FRONT + outer * inner + OUT_TAIL))
    assert bin_.ptr % 128 == 0 and bout.ptr % 128 == 0
    launches = 0
    try:
        with state(dev, case.cus, case.knobs) as cus:
            for off in case.offsets:
                addr = bin_.ptr + 4 * (FRONT + off)
                rec = af.plan(outer, n, inner, addr, cus, case.knobs)
                assert af.instantiation(rec) == case.path, "%s was written for %s; the plan shows %s" % (name, case.path, af.describe(rec))
                for is_max in (True, False):
                    for fam in case.families:
                        for label, x, want in af.FAMILIES[fam](rec, outer, n, inner, addr, is_max):
                            what = "%s (%d, %d, %d) cus=%d %s in+%d %s %s" % (name, outer, n, inner, cus, af.codes(case.knobs), off,
                                                                            "argmax" if is_max else "argmin", label)
                            launch(dev, what, bin_, bout, off, is_max, x, want, rec)
                            launches += 1
                print("ARG-RECORD %s (%d, %d, %d) cus=%d in+%d | %s" % (name, outer, n, inner, cus, off, af.describe(rec)))
    finally:
        bin_.free()
        bout.free()
    print("ARG-LAUNCHES %s | %d" % (name, launches))


def _ids(kernel):
    return ["%s-%dx%dx%d-cus%d%s" % (c.path, c.outer, c.n, c.inner, c.cus, "" if c.knobs == af.Knobs() else "-knobs%d.%d.%d" % c.knobs)
            for c in CASES[kernel]]


@pytest.mark.parametrize("case", CASES["rows_group"], ids=_ids("rows_group"))
def test_rows_group(case, dev):
    run_case(dev, "rows_group", case)


@pytest.mark.parametrize("case", CASES["rows_wave"], ids=_ids("rows_wave"))
def test_rows_wave(case, dev):
    run_case(dev, "rows_wave", case)


@pytest.mark.parametrize("case", CASES["rows"], ids=_ids("rows"))
def test_rows_and_the_folds(case, dev):
    run_case(dev, "rows", case)


@pytest.mark.parametrize("case", CASES["small_inner"], ids=_ids("small_inner"))
def test_small_inner(case, dev):
    run_case(dev, "small_inner", case)


@pytest.mark.parametrize("case", CASES["small_inner4"], ids=_ids("small_inner4"))
def test_small_inner4(case, dev):
    run_case(dev, "small_inner4", case)


@pytest.mark.parametrize("case", CASES["cols_tile"], ids=_ids("cols_tile"))
def test_cols_tile(case, dev):
    run_case(dev, "cols_tile", case)


@pytest.mark.parametrize("case", CASES["chunks"], ids=_ids("chunks"))
def test_chunks(case, dev):
    run_case(dev, "chunks", case)


@pytest.mark.parametrize("case", CASES["generic"], ids=_ids("generic"))
def test_generic(case, dev):
    run_case(dev, "generic", case)


# ---- determinism, the probe itself, and NDArray ------------------------------------------------------------------------------

REPEATED = [CASES["rows_group"][3], CASES["rows_wave"][12], CASES["rows"][0], CASES["small_inner"][4], CASES["small_inner4"][3],
            CASES["cols_tile"][17], CASES["cols_tile"][24], CASES["chunks"][2], CASES["generic"][9]]


@pytest.mark.parametrize("case", REPEATED, ids=[c.path + "-%dx%dx%d" % (c.outer, c.n, c.inner) for c in REPEATED])
def test_three_runs_give_identical_bits(case, dev):
    outer, n, inner = case.outer, case.n, case.inner
    bin_ = _lib.DeviceBuffer(4 * (FRONT + 1 + outer * n * inner + TAIL))
    bout = _lib.DeviceBuffer(4 * (OUT_FRONT + outer * inner + OUT_TAIL))
    try:
        with state(dev, case.cus, case.knobs) as cus:
            addr = bin_.ptr + 4 * (FRONT + 1)
            rec = af.plan(outer, n, inner, addr, cus, case.knobs)
            for is_max in (True, False):
                (label, x, want), = af.ties(rec, outer, n, inner, addr, is_max)[:1]
                image = np.full(FRONT + 1 + x.size + TAIL, np.inf if is_max else np.nan, np.float32)
                image[FRONT + 1:FRONT + 1 + x.size] = x.reshape(-1)
                dev.upload(bin_, image)
                runs = []
                for _ in range(3):
                    dev.upload(bout, np.full(OUT_FRONT + outer * inner + OUT_TAIL, CANARY, np.float32))
                    _lib.check(dev.L.np_argreduce(1 if is_max else 0, addr, outer, n, inner, bout.ptr + 4 * OUT_FRONT))
                    assert dev.record() == rec
                    runs.append(dev.download(bout, OUT_FRONT + outer * inner + OUT_TAIL).view(np.uint32))
                assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all()
                assert (runs[0][OUT_FRONT:OUT_FRONT + outer * inner].view(np.float32) == want).all()
    finally:
        bin_.free()
        bout.free()


def test_probe_is_cleared_by_calls_that_launch_nothing(dev):
    case = CASES["generic"][4]
    run_case(dev, "probe", case)
    assert dev.record() is not None
    _lib.check(dev.L.np_argreduce(1, None, 0, 4, 4, None))
    assert dev.record() is None
    run_case(dev, "probe", case)
    _lib.check(dev.L.np_argreduce(0, None, 3, 4, 0, None))
    assert dev.record() is None
    run_case(dev, "probe", case)
    assert dev.L.np_argreduce(1, None, 3, 0, 4, None) != 0 and dev.record() is None          # an empty axis is refused
    run_case(dev, "probe", case)
    assert dev.L.np_argreduce(1, None, 3, 4, 4, None) != 0 and dev.record() is None          # null pointers are refused
    count = C.c_uint(7)
    assert dev.L.np_debug_argreduce_last_record(None, 1, C.byref(count)) != 0 and dev.L.np_debug_argreduce_last_record(None, 0, None) != 0
    assert dev.L.np_debug_argreduce_last_record(None, 0, C.byref(count)) == 0 and count.value == 0


NDARRAY_SHAPES = [((7, 300, 1), "rows"), ((1030, 9), "group / small inner"), ((3, 40, 260), "tiles"), ((2, 1400, 3), "flat walk"),
                  ((2, 130, 67), "chunks"), ((3, 5, 7), "generic")]


@pytest.mark.parametrize("shape,what", NDARRAY_SHAPES, ids=[w for _, w in NDARRAY_SHAPES])
def test_ndarray_argmax_argmin(shape, what, dev):
    """NDArray.argmax / argmin: axis None, each axis, keepdims, a row-sliced view (the base pointer sits inside the block) and a
    pending chain (x * 1 under the lazy binding), each against expected(); the record of the last call against the plan."""
    from numpower_amd import ndarray as nd
    from numpower_amd.ndarray import NDArray
    rng = np.random.default_rng(7)
    x = rng.permutation(int(np.prod(shape))).astype(np.float32).reshape(shape) - 1000.0
    x.reshape(-1)[5::97] = np.nan
    x[1, 0] = np.nan                                          # position 0 of axis 1
    g = NDArray.array(x).gpu()

    def host(r):
        return np.float32(r) if isinstance(r, float) else r.cpu().numpy()

    for is_max, fn in ((True, NDArray.argmax), (False, NDArray.argmin)):
        assert host(fn(g)) == af.expected(x, None, is_max)
        for axis in range(len(shape)):
            got, want = host(fn(g, axis)), af.expected(x, axis, is_max)
            assert got.shape == want.shape and (got == want).all(), (shape, axis, is_max)
            outer, inner = int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
            rec = dev.record()
            assert rec is not None and rec[af.KERNEL] == af.plan(outer, shape[axis], inner, 0, dev.cus)[af.KERNEL]
        kd = fn(g, 1, True)
        assert kd.shape() == [shape[0], 1] + list(shape[2:]) and (kd.cpu().numpy().reshape(-1) == af.expected(x, 1, is_max).reshape(-1)).all()
        view = g.slice([1, shape[0]])
        for axis in (None, 0, len(shape) - 1):
            got, want = host(fn(view) if axis is None else fn(view, axis)), af.expected(x[1:], axis, is_max)
            assert np.shape(got) == want.shape and (got == want).all(), (shape, "view", axis, is_max)
        was = nd._LAZY_BINDING
        NDArray.set_lazy_binding(True)
        try:
            lazy = host(fn(view * 1.0, len(shape) - 1))
        finally:
            NDArray.set_lazy_binding(was)
        assert (lazy == af.expected(x[1:], len(shape) - 1, is_max)).all()
