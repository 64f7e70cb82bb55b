"""CPU-tier checks of the argmax / argmin family (tests/argreduce_family.py) and of the probe's boundary: expected() is the oracle's
float_argmax / float_argmin on every family and on random data with NaNs, and numpy's argmax / argmin where there is no NaN; about
50 plans are pinned by hand, so a typo in the restated planner cannot agree with itself; the header's NP_ARG_* constants are the
family's and the probe stays out of np_hip.h; the probe answers without a device; the cases of the GPU module are walked with the
device taken out: every case reaches the kernel it names and every kernel, L, FINAL, fold and COLS is reached by one."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import argreduce_family as af

ROOT = Path(__file__).resolve().parent.parent
A = 0x7F0000000000            # an address on the 128-byte grid


def _rec(kernel, targ, grid, chunks, chunk_len, xcd_runs=0, fold=0, cols=0, fold_grid=(0, 0, 0)):
    return tuple([kernel, targ] + list(grid) + [chunks, chunk_len, xcd_runs, fold, cols] + list(fold_grid) + [0, 0, 0])


def test_expected_is_the_oracle_on_random_data_with_nans(oracle):
    rng = np.random.default_rng(3)
    for shape in ((1,), (7,), (2, 3), (5, 1, 4), (3, 17, 5), (4, 9, 1), (64, 33)):
        for trial in range(6):
            x = rng.integers(-3, 4, size=shape).astype(np.float32)           # many ties
            x[rng.random(shape) < (0.0, 0.05, 0.3, 0.3, 0.9, 1.0)[trial]] = np.nan
            x[rng.random(shape) < 0.1] = np.inf
            x[rng.random(shape) < 0.1] = -np.inf
            x[rng.random(shape) < 0.1] = -0.0
            for is_max in (True, False):
                for axis in [None] + list(range(len(shape))):
                    got, want = af.expected(x, axis, is_max), oracle.argreduce(x, axis, is_max)
                    assert got.dtype == np.float32 and got.shape == want.shape and (got == want).all(), (shape, trial, axis, is_max)
                    if trial == 0:
                        assert (got == (np.argmax(x, axis) if is_max else np.argmin(x, axis))).all()


def test_expected_rules_by_hand():
    nan, inf = np.nan, np.inf
    rows = np.array([[nan, 1, inf, 2], [1, nan, 5, 5], [1, 5, nan, nan], [-inf, nan, -inf, nan], [-0.0, 0.0, -0.0, 0.0], [nan, nan, nan, nan],
                     [2, 7, 7, -3], [-3, 2, -3, 7]], np.float32)
    assert af.expected(rows, 1, True).tolist() == [0, 2, 1, 0, 0, 0, 1, 3]
    assert af.expected(rows, 1, False).tolist() == [0, 1, 2, 1, 0, 0, 3, 0]
    assert af.expected(rows[6], None, True) == 1 and af.expected(rows[6], None, True).shape == ()
    assert af.expected(rows.reshape(2, 4, 4), 1, False).shape == (2, 4)


CPU_SHAPES = [(af.ROWS_GROUP, 40, 10, 1), (af.ROWS_WAVE, 5, 131, 1), (af.ROWS, 2, 9000, 1), (af.SMALL_INNER, 2, 1500, 3), (af.SMALL_INNER4, 1, 600, 8),
              (af.COLS_TILE, 2, 140, 197), (af.CHUNKS_KERNEL, 1, 130, 67), (af.GENERIC, 3, 5, 7), (af.GENERIC, 2, 1, 3), (af.GENERIC, 2, 2, 3)]


@pytest.mark.parametrize("kernel,outer,n,inner", CPU_SHAPES)
def test_families_are_the_oracle_and_meet_their_points(kernel, outer, n, inner, oracle):
    """Every family on a shape per kernel (the record handed in, so the points are that kernel's): want is the oracle's answer, the
    winners of winner_at cover every point, ties really tie, nan_rules holds all nine patterns."""
    rec = list(af.plan(outer, n, inner, A + 4, 1))
    rec[af.KERNEL] = kernel
    if kernel in (af.ROWS, af.SMALL_INNER, af.SMALL_INNER4, af.COLS_TILE, af.CHUNKS_KERNEL):
        piece = -(-n // 3)
        rec[af.CHUNKS], rec[af.CHUNK_LEN] = 3, (piece + 3) // 4 * 4 if kernel in (af.SMALL_INNER, af.SMALL_INNER4) else piece
        assert rec[af.CHUNK_LEN] > 0 and 2 * rec[af.CHUNK_LEN] < n <= 3 * rec[af.CHUNK_LEN]
    pts = af.points(rec, outer, n, inner, A + 4)
    if kernel in (af.ROWS, af.SMALL_INNER, af.SMALL_INNER4, af.COLS_TILE, af.CHUNKS_KERNEL) and kernel != af.ROWS:
        # both sides of both piece boundaries are among the points
        assert {rec[af.CHUNK_LEN] - 1, rec[af.CHUNK_LEN], 2 * rec[af.CHUNK_LEN] - 1, 2 * rec[af.CHUNK_LEN]} <= {a for _, a in pts}
    if kernel in (af.SMALL_INNER, af.SMALL_INNER4):
        assert any(slots is not None and rec[af.CHUNK_LEN] < a < 2 * rec[af.CHUNK_LEN] - 1 for slots, a in pts)     # seams inside the middle slab
    for is_max in (True, False):
        met = set()
        for name, fam in af.FAMILIES.items():
            launches = fam(rec, outer, n, inner, A + 4, is_max)
            assert launches, name
            for label, x, want in launches:
                assert x.shape == (outer, n, inner) and x.dtype == np.float32 and want.shape == (outer * inner,)
                assert (want == oracle.argreduce(x, 1, is_max).reshape(-1)).all(), (label, is_max)
                if name == "winner_finite":
                    met.update((m, int(a)) for m, a in enumerate(want))
                    assert n == 1 or (np.sort(x, axis=1)[:, -2 if is_max else 1, :] == 3.0).all()        # one winner per output
                if name in ("ties", "ties_identity") and n > 2:
                    best = x.max(axis=1) if is_max else x.min(axis=1)
                    count = (x == best[:, None, :]).sum(axis=1)
                    assert (count >= 2).all() and (count <= 3).all() and (count == 3).any() == (outer * inner > 1)
                if name == "nan_rules" and outer * inner >= 9 and n >= 4:
                    nans = np.isnan(x).sum(axis=1).reshape(-1)
                    assert (nans[6::9] == n).all() and (nans[0::9] == 1).all() and (nans[4::9] >= 1).all()
                    bits = x.view(np.uint32)
                    assert (bits == af.QNAN_NEG).any() and (bits == af.SNAN).any() and (bits == af.QNAN_PAYLOAD).any()
        for slots, a in pts:
            if 0 <= a < n:
                assert any((m, a) in met for m in (slots if slots is not None else range(outer * inner))), (slots, a)


def test_points_name_the_seams():
    # arg_scan_contig on 1030 elements one float behind a 16-byte boundary: head 3, 256 vectors, 3 tail elements; lane 63's
    # accumulators 0 .. 3 own vectors 63, 127, 191, 255 (one trip each: the last is also the first)
    p = af.scan_positions(1030, 3, 64, (0, 63))
    assert af.head_of(A + 4, 1030) == 3 and af.head_of(A, 5) == 0 and af.head_of(A + 12, 1) == 1 and af.head_of(A + 8, 1) == 1
    for a in (0, 1, 2, 3, 6, 3 + 4 * 63, 3 + 4 * 63 + 3, 3 + 4 * 255, 3 + 4 * 255 + 3, 1027, 1028, 1029, 3 + 4 * 64, 3 + 4 * 192 + 3):
        assert a in p, a
    assert len(p) < 60
    # two trips per accumulator and a remainder: 4 * 64 * 2 + 70 vectors
    p = af.scan_positions(4 * 582, 0, 64, (0, 63))
    assert {0, 4 * 256, 4 * 512, 4 * (512 + 64) - 4 * 64 + 0, 4 * 63, 4 * (256 + 63), 4 * 575 + 3} <= set(p)
    # the tile kernel: a chunk of rows 65 .. 129: wave 1 starts at 66, its 8-row loop covers 66 .. 94 and 98 .. 126, nothing left
    r = af._tile_rows(65, 130)
    assert {65, 66, 67, 68, 94, 98, 126, 129, 97, 125} <= r
    # pack(): every point is met, slots are respected, nobody idles
    launches = af.pack([([0, 2], 5), ([0, 2], 6), ([0, 2], 7), (None, 1), (None, 9)], 4, 10)
    assert len(launches) == 2 and sorted(launches[0][[0, 2]].tolist()) == [5, 6] and launches[1][0] == 7
    assert all((l >= 0).all() and (l < 10).all() for l in launches) and {1, 9} <= set(np.concatenate(launches).tolist())


def test_plans_pinned_by_hand():
    """One or two shapes per row of the kernel table and both sides of each threshold, worked out from np_argreduce.hip with pencil:
    every number below is written out, none comes from the family."""
    K, T, B, Cc = af.Knobs, af.FOLD_THREAD, af.FOLD_BLOCK, af.FOLD_COLS_KERNEL
    # ROWS_GROUP: 10^6 rows of 10: L = 2 (2 * 8 >= 10), 2 * 10^6 lanes in 7813 workgroups; 1023 rows go to the wave kernel on 1 CU
    assert af.plan(1_000_000, 10, 1, A, 256) == _rec(1, 2, (7813, 1, 1), 1, 10)
    assert af.plan(1024, 256, 1, A, 256) == _rec(1, 32, (128, 1, 1), 1, 256)
    assert af.plan(1024, 8, 1, A, 256) == _rec(1, 1, (4, 1, 1), 1, 8) and af.plan(1024, 9, 1, A, 256)[af.TEMPLATE] == 2
    assert af.plan(1023, 10, 1, A, 1) == _rec(2, 0, (256, 1, 1), 1, 10)
    # ROWS_WAVE: 4096 = 256 * 16 rows of 257 (too long for the groups); 4095 rows: chunks = ceil(2049 / 4095) = 1
    assert af.plan(4096, 257, 1, A, 256) == _rec(2, 0, (1024, 1, 1), 1, 257)
    assert af.plan(4095, 257, 1, A, 256) == _rec(3, 0, (4095, 1, 1), 1, 257, 0, T, 0, (16, 1, 1))
    assert af.plan(5000, 32768, 1, A, 256)[af.KERNEL] == 2 and af.plan(5000, 32769, 1, A, 256)[af.KERNEL] == 3
    # ROWS: 10^8 elements on 256 CUs: 2049 chunks (odd), fold by workgroup; one CU: 9 wanted, 4097 elements allow 2
    assert af.plan(1, 100_000_000, 1, A, 256) == _rec(3, 0, (2049, 1, 1), 2049, 48805, 0, B, 0, (1, 1, 1))
    assert af.plan(1, 4096, 1, A, 1) == _rec(3, 0, (1, 1, 1), 1, 4096, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 4097, 1, A, 1) == _rec(3, 0, (2, 1, 1), 2, 2049, 0, T, 0, (1, 1, 1))
    assert af.plan(2, 32769, 1, A, 1) == _rec(3, 0, (10, 1, 1), 5, 6554, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 262145, 1, A, 8) == _rec(3, 0, (65, 1, 1), 65, 4033, 0, B, 0, (1, 1, 1))
    assert af.plan(1, 262144, 1, A, 8)[af.FOLD] == T                          # 64 chunks: the thread fold
    # SMALL_INNER: 1365 x 3 = 4095 elements stay out (-> the generic kernel: 3 outputs, 1365 >= 128 but 2048 / 3 -> chunks);
    # 1366 x 3: min_rows 1366, one slab of 1368 rows; 2733 x 3 on one CU: two slabs of ceil4(1367) = 1368, the last holds 1365
    assert af.plan(1, 1365, 3, A, 1)[af.KERNEL] == af.CHUNKS_KERNEL
    assert af.plan(1, 1366, 3, A, 1) == _rec(4, 0, (1, 1, 1), 1, 1368, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 2733, 3, A, 1) == _rec(4, 0, (2, 1, 1), 2, 1368, 0, T, 0, (1, 1, 1))
    # ... 3 x 1762 x 7: eight per CU over 3 slices = 3 slabs wanted, min_rows 586 allow 3: ceil4(588) = 588 rows, the last 586
    assert af.plan(3, 1762, 7, A, 1) == _rec(4, 0, (3, 3, 1), 3, 588, 0, T, 0, (1, 1, 1))
    # ... 300000 x 3 on 256 CUs: 512 wanted, 219 allowed: ceil4(1370) = 1372 rows, 219 slabs: the workgroup fold of 3 outputs
    assert af.plan(1, 300_000, 3, A, 256) == _rec(4, 0, (219, 1, 1), 219, 1372, 0, B, 0, (3, 1, 1))
    # SMALL_INNER4: 256 columns are groups of 4; 260 are not: tiles (2 of them, 1040-byte rows straddle lines: runs)
    assert af.plan(2, 67, 256, A, 1) == _rec(5, 0, (4, 2, 1), 4, 20, 0, T, 0, (2, 1, 1))
    assert af.plan(1, 1023, 4, A, 1)[af.KERNEL] == af.CHUNKS_KERNEL and af.plan(1, 1024, 4, A, 1) == _rec(5, 0, (1, 1, 1), 1, 1024, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 16, 260, A, 1) == _rec(6, 1, (2, 1, 1), 1, 16, 1)
    # COLS_TILE: 15 rows stay out; 2000 x 1003 on 256 CUs: 4 tiles, unaligned: 2048 / 4 = 512 chunks wanted, 2000 / 64 = 31 allowed:
    # 65 rows each, 31 chunks; the column fold: 16 * 1 < 64 and 63 * 1 < 64: COLS = 4, 251 workgroups
    assert af.plan(1, 15, 193, A, 1)[af.KERNEL] == af.GENERIC and af.plan(1, 16, 193, A, 1) == _rec(6, 1, (1, 1, 1), 1, 16, 0)
    assert af.plan(1, 2000, 1003, A, 256) == _rec(6, 0, (4, 31, 1), 31, 65, 1, Cc, 4, (251, 1, 1))
    # ... 4096 x 1024: aligned, on the line grid: 512 / 4 = 128 chunks wanted, 64 allowed, of 64 -> 65 rows: 64 chunks; COLS = 64 needs
    # 16 * 1 >= 64: no; 64 * 1 >= 64: COLS = 16.  One float off: 8 per CU, still 64 chunks, runs
    assert af.plan(1, 4096, 1024, A, 256) == _rec(6, 0, (4, 64, 1), 64, 65, 0, Cc, 16, (64, 1, 1))
    assert af.plan(1, 4096, 1024, A + 4, 256) == _rec(6, 0, (4, 64, 1), 64, 65, 1, Cc, 16, (64, 1, 1))
    assert af.plan(1, 4096, 1024, A + 4, 256, K(xcd_runs_off=1))[af.XCD_RUNS] == 0
    # ... one CU, 128 x 193 one float off 16 bytes: 8 / 1 = 8 wanted, 2 allowed: 64 -> 65 rows; aligned 260 columns: 2 / 2 = 1 chunk
    assert af.plan(1, 128, 193, A + 4, 1) == _rec(6, 0, (1, 2, 1), 2, 65, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 130, 260, A, 1) == _rec(6, 1, (2, 1, 1), 1, 130, 1) and af.plan(1, 130, 260, A + 4, 1)[af.CHUNKS] == 2
    # ... nine chunks of 65 rows in 577; 4 * 1 < 64, 13 * 1 < 64: COLS = 4, 49 workgroups; with 5 slices 13 * 5 = 65: COLS = 16
    assert af.plan(1, 577, 193, A, 2) == _rec(6, 0, (1, 9, 1), 9, 65, 0, Cc, 4, (49, 1, 1))
    assert af.plan(5, 576, 193, A, 6) == _rec(6, 0, (1, 9, 5), 9, 65, 0, Cc, 16, (13, 5, 1))
    assert af.plan(16, 579, 193, A, 18) == _rec(6, 0, (1, 9, 16), 9, 65, 0, Cc, 64, (4, 16, 1))
    # CHUNKS: 127 rows stay out; 129 x 191 on one CU: ceil(2048 / 191) = 11 wanted, 4 allowed: 33 rows each; 1052 lanes in 5 workgroups
    assert af.plan(1, 127, 65, A, 1) == _rec(8, 0, (1, 1, 1), 1, 127)
    assert af.plan(1, 129, 191, A, 1) == _rec(7, 0, (3, 1, 1), 4, 33, 0, T, 0, (1, 1, 1))
    assert af.plan(1, 300_000, 5, A, 256)[af.KERNEL] == af.SMALL_INNER and af.plan(1, 300, 5, A, 256) == _rec(7, 0, (1, 1, 1), 9, 34, 0, T, 0, (1, 1, 1))
    # GENERIC: (3, 5, 7); 4550 outputs on one CU: capped at 16 workgroups
    assert af.plan(3, 5, 7, A, 256) == _rec(8, 0, (1, 1, 1), 1, 5) and af.plan(70, 3, 65, A, 1) == _rec(8, 0, (16, 1, 1), 1, 3)
    assert af.plan(0, 5, 7, A, 1) is None and af.plan(3, 0, 7, A, 1) is None and af.plan(3, 5, 0, A, 1) is None
    assert af.capped_grid(9, 8) == 9 and af.capped_grid(2049, 2048) == 2049 and af.capped_grid(0, 8) == 1 and af.capped_grid(5, 8) == 5
    assert af.instantiation(af.plan(5, 576, 193, A, 6)) == "COLS_TILE<FINAL=0>+FOLD_COLS<16>"
    assert af.describe(af.plan(1, 128, 193, A + 4, 1)) == "COLS_TILE<FINAL=0>+FOLD_THREAD grid=(1,2,1) chunks=2 chunk_len=65 xcd_runs=0 fold_grid=(1,1,1)"


def test_header_constants_prototype_and_probe_without_a_device():
    from numpower_amd import _lib
    header = (ROOT / "include" / "np_hip_debug.h").read_text()
    assert "int np_debug_argreduce_last_record(unsigned *host_record, unsigned capacity, unsigned *host_count);" in header
    assert "np_debug_argreduce_last_record" not in (ROOT / "include" / "np_hip.h").read_text()
    assert "NP_ARG_" not in (ROOT / "include" / "np_hip.h").read_text()
    names = dict(re.findall(r"#define NP_ARG_KERNEL_(\w+) (\d+)u", header))
    assert {k: int(v) for k, v in names.items()} == {v: k for k, v in af.KERNEL_NAMES.items()}
    folds = dict(re.findall(r"#define NP_ARG_FOLD_(NONE|THREAD|BLOCK|COLS_KERNEL) (\d+)u", header))
    assert {k: int(v) for k, v in folds.items()} == {v: k for k, v in af.FOLD_NAMES.items()}
    assert "#define NP_ARG_RECORD_WORDS %du" % af.RECORD_WORDS in header
    for name, value in (("KERNEL", af.KERNEL), ("TEMPLATE", af.TEMPLATE), ("GRID_X", af.GRID_X), ("GRID_Y", af.GRID_Y), ("GRID_Z", af.GRID_Z),
                        ("CHUNKS", af.CHUNKS), ("CHUNK_LEN", af.CHUNK_LEN), ("XCD_RUNS", af.XCD_RUNS), ("FOLD", af.FOLD), ("FOLD_COLS", af.FOLD_COLS),
                        ("FOLD_GRID_X", af.FOLD_GRID_X), ("FOLD_GRID_Y", af.FOLD_GRID_Y), ("FOLD_GRID_Z", af.FOLD_GRID_Z)):
        assert "#define NP_ARG_%s %d\n" % (name, value) in header
    lib = _lib.load()
    assert hasattr(lib, "np_debug_argreduce_last_record") and len(_lib.PROTOTYPES["np_debug_argreduce_last_record"][1]) == 3
    words, count = (C.c_uint * af.RECORD_WORDS)(*([7] * af.RECORD_WORDS)), C.c_uint(9)
    assert lib.np_debug_argreduce_last_record(None, 0, None) != 0 and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_argreduce_last_record(None, 1, C.byref(count)) != 0
    assert lib.np_debug_argreduce_last_record(words, 1, C.byref(count)) == 0 and count.value == 0 and list(words) == [7] * af.RECORD_WORDS
    # the knobs are host state; a call with nothing to reduce, and a refusal, clear the record and need no device
    for code in af.codes(af.Knobs(5, 3, 1)) + af.DEFAULT_CODES:
        assert lib.np_reduce_set_variant(code) == 0
    assert lib.np_argreduce(1, None, 0, 3, 3, None) == 0 and lib.np_argreduce(0, None, 3, 0, 3, None) != 0
    assert lib.np_debug_argreduce_last_record(words, 1, C.byref(count)) == 0 and count.value == 0
    assert af.codes(af.Knobs()) == af.DEFAULT_CODES


def test_the_gpu_cases_without_a_device():
    """tests/test_gpu_argreduce_exact.py's CASES with the device taken out (256 CUs where a case runs on the device's own count):
    at every offset the plan shows the instantiation the case names; every kernel, every L, both FINAL values, every fold form
    and every COLS is named by a case; the features the table asks for are met."""
    from tests import test_gpu_argreduce_exact as t
    seen, feats = set(), set()
    total = 0
    for kernel, cases in t.CASES.items():
        assert cases, kernel
        for case in cases:
            cus = case.cus or 256
            assert set(case.families) <= set(af.FAMILIES) and {"permutation", "nan_rules"} <= set(case.families)
            for off in case.offsets:
                addr = A + 4 * (t.FRONT + off)
                rec = af.plan(case.outer, case.n, case.inner, addr, cus, case.knobs)
                assert af.instantiation(rec) == case.path, (kernel, case, off, af.describe(rec))
                seen.add(case.path)
                total += 1
                k = rec[af.KERNEL]
                if k == af.COLS_TILE:
                    wgs = rec[af.GRID_X] * rec[af.GRID_Y] * rec[af.GRID_Z]
                    feats.add(("tile", "xcd%d" % rec[af.XCD_RUNS], "wg%%8=%s" % ("0" if wgs % 8 == 0 else "x"), "outer>1" if case.outer > 1 else "outer1"))
                    feats.add(("tile chunks", min(rec[af.CHUNKS], 9)))
                    feats.add(("tile aligned", case.inner % 4 == 0 and addr % 16 == 0))
                    feats.add(("tile ncol", case.inner % 4, rec[af.GRID_X]))
                    assert rec[af.CHUNKS] == 1 or rec[af.CHUNK_LEN] % 2 == 1
                if k in (af.SMALL_INNER, af.SMALL_INNER4):
                    last = case.n - (rec[af.CHUNKS] - 1) * rec[af.CHUNK_LEN]
                    feats.add(("flat", k, "slabs", min(rec[af.CHUNKS], 3)))
                    feats.add(("flat", k, "last slab rows", min(last, 4)))
                    feats.add(("flat", k, "cnt%4", last * case.inner % 4))
                    feats.add(("flat", k, "wg per CU", rec[af.CHUNKS] * case.outer // cus if not case.knobs.flat_wg_per_cu else 0))
                if k == af.ROWS:
                    feats.add(("rows chunks", rec[af.CHUNKS]))
                if k == af.CHUNKS_KERNEL:
                    feats.add(("chunks len%4", rec[af.CHUNK_LEN] % 4))
                    feats.add(("chunks short last", case.n % rec[af.CHUNK_LEN] != 0))
                if k == af.ROWS_WAVE:
                    feats.add(("wave rows%4", case.outer % 4))
                    feats.add(("wave heads", len({af.head_of(addr + 4 * o * case.n, case.n) for o in range(case.outer)})))
    want = {"ROWS_GROUP<L=%d>" % L for L in (1, 2, 4, 8, 16, 32)} | {"ROWS_WAVE", "ROWS+FOLD_THREAD", "ROWS+FOLD_BLOCK", "SMALL_INNER+FOLD_THREAD",
            "SMALL_INNER4+FOLD_THREAD", "COLS_TILE<FINAL=1>", "COLS_TILE<FINAL=0>+FOLD_THREAD", "COLS_TILE<FINAL=0>+FOLD_COLS<4>",
            "COLS_TILE<FINAL=0>+FOLD_COLS<16>", "COLS_TILE<FINAL=0>+FOLD_COLS<64>", "CHUNKS+FOLD_THREAD", "GENERIC"}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert total > 400
    need = {("tile chunks", c) for c in (1, 2, 3, 5, 8, 9)} | {("tile aligned", True), ("tile aligned", False)}
    need |= {("tile ncol", r, tiles) for r, tiles in ((1, 1), (2, 1), (3, 1), (0, 1), (1, 2), (0, 2), (1, 3))}
    need |= {("tile", "xcd1", "wg%8=0", "outer>1"), ("tile", "xcd1", "wg%8=x", "outer1"), ("tile", "xcd1", "wg%8=x", "outer>1"), ("tile", "xcd0", "wg%8=x", "outer>1")}
    need |= {("flat", k, "slabs", s) for k in (af.SMALL_INNER, af.SMALL_INNER4) for s in (1, 2, 3)}
    need |= {("flat", k, "last slab rows", r) for k in (af.SMALL_INNER, af.SMALL_INNER4) for r in (1, 2, 3, 4)} | {("flat", af.SMALL_INNER, "cnt%4", r) for r in (0, 1, 2, 3)}
    need |= {("flat", k, "wg per CU", w) for k in (af.SMALL_INNER, af.SMALL_INNER4) for w in (2,)} | {("flat", af.SMALL_INNER, "wg per CU", 9)}
    need |= {("rows chunks", c) for c in (1, 2, 3, 5, 9, 65)} | {("chunks len%4", r) for r in range(4)} | {("chunks short last", True)}
    need |= {("wave rows%4", r) for r in range(4)} | {("wave heads", 1), ("wave heads", 4)}
    assert need <= feats, sorted(need - feats, key=str)
    # the lengths of the wave kernel: nvec < 64, 64 .. 256, and 1 / 2 / 3 vectors left per lane with and without the main loop
    nvecs = {c.n // 4 for c in t.CASES["rows_wave"] if c.path == "ROWS_WAVE"}
    for lo, hi in ((0, 63), (64, 64), (128, 128), (192, 192), (256, 256), (320, 320), (384, 384), (448, 448), (8192, 8192)):
        assert any(lo <= v <= hi for v in nvecs), (lo, hi)
