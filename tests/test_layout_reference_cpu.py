"""CPU-tier checks of the layout family (tests/layout_family.py) and of the probe's boundary: the patterns are distinct, hold every
special value and share no word with the canaries; expect() is numpy's transpose on the views and a stray write shows; fuse() is
checked exhaustively against numpy; the header's NP_LAYOUT_* constants are the family's; one plan per kernel family is pinned by
hand, so a typo in the restated dispatcher cannot agree with itself; the probe answers without a device; the cases of the GPU
module are walked with the device taken out: every named path is the planned one and every instantiation is reached."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

from tests import layout_family as lf

ROOT = Path(__file__).resolve().parent.parent


def test_patterns_are_distinct_special_and_disjoint_from_the_canaries():
    for n, salt in ((16, 0), (16, 7), (1000, 3), (70_000, 5), (1 << 21, 1)):
        w = lf.words(n, salt)
        assert w.dtype == np.uint32 and np.unique(w).size == n
        assert all(lf.specials(w).values()), (n, salt, lf.specials(w))
        for base in (lf.OUT_CANARY, lf.IN_CANARY):
            assert not np.isin(w >> 16, [base >> 16]).any()
        for i in (0, 1, 9, n - 1):
            assert lf.source_index(w[i], salt) == i
    # the largest operand of the GPU tests stays inside the runs of the bases, and the runs stay apart
    bases = sorted(lf.BASES.tolist())
    assert min(b - a for a, b in zip(bases, bases[1:])) >= lf.MAX_WORDS // 8 and 5000 * 4099 <= lf.MAX_WORDS
    assert bases[-1] + lf.MAX_WORDS // 8 <= 1 << 32
    with pytest.raises(ValueError):
        lf.words(lf.MAX_WORDS + 1)
    assert set(lf.words(64, 2).tolist()) == set(lf.words(64, 6).tolist()) and (lf.words(64, 2) != lf.words(64, 6)).all()
    assert lf.source_index(lf.OUT_CANARY | 5) is None and lf.source_index(lf.IN_CANARY) is None
    c = lf.canary(70_000)
    assert (c >> 16 == lf.OUT_CANARY >> 16).all() and c[1] != c[2] and lf.specials(lf.words(8, 0))["-0"]


@pytest.mark.parametrize("shape,perm", [((5, 7), (1, 0)), ((3, 4, 5), (2, 0, 1)), ((2, 3, 4, 5), (3, 1, 0, 2)), ((6,), (0,)), ((1, 1, 4), (2, 1, 0))])
def test_expect_is_numpys_transpose_inside_the_frame(shape, perm):
    n = int(np.prod(shape))
    for salt, off in ((0, 0), (3, 1), (5, 32)):
        image = lf.expect(shape, perm, salt, off)
        assert image.size == off + n + lf.OUT_TAIL
        x = lf.words(n, salt).view(np.float32).reshape(shape)
        assert (image[off:off + n] == np.ascontiguousarray(np.transpose(x, perm)).view(np.uint32).reshape(-1)).all()
        blank = lf.blank_output(n, off)
        assert (image[:off] == blank[:off]).all() and (image[off + n:] == blank[off + n:]).all()
        # what the comparison sees: one float written one place outside the output, in front of it or behind it, and a swap inside
        for at in ([off - 1] if off else []) + [off + n]:
            stray = image.copy()
            stray[at] = image[off]
            assert (stray != image).sum() == 1
        if n > 1:
            swapped = image.copy()
            swapped[[off, off + 1]] = swapped[[off + 1, off]]
            assert (swapped != image).sum() == 2


def test_framed_input_and_expect_strided():
    buf = lf.words(200, 4)
    image = lf.framed_input(buf, 3)
    assert image.size == 3 + 200 + lf.IN_TAIL and (image[3:203] == buf).all() and (image[:3] >> 16 == lf.IN_CANARY >> 16).all()
    want = lf.expect_strided(buf, 49, (4, 10), (50, -1), 2)
    ref = buf.reshape(4, 50)[:, ::-1][:, :10]
    assert (want[2:42] == ref.reshape(-1)).all() and want.size == 2 + 40 + lf.OUT_TAIL
    assert (lf.expect_strided(buf, 0, (3, 5), (0, 2))[:15] == np.tile(buf[0:10:2], 3)).all()


def _check_fuse(shape, perm):
    fshape, fperm = lf.fuse(shape, perm)
    n = int(np.prod(shape))
    x = np.arange(n).reshape(shape)
    assert int(np.prod(fshape)) == n and sorted(fperm) == list(range(len(fshape))) and 1 not in fshape
    got = np.transpose(x.reshape(fshape), fperm).reshape(-1) if fshape else x.reshape(-1)
    assert (got == np.transpose(x, perm).reshape(-1)).all(), (shape, perm, fshape, fperm)
    # nothing left to fuse: no two neighbouring input axes stay neighbours in order
    assert all(fperm[o + 1] != fperm[o] + 1 for o in range(len(fperm) - 1)), (shape, perm, fshape, fperm)


def test_fuse_every_permutation_of_up_to_five_axes():
    count = 0
    for ndim in range(0, 6):
        for shape in itertools.product((1, 2, 3), repeat=ndim):      # extent-1 axes in every position and every number
            for perm in itertools.permutations(range(ndim)):
                _check_fuse(shape, perm)
                count += 1
    assert count == 1 + 3 + 9 * 2 + 27 * 6 + 81 * 24 + 243 * 120
    assert lf.fuse((30, 3, 64, 65), (0, 2, 3, 1)) == ((30, 3, 4160), (0, 2, 1))
    assert lf.fuse((2, 3, 4, 5, 6, 7), (5, 0, 1, 2, 3, 4)) == ((720, 7), (1, 0))
    assert lf.fuse((5, 1, 7, 1, 9), (4, 3, 2, 1, 0)) == ((5, 7, 9), (2, 1, 0))
    assert lf.fuse((3, 1, 5, 7), (0, 2, 1, 3)) == ((105,), (0,)) and lf.fuse((1, 1), (1, 0)) == ((), ())


@pytest.mark.parametrize("shape,perm", [((2, 3, 1, 2, 3, 2, 1, 2), (7, 6, 5, 4, 3, 2, 1, 0)), ((2, 3, 1, 2, 3, 2, 1, 2), (0, 1, 2, 3, 4, 5, 6, 7)),
                                        ((2, 1, 3, 2, 1, 2, 3, 2), (2, 3, 0, 1, 6, 7, 4, 5)), ((3, 2, 2, 1, 1, 2, 3, 2), (5, 6, 7, 4, 3, 0, 1, 2)),
                                        ((2, 2, 2, 2, 2, 2, 2, 2), (1, 0, 3, 2, 5, 4, 7, 6)), ((4, 5, 6, 7, 8, 3, 2, 2), (7, 6, 5, 4, 3, 2, 1, 0)),
                                        ((1, 2, 1, 3, 1, 2, 1, 3), (1, 3, 5, 7, 0, 2, 4, 6))])
def test_fuse_eight_axes(shape, perm):
    _check_fuse(shape, perm)


def test_header_constants_prototype_and_probe_without_a_device():
    from numpower_amd import _lib
    header = (ROOT / "include" / "np_hip_debug.h").read_text()
    assert "int np_debug_layout_last_record(unsigned *host_record, unsigned capacity, unsigned *host_count);" in header
    assert "np_debug_layout_last_record" not in (ROOT / "include" / "np_hip.h").read_text()
    names = dict(re.findall(r"#define NP_LAYOUT_PATH_(\w+) (\d+)u", header))
    assert {k: int(v) for k, v in names.items()} == {v: k for k, v in lf.FAMILY_NAMES.items()}
    assert "#define NP_LAYOUT_RECORD_WORDS %du" % lf.RECORD_WORDS in header
    for name, value in (("FAMILY", lf.FAMILY), ("FORM", lf.FORM), ("ORDER", lf.ORDER), ("GRID_X", lf.GRID_X), ("GRID_Y", lf.GRID_Y),
                        ("GRID_Z", lf.GRID_Z), ("EXTRA", lf.EXTRA)):
        assert "#define NP_LAYOUT_%s %d\n" % (name, value) in header
    lib = _lib.load()
    assert hasattr(lib, "np_debug_layout_last_record") and len(_lib.PROTOTYPES["np_debug_layout_last_record"][1]) == 3
    words, count = (C.c_uint * lf.RECORD_WORDS)(*([7] * lf.RECORD_WORDS)), C.c_uint(9)
    assert lib.np_debug_layout_last_record(None, 0, None) != 0 and b"null pointer" in lib.np_last_error()
    assert lib.np_debug_layout_last_record(None, 1, C.byref(count)) != 0
    assert lib.np_debug_layout_last_record(words, 1, C.byref(count)) == 0 and count.value == 0 and list(words) == [7] * lf.RECORD_WORDS
    # the knobs are host state; calls that have nothing to move clear the record and need no device
    for code in lf.Knobs(tile=6, walign64_below=0, walign_order=2, tile_order=1, plane_order=0).codes() + lf.DEFAULT_CODES:
        assert lib.np_layout_set_variant(code) == 0
    assert lib.np_transpose2d(None, None, 0, 3, 3) == 0 and lib.np_copy2d(None, 4, None, 4, 0, 3) == 0
    assert lib.np_debug_layout_last_record(words, 1, C.byref(count)) == 0 and count.value == 0


A, B = 0x7F0000000000, 0x7F1000000000          # two addresses on the 128-byte grid


def _rec(family, form, order, grid, extra=()):
    return tuple([family, form, order] + list(grid) + list(extra) + [0] * (lf.RECORD_WORDS - 6 - len(extra)))


def test_plans_pinned_by_hand():
    """One or two shapes per kernel family, worked out from np_layout.hip with pencil: every number below is written out, none
    comes from the family."""
    K = lf.Knobs
    # MEMCPY: (3, 1, 5, 7) with the two middle axes swapped fuses to one axis
    assert lf.plan_permute((3, 1, 5, 7), (0, 2, 1, 3), A, B, 256) == _rec(1, 0, 0, (0, 0, 0))
    assert lf.plan_strided_copy((5, 1, 7), (7, 999, 1), 256) == _rec(1, 0, 0, (0, 0, 0))
    assert lf.plan_copy2d(64, 64, 64, 9, 256) == _rec(1, 0, 0, (0, 0, 0))
    # INTERLEAVE: 3 planes of 4100 positions, batch 5: 3 tiles of 2048; the way back; off 16 bytes it is the skinny kernel
    assert lf.plan_transpose2d(5, 3, 4100, A, B, 256) == _rec(2, 3 | 1 << 8, 0, (3, 5, 1))
    assert lf.plan_transpose2d(5, 4100, 3, A, B, 256) == _rec(2, 3, 0, (3, 5, 1))
    assert lf.plan_transpose2d(5, 3, 4100, A + 4, B, 256) == _rec(3, 0, 0, (17, 5, 1))
    # SKINNY: 100003 x 3 is tall: 391 workgroups of 256 rows; 16 x 10^7 is capped at 32 per CU
    assert lf.plan_transpose2d(1, 100_003, 3, A, B, 256) == _rec(3, 1, 0, (391, 1, 1))
    assert lf.plan_transpose2d(2, 16, 10_000_000, A, B, 256) == _rec(3, 0, 0, (8192, 2, 1))
    # TILE: 257 x 1001 on 256 CUs: 3 x 8 = 24 tiles of 128 < 1024 -> 64-tiles, 16 x 5 of them, not VEC
    assert lf.plan_transpose2d(1, 257, 1001, A, B, 256) == _rec(4, 64, 0, (80, 1, 1), (16, 5, 1001, 257, 1))
    # ... 4096 x 4096: 1024 tiles of 128, rows on the line grid, VEC; forced XCD runs
    assert lf.plan_transpose2d(1, 4096, 4096, A, B, 256, K(tile_order=1)) == _rec(4, 128 | 1 << 8, 1, (1024, 1, 1), (32, 32, 4096, 4096, 1))
    # ... 1031 x 1033 never reaches the write-aligned kernel on 256 CUs (81 tiles of 128): 17 x 17 tiles of 64
    assert lf.plan_transpose2d(1, 1031, 1033, A, B, 256) == _rec(4, 64, 0, (289, 1, 1), (17, 17, 1033, 1031, 1))
    # WALIGN: 4099^2: 33 x 33 = 1089 tiles of 128 >= 1024, below 1200 -> 64-tiles: 65 x ceil(4130 / 64) = 65 x 65, order 1
    assert lf.plan_transpose2d(1, 4099, 4099, A, B, 256) == _rec(5, 64, 1, (4225, 1, 1), (65, 65, 4099, 4099, 1))
    # ... 5000 x 4099: 40 x 33 = 1320 tiles -> 128-tiles: 33 x ceil(5031 / 128) = 33 x 40
    assert lf.plan_transpose2d(1, 5000, 4099, A, B, 256) == _rec(5, 128, 1, (1320, 1, 1), (33, 40, 4099, 5000, 1))
    # ... 8191 x 8193 is above 6 * 10^7 elements: order 0; an output 16 bytes off the grid: the plain 128-tiles, 65 x 64
    assert lf.plan_transpose2d(1, 8191, 8193, A, B, 256) == _rec(5, 128, 0, (65 * 65, 1, 1), (65, 65, 8193, 8191, 1))
    assert lf.plan_transpose2d(1, 8191, 8193, A, B + 16, 256) == _rec(4, 128, 0, (65 * 64, 1, 1), (65, 64, 8193, 8191, 1))
    # ... on one CU 259 x 130 is 3 x 2 = 6 >= 4 tiles of 128: write-aligned 64-tiles 3 x ceil(290 / 64) = 3 x 5; 128-tiles with 7000: 2 x 3
    assert lf.plan_transpose2d(1, 259, 130, A, B, 1) == _rec(5, 64, 1, (15, 1, 1), (3, 5, 130, 259, 1))
    assert lf.plan_transpose2d(1, 259, 130, A, B, 1, K(walign64_below=0, walign_order=2)) == _rec(5, 128, 2, (6, 1, 1), (2, 3, 130, 259, 1))
    # the pitched planes of (70, 130, 66) reversed: A = 70 rows, B = 66 columns, rows 130 * 66 apart, output rows 130 * 70 apart
    assert lf.plan_permute((70, 130, 66), (2, 1, 0), A, B, 256) == _rec(4, 64, 0, (4, 1, 130), (2, 2, 8580, 9100, 1))
    # ... through np_permute to the write-aligned kernel: (2, 257, 2, 64) -> (N, M, B, A): out_pitch 257, batch strides 64 * 257 * (1, 2)
    assert lf.plan_permute((2, 257, 2, 64), (2, 0, 3, 1), A, B, 1) == _rec(5, 64, 1, (5, 1, 4), (1, 5, 128, 257, 2))
    # PLANE: (100, 3, 100, 2) -> (2, 1, 0, 3): E = 2, side 45 (45 * 45 * 2 = 4050), 3 tiles of 34 along B, rows of 68 floats at pitch
    # 128 + 2 = 130, ta_max = min(4096 / 68 = 60, 4608 / 130 = 35) -> 3 tiles of 34 along A; 3 * 3 * 3 workgroups
    assert lf.plan_permute((100, 3, 100, 2), (2, 1, 0, 3), A, B, 256) == _rec(6, 1, 1, (27, 1, 1), (100, 100, 2, 34, 34, 3, 3, 130, 1))
    # ... (6, 40, 300, 8) with axes 1, 2 swapped: float4 elements, E = 2 of them, cap 1024: side 22, B = 300 -> 14 tiles of 22,
    # rows of 44 at pitch 45, ta_max = min(1024 / 44 = 23, 1152 / 45 = 25, A = 40) = 23 -> 2 tiles of 20; 2 * 14 * 6 = 168
    assert lf.plan_permute((6, 40, 300, 8), (0, 2, 1, 3), A, B, 256) == _rec(6, 4, 0, (168, 1, 1), (40, 300, 2, 20, 22, 2, 14, 45, 0))
    # ... one float off 16 bytes: single floats, E = 8: side 22 again (22 * 22 * 8 = 3872), rows of 176 floats at pitch 192 + 8,
    # ta_max = min(4096 / 176 = 23, 4608 / 200 = 23) -> 2 tiles of 20
    assert lf.plan_permute((6, 40, 300, 8), (0, 2, 1, 3), A + 4, B, 256) == _rec(6, 1, 1, (168, 1, 1), (40, 300, 8, 20, 22, 2, 14, 200, 1))
    # ... a short A lengthens the B run: (5, 3, 1000) reversed: room 4096 / 5 = 819 -> 256, 4 tiles of 250 at pitch 251, one of 5 along A
    assert lf.plan_permute((5, 3, 1000), (2, 1, 0), A, B, 256) == _rec(6, 1, 1, (12, 1, 1), (5, 1000, 1, 5, 250, 1, 4, 251, 1))
    # GATHER: a kept inner axis of 32: float4s, 9 * 11 * 8 = 792 of them in 4 workgroups; of 33: 3267 floats in 13
    assert lf.plan_permute((9, 11, 32), (1, 0, 2), A, B, 256) == _rec(7, 32 | 4 << 8, 0, (4, 1, 1))
    assert lf.plan_permute((9, 11, 33), (1, 0, 2), A, B, 256) == _rec(7, 32 | 1 << 8, 0, (13, 1, 1))
    # ... capped at 16 workgroups per CU; the plane path switched off (variant 3): the reversal is a gather of single floats
    assert lf.plan_permute((40, 41, 64), (1, 0, 2), A, B, 1) == _rec(7, 32 | 4 << 8, 0, (16, 1, 1))
    assert lf.plan_permute((9, 10, 11, 12), (3, 2, 1, 0), A, B, 256, K(tile=3)) == _rec(7, 32 | 1 << 8, 0, (47, 1, 1))
    assert lf.plan_strided_copy((30, 64), (-64, 1), 256) == _rec(7, 32 | 4 << 8, 0, (2, 1, 1))
    assert lf.plan_strided_copy((30, 64), (130, 1), 256) == _rec(7, 32 | 1 << 8, 0, (8, 1, 1))
    assert lf.plan_strided_copy((1 << 16, 1 << 16), (1 << 17, 1), 256)[lf.FORM] == 32 | 4 << 8      # 2^30 float4s
    assert lf.plan_strided_copy((1 << 16, 1 << 16), (1 << 17, 2), 256)[lf.FORM] == 64 | 1 << 8      # 2^32 floats: 64-bit indices
    # ... the two 64-bit-index launches the suite makes, both in tests/test_gpu_fullsize.py::test_layout_beyond_2p31_elements: (23171, 2, 46350)
    # with the first two axes swapped, and the reversed, transposing np_strided_copy of 46342 x 46350
    assert lf.plan_permute((23171, 2, 46350), (1, 0, 2), A, B, 256) == _rec(7, 64 | 1 << 8, 0, (4096, 1, 1))
    assert lf.plan_strided_copy((46350, 46342), (1, -46350), 256) == _rec(7, 64 | 1 << 8, 0, (4096, 1, 1))
    # COPY2D: 37 rows of 64 floats = 592 float4s in 3 workgroups; of 63: 2331 floats in 10
    assert lf.plan_copy2d(67, 64, 64, 37, 256) == _rec(8, 4, 0, (3, 1, 1))
    assert lf.plan_copy2d(70, 80, 63, 37, 256) == _rec(8, 1, 0, (10, 1, 1))
    assert lf.plan_transpose2d(0, 4, 4, A, B, 256) is None and lf.plan_permute((4, 0), (1, 0), A, B, 256) is None
    assert lf.describe(lf.plan_transpose2d(1, 259, 130, A, B, 1)) == "WALIGN<64> order=1 tiles=3x5 pitch=130/259 nbatch=1 grid=(15,1,1)"
    assert lf.instantiation(lf.plan_permute((6, 40, 300, 8), (0, 2, 1, 3), A, B, 256)) == "PLANE<W=4> xcd_runs=0"


def test_no_entry_point_loses_vec_to_a_batch_stride_alone():
    """plan_planes restates the rule (a batch stride that is no multiple of 4 floats sends an otherwise float4-loadable transpose to
    the dword form), and no shape reaches it: with rows and cols multiples of 4 every stride np_permute / np_transpose2d build is a
    multiple of rows or of cols.  Searched over every permutation of the 3- and 4-axis shapes below."""
    pb = lf.PlaneBatch(256, 128, [3], [128 * 256 + 2], [128 * 256])
    assert lf.plan_planes(A, B, 3, 128, 256, pb, 1)[lf.FORM] == 128
    pb.bin = [128 * 256]
    assert lf.plan_planes(A, B, 3, 128, 256, pb, 1)[lf.FORM] == 128 | 1 << 8
    found = 0
    for shape in itertools.product((3, 64, 68), repeat=3):
        for perm in itertools.permutations(range(3)):
            rec = lf.plan_permute(shape, perm, A, B, 256)
            if rec[lf.FAMILY] == lf.TILE:
                fshape, fperm = lf.fuse(shape, perm)
                a_axis = fperm[-1]
                vec_without_batch = fshape[a_axis] % 4 == 0 and fshape[-1] % 4 == 0
                assert (rec[lf.FORM] >> 8 == 1) == vec_without_batch, (shape, perm)
                found += 1
    assert found >= 20


def test_the_gpu_cases_without_a_device(monkeypatch):
    """tests/test_gpu_layout_exact.py walked with the device taken out: every case's named instantiation is the one its plan shows
    (at 256 CUs where it runs on the device's own count), every expectation has the size of its frame, every operand of 64 elements
    and more holds every special value, every kernel instantiation of np_layout.hip except the 64-bit-index gather is reached, and
    out_pitch mod 32 takes all 31 values on both write-aligned tile sizes."""
    import contextlib
    import inspect
    from tests import test_gpu_layout_exact as t
    seen, shifts, launches, walked = set(), {64: set(), 128: set()}, [0], {}

    class Dev:
        cus = 256

    @contextlib.contextmanager
    def state(dev, cus=0, knobs=lf.Knobs()):
        yield cus if cus else dev.cus

    def launch(dev, what, path, payload, in_off, want_of, out_n, out_off, call, plan, salt=0):
        rec = plan(A + 4 * in_off, B + 4 * out_off)
        assert lf.instantiation(rec) == path, (what, path, lf.describe(rec))
        if payload.size <= 300_000:
            assert want_of(out_off).size == out_off + out_n + lf.OUT_TAIL, what
            assert payload.size < 64 or all(lf.specials(payload).values()), what
        seen.add(path)
        if rec[lf.FAMILY] == lf.WALIGN:
            shifts[rec[lf.FORM]].add(rec[lf.EXTRA + 3] % 32)
        launches[0] += 1

    monkeypatch.setattr(t, "state", state)
    monkeypatch.setattr(t, "launch", launch)
    for name, fn in inspect.getmembers(t, inspect.isfunction):
        if not name.startswith("test_") or "dev" not in inspect.signature(fn).parameters or name.startswith(("test_probe", "test_ndarray")):
            continue
        axes = []
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                # plain value lists only: a pytest.param or an indirect fixture would not be unpacked right below
                assert not mark.kwargs.get("indirect") and not any(hasattr(v, "marks") for v in mark.args[1]), name
                names = [a.strip() for a in mark.args[0].split(",")]
                axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in mark.args[1]])
        before = launches[0]
        for combo in itertools.product(*axes):
            fn(dev=Dev(), **{k: v for part in combo for k, v in part.items()})
        walked[name] = launches[0] - before
    # every test of the module that launches through launch() was walked, none quietly left out
    module_tests = {n for n, f in inspect.getmembers(t, inspect.isfunction) if n.startswith("test_")}
    assert module_tests - set(walked) == {"test_probe_is_cleared_by_calls_that_move_nothing",
                                          "test_ndarray_transpose_of_a_row_sliced_view_and_of_a_pending_chain"}
    assert all(count > 0 for count in walked.values()), walked
    assert walked["test_walign_every_shift"] == 31 * 2 * 9 and walked["test_skinny"] == 16 * 24 and walked["test_permute"] == len(t.PERMUTE_CASES)
    assert launches[0] > 1400
    want = {"MEMCPY", "SKINNY<TALL=0>", "SKINNY<TALL=1>", "GATHER<u32,W=1>", "GATHER<u32,W=4>", "COPY2D<V=1>", "COPY2D<V=4>"}
    want |= {"INTERLEAVE<R=%d,%s>" % (r, d) for r in (2, 3, 4) for d in ("to_interleaved", "to_planes")}
    want |= {"TILE<%d,VEC=%d> order=%d" % (tile, v, o) for tile in (64, 128) for v in (0, 1) for o in (0, 1)}
    want |= {"WALIGN<%d> order=%d" % (tile, o) for tile in (64, 128) for o in (0, 1, 2)}
    want |= {"PLANE<W=%d> xcd_runs=%d" % (w, x) for w in (1, 4) for x in (0, 1)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert shifts[64] >= set(range(1, 32)) and shifts[128] >= set(range(1, 32))
