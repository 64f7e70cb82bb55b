"""The thin, few-row and matrix-vector products of np_sgemm.hip against the exact family (tests/gemm_family.py): every element of
every case is compared BIT FOR BIT with the integer product, on operands where a dropped, doubled or mis-paired a.b moves the
result by at least 1, and every case asserts through np_sgemm_debug_last_path the WHOLE mask of what ran — kernel, template
instantiation class (lane width L, accumulator count MV), K-chunks, fold.

Through the C ABI (np_sgemm, np_sgemv).  A, B and x sit at float offsets 0 .. 3 inside NaN-filled allocations (a row view of a
3-D array arrives that way; every one of these kernels loads float4s from dword-aligned addresses), C inside a -777 canary frame
with a NaN interior; every case runs twice and compares the bits of the two runs.  One shape per path takes all 4 x 4 offset
pairs, the others the two diagonal extremes (0, 0) and (3, 3); the mask changes with alignment only where np_sgemv tests
aligned16 (sgemv_staged_rows_kernel, the vec form of sgemv_kernel): those cases are named.  One shape per path runs every
specials() kind at three K positions (first, last, one on a chunk / step boundary of that kernel).

Masks are written for the 256 CUs of the MI355X: the launchers size their K-chunks by np::num_cus().  The names are checked
against the dispatcher's arithmetic (gemm_family.path / gemv_path) in tests/test_gemm_reference_cpu.py, and again here."""
import ctypes as C

import pytest

from numpower_amd import _lib
from tests import gemm_family as gf
from tests.gemm_exact import ALL_OFFSETS, DIAGONAL, Dev, exact_operands, run, sgemm_variant, with_specials
from tests.gemm_family import (FEWROWS, FEWROWS_SPLITK1, FEWROWS_SPLITK2, FOLD, GEMV_CHUNKS, GEMV_FEWROWS_CHUNKS, GEMV_SHORT_ROWS,
                               GEMV_STAGED, GEMV_WAVE, GEMV_WAVE_VEC, LANES, MV, PEELED, SKINNY, THIN_CHUNKS, THIN_K_CHUNKS,
                               THIN_LANES, THIN_LEFT, THIN_MFMA16, THIN_MFMA32, THIN_MFMA32X2, TILED)

pytestmark = pytest.mark.gpu

THIN_Q_DEFAULT = 59          # g_thin_underfilled_to_planner


@pytest.fixture(scope="module")
def dev(hip):
    return Dev(hip)


def product(dev, m, n, k, mask, offsets=DIAGONAL, label=""):
    assert gf.path(m, n, k) == mask, "%s %s: the case names %s, the dispatcher's arithmetic gives %s" % (
        label, (m, n, k), gf.describe(mask), gf.describe(gf.path(m, n, k)))
    A, B, want = exact_operands(m, n, k)
    run(dev, A, B, want, mask, offsets, label=label)


def matvec(dev, m, n, mask, offsets=DIAGONAL, label=""):
    amp = gf.amp_for(n)
    A, _ = gf.operands(m, 1, n, 11, amp, amp)
    x = gf.vector(n, 12, amp)
    run(dev, A, x, gf.expected(A, x), mask, offsets, gemv=True, label=label)


# ---- sgemm_thin_kernel: every L ---------------------------------------------------------------------------------------------
def lanes_for(k):
    L = 1
    while L * 8 < k and L < 64:
        L *= 2
    return L


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_thin_lanes_every_width(n, dev):
    """sgemm_thin_kernel<NV, L>, L = 1 .. 64 by K (~8 k per lane), a ragged last workgroup (M = 2051); N = 1 with K >= 256 is
    np_sgemv and asserted as such (a wave per row, rows of any alignment)."""
    seen = set()
    for k in (1, 8, 9, 16, 17, 33, 65, 129, 255 if n == 1 else 257, 1023):
        for m in (2051, 2048):
            if n == 1 and k >= 256:
                mask = GEMV_WAVE                                   # 1023 % 4 != 0: never the vec form
            else:
                mask = THIN_LANES | LANES(lanes_for(k))
                seen.add(lanes_for(k))
            product(dev, m, n, k, mask, ALL_OFFSETS if (m, k) == (2051, 33) else DIAGONAL, "thin lanes")
    assert seen == ({1, 2, 4, 8, 16, 32, 64} if n > 1 else {1, 2, 4, 8, 16, 32})


def test_thin_lanes_many_rows_long_k(dev):
    """M >= 65536 keeps K >= 1024 on the lane-group kernel (B stays in the caches while the rows stream past)."""
    product(dev, 65537, 4, 1024, THIN_LANES | LANES(64), label="thin lanes, M >= 65536")


def test_thin_lanes_specials(dev):
    with_specials(dev, 2051, 3, 257, THIN_LANES | LANES(64), 64, label="thin lanes")


# ---- sgemm_thin_mfma_kernel over the whole K ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 16, 17, 31, 32])
def test_thin_mfma_whole_k(n, dev):
    """sgemm_thin_mfma_kernel<16> (N <= 16) / <32>: the float4 that straddles K, a tail inside a 32-step and a 64-chunk of B,
    M % 16 and M % 32 != 0."""
    mask = THIN_MFMA16 if n <= 16 else THIN_MFMA32
    for k in (4, 5, 7, 31, 33, 63, 64, 65, 129, 1021):
        for m in (2111, 2049):
            product(dev, m, n, k, mask, ALL_OFFSETS if (m, k) == (2111, 65) and n in (5, 31) else DIAGONAL, "thin mfma")


def test_thin_mfma_whole_k_specials(dev):
    with_specials(dev, 2049, 5, 129, THIN_MFMA16, 64, label="thin mfma 16")
    with_specials(dev, 2111, 31, 129, THIN_MFMA32, 63, label="thin mfma 32")


@pytest.mark.parametrize("mnk, kernel", [((2049, 9, 1027), THIN_MFMA16), ((2049, 24, 4099), THIN_MFMA32), ((4100, 16, 2050), THIN_MFMA16),
                                         # N <= 4 reaches the MFMA kernel only with K >= 1024 and M < 65536, and such a launch
                                         # (fewer than 2048 workgroups, K >= 1024) is always cut into K-chunks
                                         ((2049, 3, 1027), THIN_MFMA16)])
def test_thin_mfma_k_chunks_from_2048_rows(mnk, kernel, dev):
    """M >= 2048 with too few rows to fill the machine: 2 to 8 K-chunks of 576, the last one ragged, K % 4 != 0, folded."""
    product(dev, *mnk, kernel | THIN_K_CHUNKS | FOLD, ALL_OFFSETS if mnk == (2049, 9, 1027) else DIAGONAL, "thin mfma, K-chunks")
    if mnk == (2049, 9, 1027):
        with_specials(dev, *mnk, kernel | THIN_K_CHUNKS | FOLD, 576, label="thin mfma, K-chunks")


# ---- the K-chunked forms below 2048 rows: reached only with thin_to_planner() switched off ---------------------------------------
BELOW_2048 = [((17, 17, 16384), FEWROWS_SPLITK1 | FOLD), ((33, 32, 16387), FEWROWS_SPLITK1 | FOLD), ((64, 20, 20001), FEWROWS_SPLITK1 | FOLD),
              ((32, 33, 16384), FEWROWS_SPLITK2 | FOLD), ((64, 64, 17003), FEWROWS_SPLITK2 | FOLD), ((40, 63, 16390), FEWROWS_SPLITK2 | FOLD),
              ((100, 33, 16384), THIN_MFMA32X2 | THIN_K_CHUNKS | FOLD), ((2047, 50, 16386), THIN_MFMA32X2 | THIN_K_CHUNKS | FOLD),
              ((65, 64, 16389), THIN_MFMA32X2 | THIN_K_CHUNKS | FOLD),
              ((100, 9, 16384), THIN_MFMA16 | THIN_K_CHUNKS | FOLD), ((300, 16, 16387), THIN_MFMA16 | THIN_K_CHUNKS | FOLD),
              ((784, 10, 20000), THIN_MFMA16 | THIN_K_CHUNKS | FOLD), ((500, 32, 16385), THIN_MFMA32 | THIN_K_CHUNKS | FOLD),
              ((20, 8, 50000), THIN_MFMA16 | THIN_K_CHUNKS | FOLD),
              # fewer than four row tiles: waves of the workgroup that own no row
              ((30, 16, 20000), THIN_MFMA16 | THIN_K_CHUNKS | FOLD)]
FULL_OFFSETS_BELOW_2048 = {(33, 32, 16387), (40, 63, 16390), (65, 64, 16389), (300, 16, 16387), (500, 32, 16385)}
SPECIALS_BELOW_2048 = {(33, 32, 16387): 1055, (40, 63, 16390): 1056, (65, 64, 16389): 2111, (30, 16, 20000): 2240, (500, 32, 16385): 2112}


@pytest.mark.parametrize("mnk, mask", BELOW_2048)
def test_k_chunked_forms_below_2048_rows(mnk, mask, dev):
    """sgemm_fewrows_splitk_kernel<1> / <2>, sgemm_thin_mfma_kernel<32, 2> and the K-chunked <16> / <32> launches for 17 .. 2047
    rows: np_sgemm_set_variant(-(40 + 0)) keeps thin_to_planner() from handing them to the planner."""
    assert gf.path(*mnk, q=0) == mask
    A, B, want = exact_operands(*mnk)
    with sgemm_variant(dev, -40, -(40 + THIN_Q_DEFAULT)):
        run(dev, A, B, want, mask, ALL_OFFSETS if mnk in FULL_OFFSETS_BELOW_2048 else DIAGONAL, label="q = 0")
        if mnk in SPECIALS_BELOW_2048:
            with_specials(dev, *mnk, mask, SPECIALS_BELOW_2048[mnk], label="q = 0")


@pytest.mark.parametrize("mnk", [mnk for mnk, _ in BELOW_2048])
def test_the_same_shapes_go_to_the_planner_by_default(mnk, dev):
    """The round-5 rule as an assertion: at the default q = 59 each of these launches has fewer than 59 / 4 workgroups per CU
    (tests/test_gemm_reference_cpu.py restates the arithmetic) and goes to the tiled kernels — still exact.  Whether the planner
    cuts K and folds partials of its own is its model's business: FOLD is the one bit left open."""
    assert gf.path(*mnk) == TILED
    A, B, want = exact_operands(*mnk)
    run(dev, A, B, want, frozenset((TILED, TILED | FOLD)), DIAGONAL, label="default q")


# ---- sgemm_thin_chunks_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mnk", [(1, 1, 65536), (3, 3, 65539), (16, 8, 70001), (10, 7, 131073)])
def test_thin_chunks(mnk, dev):
    product(dev, *mnk, THIN_CHUNKS | FOLD, ALL_OFFSETS if mnk == (3, 3, 65539) else DIAGONAL, "thin chunks")
    if mnk == (3, 3, 65539):
        with_specials(dev, *mnk, THIN_CHUNKS | FOLD, 4097, label="thin chunks")


# ---- sgemm_fewrows_kernel: MV = 1, 2, 4, 8 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [(259, 23500), (256, 23440), (1031, 5821), (4099, 1467)])
def test_fewrows(nk, dev):
    """N % 4 != 0 (the lanes that are not `whole`), N % 256, chunks whose last one is short; every MV."""
    n, k = nk
    for m in (8, 5, 4, 3, 2, 1):
        mv = 1 if m == 1 else 2 if m == 2 else 4 if m <= 4 else 8
        product(dev, m, n, k, FEWROWS | MV(mv) | FOLD, ALL_OFFSETS if (m, n) == (3, 259) else DIAGONAL, "few rows")


def test_fewrows_specials(dev):
    with_specials(dev, 3, 259, 23500, FEWROWS | MV(4) | FOLD, 32, label="few rows")
    with_specials(dev, 8, 1031, 5821, FEWROWS | MV(8) | FOLD, 4100, label="few rows")


# ---- sgemm_skinny_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mnk, mask", [((9, 515, 31100), SKINNY | FOLD), ((17, 4099, 3907), SKINNY | FOLD), ((32, 4100, 3903), SKINNY | FOLD),
                                       ((32, 32771, 512), SKINNY)])      # one chunk: C written directly, no fold
def test_skinny(mnk, mask, dev):
    """K % 16 and K % 64 != 0, N % 4 != 0, N % 128 != 0; chunks > 1 with the fold, and one chunk without."""
    product(dev, *mnk, mask, ALL_OFFSETS if mnk == (17, 4099, 3907) else DIAGONAL, "skinny")


def test_skinny_specials(dev):
    with_specials(dev, 17, 4099, 3907, SKINNY | FOLD, 256, label="skinny")


# ---- sgemm_thin_left_kernel: MV = 4, 8, 16 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65536, 65537, 65538, 65539, 70001])
def test_thin_left(n, dev):
    for k in (1, 3, 64):
        for m in (16, 9, 8, 5, 4, 1):
            product(dev, m, n, k, THIN_LEFT | MV(4 if m <= 4 else 8 if m <= 8 else 16),
                    ALL_OFFSETS if (m, n, k) == (5, 65539, 3) else DIAGONAL, "thin left")


def test_thin_left_specials(dev):
    with_specials(dev, 5, 65539, 64, THIN_LEFT | MV(8), 32, label="thin left")
    with_specials(dev, 9, 65537, 64, THIN_LEFT | MV(16), 4, label="thin left")


# ---- try_peeled ------------------------------------------------------------------------------------------------------------------
def test_peeled_edges_forced(dev):
    """np_sgemm_set_variant(-11): the edge is peeled whenever there is one.  With one thin edge the form is forced: the column edge
    (2304 x 2 x 77) runs sgemm_thin_kernel<4, 16>, the row edge (1 x 2176 x 2760) sgemm_fewrows_kernel<1> over chunks with its fold,
    the main block the tiled kernels (whether those fold K-chunks of their own is the planner's model: the one bit left open where
    no edge folds).  With both edges (2305, 2178, 77) the model picks rows, columns or both; the row edge (1 x 2178 x 77) is too
    small for the few-row kernel and goes to the tiled ones, so the mask is PEELED | TILED with or without the column kernel."""
    main = PEELED | TILED
    columns = main | THIN_LANES | LANES(16)
    assert gf.path(2304, 2, 77) == THIN_LANES | LANES(16) and gf.path(1, 2176, 2760) == FEWROWS | MV(1) | FOLD and gf.path(1, 2178, 77) == TILED
    with sgemm_variant(dev, -11, -10):
        A, B, want = exact_operands(2304, 2178, 77)
        run(dev, A, B, want, frozenset((columns, columns | FOLD)), ((0, 0),), label="peeled columns")
        A, B, want = exact_operands(2305, 2178, 77)
        run(dev, A, B, want, frozenset((main, main | FOLD, columns, columns | FOLD)), ((0, 0),), label="peeled, both edges thin")
        A, B, want = exact_operands(2305, 2176, 2760)
        run(dev, A, B, want, main | FEWROWS | MV(1) | FOLD, ((0, 0),), label="peeled rows")
    A, B, want = exact_operands(2304, 2178, 77)
    run(dev, A, B, want, frozenset((TILED, TILED | FOLD)), ((0, 0),), label="not peeled by default")


# ---- np_sgemv --------------------------------------------------------------------------------------------------------------------
def short_rows_mask(n):
    L = 1
    while L * 8 < n:
        L *= 2
    return GEMV_SHORT_ROWS | LANES(min(L, 32))


@pytest.mark.parametrize("mn", [(262144, 4), (262145, 63), (262147, 7), (262400, 33)])
def test_sgemv_staged_rows(mn, dev):
    """sgemv_staged_rows_kernel needs a 16-byte aligned A (its slabs are float4 streams); at any other offset of A the lane-group
    kernel takes the shape.  x may start anywhere (it is copied to LDS by dwords)."""
    m, n = mn
    fallback = short_rows_mask(n)
    matvec(dev, m, n, lambda oa, ox: GEMV_STAGED if oa == 0 else fallback,
           ALL_OFFSETS if mn == (262147, 7) else ((0, 0), (0, 3), (1, 0), (3, 3)), "staged rows")
    assert gf.gemv_path(m, n) == GEMV_STAGED and gf.gemv_path(m, n, a_aligned=False) == fallback


@pytest.mark.parametrize("m", [1024, 1027])
def test_sgemv_short_rows_every_width(m, dev):
    seen = set()
    for n in (1, 8, 9, 16, 17, 33, 65, 129, 256):
        mask = short_rows_mask(n)
        seen.add(mask >> 20)
        assert gf.gemv_path(m, n) == mask
        matvec(dev, m, n, mask, ALL_OFFSETS if (m, n) == (1027, 33) else DIAGONAL, "short rows")
    assert seen == {1, 2, 3, 4, 5, 6}          # L = 1, 2, 4, 8, 16, 32


@pytest.mark.parametrize("n", [65536, 65537, 70003])
def test_sgemv_fewrows_chunks(n, dev):
    for m in (2, 3, 16):
        assert gf.gemv_path(m, n) == GEMV_FEWROWS_CHUNKS | FOLD
        matvec(dev, m, n, GEMV_FEWROWS_CHUNKS | FOLD, ALL_OFFSETS if (m, n) == (3, 65537) else DIAGONAL, "few rows, chunks")


@pytest.mark.parametrize("mn", [(1, 16384), (1, 65539), (17, 16387), (300, 20001)])
def test_sgemv_chunks(mn, dev):
    assert gf.gemv_path(*mn) == GEMV_CHUNKS | FOLD
    matvec(dev, *mn, GEMV_CHUNKS | FOLD, ALL_OFFSETS if mn == (17, 16387) else DIAGONAL, "chunks")


@pytest.mark.parametrize("mn, vec", [((5, 300), True), ((1023, 257), False), ((17, 260), True), ((4, 8191), False)])
def test_sgemv_wave(mn, vec, dev):
    """sgemv_kernel: the float4 form needs N % 4 == 0 and A and x both 16-byte aligned; x at offset 1 alone turns it off."""
    m, n = mn
    mask = (lambda oa, ox: GEMV_WAVE | (GEMV_WAVE_VEC if oa == 0 and ox == 0 else 0)) if vec else GEMV_WAVE
    assert gf.gemv_path(m, n) == GEMV_WAVE | (GEMV_WAVE_VEC if vec else 0) and gf.gemv_path(m, n, x_aligned=False) == GEMV_WAVE
    matvec(dev, m, n, mask, ALL_OFFSETS if mn in ((17, 260), (1023, 257)) else ((0, 0), (0, 1), (3, 3)), "wave per row")


def test_sgemv_specials(dev):
    with_specials(dev, 262147, 1, 7, GEMV_STAGED, 4, gemv=True, label="staged rows")
    with_specials(dev, 1027, 1, 33, GEMV_SHORT_ROWS | LANES(8), 16, gemv=True, label="short rows")
    with_specials(dev, 3, 1, 65537, GEMV_FEWROWS_CHUNKS | FOLD, 1028, gemv=True, label="few rows, chunks")
    with_specials(dev, 17, 1, 16387, GEMV_CHUNKS | FOLD, 4100, gemv=True, label="chunks")
    with_specials(dev, 17, 1, 260, GEMV_WAVE | GEMV_WAVE_VEC, 255, gemv=True, label="wave per row, vec")
    with_specials(dev, 1023, 1, 257, GEMV_WAVE, 255, gemv=True, label="wave per row")


def test_the_probe_follows_the_outermost_call(dev):
    """An empty product launches nothing and leaves 0; np_sgemm with N = 1 reports the np_sgemv kernel it handed the shape to, and
    a plain np_sgemv afterwards reports itself alone."""
    A, B, want = exact_operands(2048, 1, 1023)
    run(dev, A, B, want, GEMV_WAVE, ((0, 0),), label="N = 1")
    _lib.check(dev.L.np_sgemm(0, 4, 4, None, None, None))
    assert dev.last_path() == 0
    matvec(dev, 5, 300, GEMV_WAVE | GEMV_WAVE_VEC, ((0, 0),), "after")
    null = C.POINTER(C.c_uint)()
    assert dev.L.np_sgemm_debug_last_path(null) != 0
