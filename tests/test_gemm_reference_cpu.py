"""The exact product family (tests/gemm_family.py) against itself and against independent arithmetic, without a device: the
integer product must come out bit-identical from numpy's fp32 matmul, from fp32 loops over K in several orders and chunkings,
and from the oracle's OpenBLAS — which is what entitles tests/test_gpu_gemm_exact.py to compare a kernel with it bit for bit,
whatever order the kernel sums in.  Also here: the class maps of specials() against numpy's fp64 product, the dispatcher's
arithmetic behind every mask the GPU module names, and the probe's declaration."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import gemm_family as gf

ROOT = Path(__file__).resolve().parent.parent

# about one shape per path of the GPU module, with the longest K it uses (131073) and the ragged sizes around the seams
SHAPES = [(2051, 3, 257), (2048, 1, 255), (2111, 31, 65), (2049, 5, 1021), (2049, 9, 1027), (2049, 24, 4099), (17, 17, 16384),
          (33, 32, 16387), (40, 63, 16390), (65, 64, 16389), (30, 16, 20000), (20, 8, 50000), (3, 3, 65539), (16, 8, 70001),
          (10, 7, 131073), (3, 259, 23500), (8, 1031, 5821), (9, 515, 31100), (17, 4099, 3907), (5, 65539, 3), (16, 70001, 64),
          (1, 1, 65536), (1, 7, 1), (2, 2, 2)]
# np_sgemv: (rows, columns)
GEMV_SHAPES = [(262147, 7), (1027, 33), (1024, 256), (3, 65537), (16, 70003), (1, 65539), (300, 20001), (17, 260), (4, 8191), (1023, 257)]


def _same(a, b):
    return a.shape == b.shape and bool((gf.bits(a) == gf.bits(b)).all())


def _loop(A, B, order):
    """C in fp32, one rank-1 update per k, in the given order of k."""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for kk in order:
        acc += np.multiply.outer(A[:, kk], B[kk])          # fp32 products (exact) added in fp32
    return acc


def _chunked(A, B, length, backwards):
    """fp32 partial products of K-chunks of `length`, folded in fp32 forwards or backwards."""
    k = A.shape[1]
    parts = [A[:, c:c + length] @ B[c:c + length] for c in range(0, k, length)]
    acc = np.zeros_like(parts[0])
    for p in (reversed(parts) if backwards else parts):
        acc += p
    return acc


@pytest.mark.parametrize("mnk", SHAPES)
def test_every_summation_order_gives_the_integer_product(mnk, oracle):
    m, n, k = mnk
    amp = gf.amp_for(k)
    A, B = gf.operands(m, n, k, 3, amp, amp)
    assert A.dtype == B.dtype == np.float32 and (A != 0).all() and (B != 0).all() and np.abs(A).max() <= amp
    want = gf.expected(A, B)
    assert want.dtype == np.float32 and want.shape == (m, n)
    if m * n * k <= 1 << 24:
        assert _same(want, gf.expected_int64(A, B))                       # no floating point anywhere
    assert _same(want, A @ B)
    if m * n <= 1 << 12 or k <= 1024:
        assert _same(want, _loop(A, B, range(k))) and _same(want, _loop(A, B, range(k - 1, -1, -1)))
    for length in (7, 64, 4096):
        if m * n * (k // length + 1) <= 1 << 26:                           # (the partials of a wide C in chunks of 7 are GBs)
            assert _same(want, _chunked(A, B, length, False)) and _same(want, _chunked(A, B, length, True))
    assert _same(want, oracle.matmul(A, B))                               # OpenBLAS cblas_sgemm


@pytest.mark.parametrize("mn", GEMV_SHAPES)
def test_matrix_vector_products_the_same(mn, oracle):
    m, n = mn
    amp = gf.amp_for(n)
    A, _ = gf.operands(m, 1, n, 4, amp, amp)
    x = gf.vector(n, 5, amp)
    want = gf.expected(A, x)
    assert want.shape == (m,) and _same(want, A @ x) and _same(want, (A[:, ::-1] @ x[::-1]))
    assert _same(want, _chunked(A, x.reshape(n, 1), 4096, True)[:, 0]) and _same(want, _chunked(A, x.reshape(n, 1), 7, False)[:, 0])
    assert _same(want, oracle.matvec(A, x))                               # OpenBLAS cblas_sgemv


def test_family_refuses_what_is_not_exact():
    gf.operands(2, 2, 1 << 10, 1, 127, 129)                               # 2^10 . 127 . 129 = 2^24 - 2^10
    with pytest.raises(ValueError):
        gf.operands(2, 2, 1 << 10, 1, 128, 128)                           # 2^24 exactly
    with pytest.raises(ValueError):
        gf.operands(1, 1, 1 << 24, 1, 1, 1)
    with pytest.raises(ValueError):
        gf.operands(2, 2, 8, 1, 0, 1)
    with pytest.raises(ValueError):
        gf.vector(1 << 22, 1, 4)
    with pytest.raises(ValueError):
        gf.vector(8, 1, 0)
    with pytest.raises(ValueError):
        gf.expected(np.array([[1.5]], np.float32), np.array([[2.0]], np.float32))
    with pytest.raises(ValueError):
        gf.expected(np.array([[np.inf]], np.float32), np.array([[2.0]], np.float32))
    with pytest.raises(ValueError):
        gf.expected(np.full((1, 1 << 12), 64, np.float32), np.full((1 << 12, 1), 64, np.float32))      # 2^24
    with pytest.raises(ValueError):      # the sum is 0, the partial sums are not below 2^24: refused on |A| . |B|
        gf.expected(np.full((1, 1 << 13), 64, np.float32), np.tile(np.array([[64], [-64]], np.float32), (1 << 12, 1)))
    for k in (1, 77, 16384, 131073):
        a = gf.amp_for(k)
        assert k * a * a < gf.EXACT_LIMIT and (a == 64 or k * (a + 1) * (a + 1) >= gf.EXACT_LIMIT)


def test_k_seams():
    assert gf.k_seams(1) == [0] and gf.k_seams(5) == [0, 1, 2, 3, 4] and gf.k_seams(7) == [0, 1, 3, 4, 5, 6]
    s = set(gf.k_seams(16390))
    for unit in gf.SEAM_UNITS:
        for v in range(0, 16390, unit):
            assert {max(v - 1, 0), v, v + 1} <= s
    assert {0, 16386, 16387, 16388, 16389} <= s and 16382 not in s and min(s) == 0 and max(s) == 16389
    assert gf.k_seams(131073)[-1] == 131072 and len(gf.k_seams(131073)) > 90000


@pytest.mark.parametrize("mnk", [(5, 4, 64), (3, 3, 257), (17, 9, 1027), (1, 5, 33), (4, 1, 70)])
def test_specials_class_maps_against_fp64(mnk):
    """The class map comes from the planted positions; numpy's fp64 product of the same operands must show the same classes, and
    the finite elements must be the exact product of the operands with the planted NaN / Inf taken out."""
    m, n, k = mnk
    A, B = gf.operands(m, n, k, 9, 8, 8)
    base = gf.expected(A, B)
    seams = gf.k_seams(k)
    seen = set()
    for vector_form in (False, True) if n == 1 else (False,):
        Bv = B[:, 0].copy() if vector_form else B
        for ks, i, j in ((seams[0], 0, 0), (seams[-1], m - 1, n - 1), (seams[len(seams) // 2], m - 1, 0), (seams[1], 0, n - 1)):
            for kind in gf.SPECIAL_KINDS:
                A2, B2, cls, want = gf.specials(A, Bv, kind, ks, i, j, ks2=(ks + k // 2) % k, base=None if ks else gf.expected(A, Bv))
                with np.errstate(invalid="ignore", over="ignore"):
                    c64 = A2.astype(np.float64) @ B2.astype(np.float64)
                assert cls.shape == c64.shape == want.shape and (gf.classify(c64) == cls).all() and (gf.classify(want) == cls).all()
                fin = cls == gf.FINITE
                assert (want[fin] == c64[fin]).all()
                Bm = B2.reshape(k, -1)
                clean = gf.expected(np.where(np.isfinite(A2), A2, 0), np.where(np.isfinite(Bm), Bm, 0)).reshape(want.shape)
                assert (want[fin] == clean[fin]).all()
                untouched = fin & (np.arange(m) != i).reshape(-1, *([1] * (cls.ndim - 1)))
                if kind != gf.INF_MEETS_MINUS_INF:
                    assert (want[untouched] == base.reshape(want.shape)[untouched]).all()          # the other rows: the base product
                assert (A2 != A).sum() + (~np.isfinite(A2)).sum() <= 3 and (~np.isfinite(B2)).sum() <= 2
                seen.update(np.unique(cls).tolist())
                if kind == gf.INF_TIMES_ZERO:
                    assert (cls == gf.NAN).sum() == 1 and cls.reshape(m, -1)[i, j] == gf.NAN                # C[i, j] alone
                if kind == gf.INF_MEETS_MINUS_INF:
                    assert cls.reshape(m, -1)[i, j] == gf.NAN and (m == 1 or cls.reshape(m, -1)[(i + 1) % m, j] in (gf.PLUS_INF, gf.MINUS_INF))
    assert seen == ({gf.FINITE, gf.PLUS_INF, gf.MINUS_INF, gf.NAN} if m > 1 and n > 1 else seen) and gf.NAN in seen
    with pytest.raises(ValueError):
        gf.specials(A, B, gf.INF_MEETS_MINUS_INF, 3, 0, 0, ks2=3)


def test_frames():
    x = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    for off in range(4):
        image, start = gf.framed(x, off, pad=8)
        assert start == 8 + off and image.size == 12 + 16 + off and (image[start:start + 12] == x.reshape(-1)).all()
        assert np.isnan(image[:start]).all() and np.isnan(image[start + 12:]).all()
        image, start = gf.canary(12, off, pad=8)
        assert np.isnan(image[start:start + 12]).all() and gf.frame_intact(image, start, 12)
        for hit in (start - 1, start + 12, 0, image.size - 1):
            spoiled = image.copy()
            spoiled[hit] = 1.0
            assert not gf.frame_intact(spoiled, start, 12)
    with pytest.raises(ValueError):
        gf.framed(x, 4)
    with pytest.raises(ValueError):
        gf.framed(x, 0, pad=6)


def test_the_planner_bound_shapes_of_test_matmul_thin():
    """thin_to_planner(): a thin K-chunk launch of fewer than q / 4 workgroups per CU goes to the planner; at the default q = 59
    on 256 CUs that is anything under 59 . 256 / 4 = 3776 workgroups.  The K-chunk plans of launch_thin_nv (target = 8 . 256 =
    2048 workgroups; twice that many K-chunks at most, each at least 2048 long and a multiple of 64) for the shapes
    test_gpu_parity.py::test_matmul_thin lists under "17 <= M < 2048 against a very long K":
      (784, 10, 200000)  13 blocks of 64 rows; min(ceil(4096 / 13), 200000 / 2048) = 97 chunks -> 2112 long -> 95: 13 . 95 = 1235
      (500, 5, 30001)    8 blocks; min(512, 14) = 14 chunks of 2176: 8 . 14 = 112
      (100, 17, 16384)   1 block of 128 rows; min(4096, 8) = 8 chunks of 2048: 8
      (2047, 3, 20000)   32 blocks; min(128, 9) = 9 chunks of 2240: 32 . 9 = 288
    and of sgemm_fewrows_splitk_kernel (one or two 32-row tiles; wave-chunks of >= 1024, four to a workgroup):
      (17, 32, 100000)   1 tile, min(16384, 97) = 97 wave-chunks of 1056 -> 95 -> 24 groups: 24
      (32, 64, 300000)   1 tile, min(16384, 292) = 292 wave-chunks of 1056 -> 285 -> 72 groups ... the issue's 73 counts 1028-long
                         chunks before rounding to 32; either way far below 3776
    All below 3776: each goes to the planner, and only np_sgemm_set_variant(-(40 + 0)) brings the K-chunked kernels back."""
    assert 59 * 256 // 4 == 3776
    for mnk, workgroups in (((784, 10, 200000), 1235), ((500, 5, 30001), 112), ((100, 17, 16384), 8), ((2047, 3, 20000), 288),
                            ((17, 32, 100000), 24)):
        assert gf.thin_chunks(*mnk)[1] == workgroups, (mnk, gf.thin_chunks(*mnk))
        assert gf.path(*mnk) == gf.TILED and gf.path(*mnk, q=0) == gf.thin_chunks(*mnk)[0] | gf.FOLD
    assert gf.thin_chunks(32, 64, 300000)[1] < 100 and gf.path(32, 64, 300000) == gf.TILED
    # the other shapes of that list: every one to the planner by default, every one a K-chunked kernel with q = 0
    for mnk in ((300, 16, 65537), (64, 64, 100001), (100, 33, 20000), (2047, 50, 16384), (40, 63, 70000), (20, 8, 50000), (30, 16, 20000),
                (32, 32, 65536), (33, 20, 40000), (48, 12, 30000)):
        assert gf.thin_chunks(*mnk)[1] < 3776 and gf.path(*mnk) == gf.TILED and gf.path(*mnk, q=0) & gf.FOLD
    # the smallest K at which the default reaches them again: 2048 rows short of one, N <= 16 (32 blocks of 64 rows, 128 chunks)
    assert gf.path(2047, 16, 2048 * 117) == gf.TILED and gf.path(2047, 16, 2048 * 118) == gf.THIN_MFMA16 | gf.THIN_K_CHUNKS | gf.FOLD
    # ... a hundred rows (2 blocks, at most 2048 chunks of at least 2048) from 1888 chunks: K ~ 3.9e6
    assert gf.path(100, 16, 1887 * 2048) == gf.TILED and gf.path(100, 16, 1888 * 2048) == gf.THIN_MFMA16 | gf.THIN_K_CHUNKS | gf.FOLD
    # ... and one 32-row tile of sgemm_fewrows_splitk_kernel (four wave-chunks of >= 1024 to a workgroup) from K = 3776 . 4096 ~ 1.5e7
    assert gf.path(32, 32, 3775 * 4096) == gf.TILED and gf.path(32, 32, 3776 * 4096) == gf.FEWROWS_SPLITK1 | gf.FOLD
    assert gf.path(32, 64, 3775 * 4096) == gf.TILED and gf.path(32, 64, 3776 * 4096) == gf.FEWROWS_SPLITK2 | gf.FOLD


def test_the_masks_the_gpu_module_names_follow_from_the_dispatcher():
    from tests import test_gpu_gemm_exact as g
    for mnk, mask in g.BELOW_2048:
        assert gf.path(*mnk, q=0) == mask and gf.path(*mnk) == gf.TILED, mnk
        assert g.SPECIALS_BELOW_2048.get(mnk, 4) in gf.k_seams(mnk[2])
        if mnk in g.SPECIALS_BELOW_2048:
            assert g.SPECIALS_BELOW_2048[mnk] in (gf.thin_chunks(*mnk)[3], gf.thin_chunks(*mnk)[3] - 1)      # on that kernel's chunk edge
    assert gf.path(2049, 3, 1027) == gf.THIN_MFMA16 | gf.THIN_K_CHUNKS | gf.FOLD          # N <= 4 on the MFMA kernel: always K-chunked
    assert gf.path(65537, 4, 1024) == gf.THIN_LANES | gf.LANES(64) and gf.path(65535, 4, 1024) == gf.THIN_MFMA16 | gf.THIN_K_CHUNKS | gf.FOLD
    assert gf.path(32, 32771, 512) == gf.SKINNY and gf.path(32, 4100, 3903) == gf.SKINNY | gf.FOLD and gf.path(33, 4100, 3903) == gf.TILED
    assert gf.path(8, 70001, 64) == gf.THIN_LEFT | gf.MV(8) and gf.path(8, 70001, 65) == gf.TILED
    assert gf.path(2048, 1, 255) == gf.THIN_LANES | gf.LANES(32) and gf.path(2048, 1, 256) == gf.GEMV_SHORT_ROWS | gf.LANES(32)
    assert gf.path(2048, 1, 1024) == gf.GEMV_WAVE | gf.GEMV_WAVE_VEC and gf.path(2048, 1, 1024, aligned=False) == gf.GEMV_WAVE
    assert gf.gemv_path(262144, 4) == gf.GEMV_STAGED and gf.gemv_path(262143, 4) == gf.GEMV_SHORT_ROWS | gf.LANES(1)
    assert gf.gemv_path(262144, 64) == gf.GEMV_SHORT_ROWS | gf.LANES(8) and gf.gemv_path(262144, 3) == gf.GEMV_SHORT_ROWS | gf.LANES(1)
    assert gf.gemv_path(1023, 256) == gf.GEMV_WAVE | gf.GEMV_WAVE_VEC and gf.gemv_path(17, 65536) == gf.GEMV_CHUNKS | gf.FOLD
    assert gf.gemv_path(1, 16383) == gf.GEMV_WAVE and gf.gemv_path(1, 65536) == gf.GEMV_CHUNKS | gf.FOLD
    assert gf.describe(gf.FEWROWS | gf.MV(4) | gf.FOLD) == "FEWROWS|FOLD|MV=4" and gf.describe(0) == "0"


def test_sgemm_probe_is_declared_exported_and_prototyped():
    from numpower_amd import _lib
    header = (ROOT / "include" / "np_hip_debug.h").read_text()
    lib = _lib.load()
    name = "np_sgemm_debug_last_path"
    assert "int %s(unsigned *host_mask);" % name in header and hasattr(lib, name) and name in _lib.PROTOTYPES
    assert name not in (ROOT / "include" / "np_hip.h").read_text()
    defines = dict(re.findall(r"#define NP_SGEMM_PATH_(\w+) (0x[0-9a-f]+)u", header))
    assert {k: int(v, 16) for k, v in defines.items()} == gf.PATH_BITS                   # one bit each, the family's copy agrees
    assert len(set(gf.PATH_BITS.values())) == 20 and all(v & (v - 1) == 0 and v < 1 << 20 for v in gf.PATH_BITS.values())
    assert "#define NP_SGEMM_PATH_LANES(L) ((unsigned)(__builtin_ctz((unsigned)(L)) + 1) << 20)" in header
    assert "#define NP_SGEMM_PATH_MV(MV) ((unsigned)(__builtin_ctz((unsigned)(MV)) + 1) << 24)" in header
    assert [gf.LANES(1 << e) >> 20 for e in range(7)] == list(range(1, 8)) and [gf.MV(1 << e) >> 24 for e in range(5)] == list(range(1, 6))
    # without a device, before any product: a null pointer is refused, the mask reads 0
    assert lib.np_sgemm_debug_last_path(None) != 0
    mask = C.c_uint(0xffffffff)
    assert lib.np_sgemm_debug_last_path(C.byref(mask)) == 0 and mask.value == 0


# ---- the tiled kernels: tests/test_gpu_gemm_tiled_exact.py without a device --------------------------------------------------------------
def _tiled_expectations():
    """(case, offsets, records, mask) for every case of the GPU module at (0, 0) and (3, 3), under the case's own setters (the
    planner-chosen ones ask np_sgemm_debug_plan, which reads them)."""
    from numpower_amd import _lib
    from tests import test_gpu_gemm_tiled_exact as t
    from tests.gemm_exact import VARIANT_DEFAULTS
    lib = _lib.load()
    out = []
    for c in t.all_cases():
        try:
            for code in t.codes_of(c):
                assert lib.np_sgemm_set_variant(code) == 0, (c, code)
            for off in ((0, 0),) if c.get("offsets") == "aligned" else ((0, 0), (3, 3)):
                records, mask = t.expectation(c, lib, *off)
                out.append((c, off, records, mask))
        finally:
            for code in VARIANT_DEFAULTS:
                assert lib.np_sgemm_set_variant(code) == 0
    return out


def test_the_records_the_tiled_gpu_module_names_follow_from_the_launchers():
    from tests import test_gpu_gemm_tiled_exact as t
    keep = gf.F_VEC | gf.F_EDGE | gf.F_KTAIL | gf.F_PRIO | gf.F_BUF
    seen = set()
    for c, off, records, mask in _tiled_expectations():
        assert 1 <= len(records) <= gf.LAUNCH_KEPT and mask in (0, gf.TILED, gf.TILED | gf.FOLD), c
        if "flags" in c and off == (0, 0):
            assert records[0].flags & keep == c["flags"], (c, records)
        if off == (3, 3) and c["kind"] != "padded":
            assert not any(r.flags & (gf.F_VEC | gf.F_BUF) for r in records), (c, records)       # no float4 rows, no buffer loop off 16 bytes
        if "seam" in c:
            assert c["seam"] in gf.k_seams(c["k"])
            if c["kind"] == "streamk":       # on a range edge of the kernel's own floor(iters . w / G) split, inside a tile
                starts, nk = gf.streamk_range_starts(c["m"], c["n"], c["k"], records[0].grid_x)
                assert c["seam"] % 16 == 0 and c["seam"] // 16 in {s % nk for s in starts if s % nk}, (c, starts[:4])
        if c["kind"] == "kq_chunks" and not c.get("refused"):
            assert mask == gf.TILED | gf.FOLD and records[-1].k_last >= 4 and records[-1].grid_x * records[-1].grid_z % c["S"] == 0, (c, records)
            major = c.get("knobs", {}).get("chunk_major", True)
            assert bool(records[-1].flags & gf.F_CHUNK_MAJOR) == major and (records[-1].s == c["S"]) == major
        seen.update(r.instantiation() for r in records)
    T, E, KT, P, BF, SUB, M1 = gf.F_VEC, gf.F_EDGE, gf.F_KTAIL, gf.F_PRIO, gf.F_BUF, gf.F_SUB, gf.F_PIPE_MODE1
    # sgemm_dma_kernel / sgemm_streamk_kernel <EDGE, KTAIL, PRIO, BUF>: the 8 of each (VEC is no template argument of theirs)
    eight = {E | KT, E | BF, E, KT, P | BF, P, BF, 0}
    for family in (gf.K_DMA, gf.K_STREAMK):
        assert {i[5] & ~T for i in seen if i[0] == family} == eight, family
    # sgemm_dmas_kernel: 5 tile shapes x EDGE x KTAIL, and every S
    assert {(i[4], i[5]) for i in seen if i[0] == gf.K_DMAS} >= {(s, f) for s in (0, 1, 2, 3, 5) for f in (0, E, KT, E | KT)}
    # sgemm_kq_kernel: 7 shapes x (VEC, VEC | EDGE, EDGE)
    assert {(i[4], i[5]) for i in seen if i[0] == gf.K_KQ} == {(s, f) for s in range(7) for f in (T, T | E, E)}
    # the register-staged tiles: 4 launch_sgemm_tile forms (two share <128, 128, 16> and differ in MINW) and the two pipe modes x 3
    assert {(i[1], i[3], i[5]) for i in seen if i[0] == gf.K_TILE} == {(b, k, f) for b, k in ((128, 16), (128, 32), (64, 16)) for f in (T, T | E, E)}
    assert {i[5] for i in seen if i[0] == gf.K_PIPE} == {f | m for f in (T, T | E, E) for m in (0, M1)}
    assert {i[5] for i in seen if i[0] == gf.K_TILE_SUB} == {f | SUB for f in (T, T | E, E)} and any(i[0] == gf.K_PAD_COPY for i in seen)
    # every S of the mid tiles, as launched
    by_shape = {}
    for c, off, records, mask in _tiled_expectations():
        for r in records:
            if r.family == gf.K_DMAS:
                by_shape.setdefault(r.shape, set()).add(r.s)
    assert by_shape[0] == {1, 2, 4, 8, 16} and by_shape[3] == {1, 2, 4, 8, 16} and by_shape[1] == {1, 2, 4, 8} and by_shape[2] >= {2, 4} and by_shape[5] >= {1}
    # a forced K-chunk plan wants a remainder of at least 4: shorter ones never reach launch_kq
    assert gf.tiled_launches("kq_chunks", 33, 35, 1281, shape=1, S=5) is None and gf.tiled_launches("kq_chunks", 48, 48, 1923, shape=0, S=7) is None


def test_launcher_arithmetic_by_hand():
    """A few records worked out by hand from np_sgemm.hip."""
    L = gf.Launch
    T, E, KT, P, BF = gf.F_VEC, gf.F_EDGE, gf.F_KTAIL, gf.F_PRIO, gf.F_BUF
    kn7 = gf.Knobs(variant=7)
    assert gf.tiled_launches("dma", 257, 130, 50, knobs=kn7) == ([L(gf.K_DMA, 256, 128, 16, -1, E | KT, 1, 4, 1, 0)], False)
    assert gf.tiled_launches("dma", 4096, 4096, 4096) == ([L(gf.K_DMA, 256, 128, 16, -1, T | P | BF | gf.F_SWIZZLE, 1, 512, 1, 0)], False)
    assert gf.tiled_launches("dma", 200, 3, 50, knobs=kn7)[0][0].family == gf.K_PIPE
    # stream-K: 4 tiles x 1537 K-tiles = 6148 on 256 workgroups (512 would leave ranges of 13 < 24)
    assert gf.streamk_range_starts(512, 256, 24592, 256)[0][:3] == [0, 24, 48] and gf.streamk_range_starts(512, 256, 24592, 256)[0][64] == 1537
    assert gf.streamk_grid(512, 256, 24592) == 256 and gf.streamk_grid(768, 384, 208) == 0 and gf.streamk_grid(513, 257, 11008) == 256
    assert gf.tiled_launches("streamk", 512, 256, 24592) == ([L(gf.K_STREAMK, 256, 128, 16, -1, P, 1, 256, 1, 0)], False)
    # launch_dmas: the clamp loop (77 x 65 x 130 from S = 16: chunks of 16, 32, 48 are under 64; S = 2, Kc = 80) and residency
    assert gf.dmas_plan(0, 77, 65, 130, 1, 16) == (2, 80, 1) and gf.dmas_plan(2, 768, 768, 256, 1, 4) is None
    assert gf.dmas_plan(0, 129, 130, 1025, 1, 16) == (8, 144, 4) and gf.dmas_plan(4, 64, 64, 64, 1, 1) is None
    assert gf.tiled_launches("dmas", 129, 130, 65, shape=2, S=1)[0][0].shape == 5            # ragged, whole K: eight waves
    assert gf.tiled_launches("dmas", 64, 64, 64, shape=2, S=1)[0][0].shape == 2
    # launch_plan: 33 x 35 x 2049 in 5 chunks of 448, remainder 257, 2 x 2 tiles of 32 x 32
    records, folded = gf.tiled_launches("kq_chunks", 33, 35, 2049, shape=1, S=5)
    assert folded and records == [L(gf.K_KQ, 32, 32, 64, 1, E | gf.F_CHUNK_MAJOR, 5, 20, 1, 257)]
    records, _ = gf.tiled_launches("kq_chunks", 33, 35, 2049, shape=1, S=5, knobs=gf.Knobs(chunk_major=False))
    assert records == [L(gf.K_KQ, 32, 32, 64, 1, E, 1, 4, 5, 257)]
    assert gf.split_chunk_length(0, 2052, 2) == 1040 and gf.split_chunk_length(6, 10000, 8) == 1280
    words = [5, 128 | 64 << 16, 32 | 2 << 16, E | KT, 4, 24, 3, 0]
    assert L.decode(words) == L(gf.K_DMAS, 128, 64, 32, 1, E | KT, 4, 24, 3, 0) and "DMAS(128x64x32 shape 1, EDGE|KTAIL, S 4" in repr(L.decode(words))


def test_split_k_plans_pinned():
    """With the mid and k-quartered plans off (-14, -20, -22) cfg 0 .. 2 plan alone.  The smallest square-ish shapes whose plan
    splits every tile row with a remainder chunk, and one that splits only a tail of rows, as the GPU module uses them."""
    from numpower_amd import _lib
    from tests import test_gpu_gemm_tiled_exact as t
    from tests.gemm_exact import VARIANT_DEFAULTS
    lib = _lib.load()
    try:
        for code in t.SPLITK_CODES:
            assert lib.np_sgemm_set_variant(code) == 0
        pinned = {(64, 64, 516): (2, 1, 4, 144, 84), (128, 128, 2052): None, (1216, 1728, 1028): (2, 1, 8, 144, 20)}
        for c in t.SPLITK_ALL_ROWS + t.SPLITK_TAIL_ROWS:
            cfg, tail_rows, chunks, streamk = t.plan_of(lib, c["m"], c["n"], c["k"], 1)
            rows = -(-c["m"] // gf.CFG_TILES[cfg][0])
            Kc = gf.split_chunk_length(cfg, c["k"], chunks)
            assert not streamk and cfg <= 2 and chunks >= 2 and c["k"] % Kc, (c, cfg, tail_rows, chunks)
            if pinned[c["m"], c["n"], c["k"]]:
                assert (cfg, tail_rows, chunks, Kc, c["k"] % Kc) == pinned[c["m"], c["n"], c["k"]]
            records, mask = t.expectation(c, lib)
            assert mask == gf.TILED | gf.FOLD and records[-1].k_last == c["k"] % Kc and records[-1].grid_z == chunks
            if c in t.SPLITK_ALL_ROWS:
                assert tail_rows == rows and len(records) == 1
            else:
                assert 0 < tail_rows < rows and len(records) == 2 and records[0].grid_z == 1 and records[0].k_last == 0
    finally:
        for code in VARIANT_DEFAULTS:
            assert lib.np_sgemm_set_variant(code) == 0


def test_subtracting_expectation_against_int64():
    for m, n, k in ((5, 4, 64), (129, 127, 17), (200, 72, 64)):
        A, B = gf.operands(m, n, k, 3, 64, 64)
        c0 = np.random.default_rng(1).integers(-1000, 1001, size=(m, n)).astype(np.float32)
        want = gf.expected_sub(c0, A, B)
        exact = c0.astype(np.int64) - A.astype(np.int64) @ B.astype(np.int64)
        assert want.dtype == np.float32 and (want.astype(np.int64) == exact).all() and np.abs(exact).max() < gf.EXACT_LIMIT
        acc = c0.copy()                                                    # a subtraction per step, in fp32: the same bits
        for kk in range(k):
            acc -= np.multiply.outer(A[:, kk], B[kk])
        assert _same(acc, want) and _same(c0 - A @ B, want)
    with pytest.raises(ValueError):
        gf.expected_sub(np.full((1, 1), 2.0 ** 24 - 4, np.float32), np.full((1, 1), 2, np.float32), np.full((1, 1), 2, np.float32))
    with pytest.raises(ValueError):
        gf.expected_sub(np.full((1, 1), 0.5, np.float32), np.ones((1, 1), np.float32), np.ones((1, 1), np.float32))


def test_launch_probe_is_declared_exported_and_prototyped():
    from numpower_amd import _lib
    header = (ROOT / "include" / "np_hip_debug.h").read_text()
    lib = _lib.load()
    assert "int np_sgemm_debug_last_launches(unsigned *host_records, unsigned capacity, unsigned *host_count);" in header
    assert "int np_sgemm_debug_sub_ld(size_t M, size_t N, size_t K, const float *A, size_t lda, const float *B, size_t ldb, float *C, size_t ldc);" in header
    assert "int np_sgemm_debug_plan_unaligned(size_t M, size_t N, size_t K, int cus, double *out);" in header
    for name in ("np_sgemm_debug_last_launches", "np_sgemm_debug_sub_ld", "np_sgemm_debug_plan_unaligned"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and name not in (ROOT / "include" / "np_hip.h").read_text()
    kernels = {k: int(v) for k, v in re.findall(r"#define NP_SGEMM_KERNEL_(\w+) (\d+)u", header)}
    flags = {k: int(v, 16) for k, v in re.findall(r"#define NP_SGEMM_LAUNCH_F_(\w+) (0x[0-9a-f]+)u", header)}
    assert kernels == gf.KERNELS and flags == gf.LAUNCH_FLAGS
    assert "#define NP_SGEMM_LAUNCH_WORDS %du" % gf.LAUNCH_WORDS in header and "#define NP_SGEMM_LAUNCH_KEPT %du" % gf.LAUNCH_KEPT in header
    assert gf.LAUNCH_KEPT >= 8
    words = dict(re.findall(r"#define NP_SGEMM_LAUNCH_(FAMILY|TILE|BK|FLAGS|S|GRID_X|GRID_Z|K_LAST) (\d)\n", header))
    assert [int(words[w]) for w in ("FAMILY", "TILE", "BK", "FLAGS", "S", "GRID_X", "GRID_Z", "K_LAST")] == list(range(8))
    # without a device, before any product: null pointers are refused, no launch is recorded; the wrapper checks its arguments
    count = C.c_uint(77)
    assert lib.np_sgemm_debug_last_launches(None, 0, None) != 0 and lib.np_sgemm_debug_last_launches(None, 4, C.byref(count)) != 0
    assert lib.np_sgemm_debug_last_launches(None, 0, C.byref(count)) == 0 and count.value == 0
    assert lib.np_sgemm_debug_sub_ld(0, 4, 4, None, 4, None, 4, None, 4) != 0 and lib.np_sgemm_debug_sub_ld(4, 4, 4, 16, 3, 16, 4, 16, 4) != 0
