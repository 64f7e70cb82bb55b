"""Everything behind launch_sgemm_ld (np_sgemm.hip) against the exact family (tests/gemm_family.py): the 256 x 128 LDS-DMA kernel
and its stream-K form, the mid tiles (sgemm_dmas_kernel), the k-quartered tiles (sgemm_kq_kernel), the register-staged tiles,
pad_copy_kernel, the split-K plans with their remainder chunk, and the subtracting epilogue of np::sgemm_sub_ld.

The discipline of tests/test_gpu_gemm_exact.py (tests/gemm_exact.py: run_tiled): integer operands at float offsets inside NaN, C
inside a -777 canary with a NaN interior — row gaps of a window and the gaps between the matrices of a batch included — every
float of C's buffer compared bit for bit, twice, a clean np_sync, and the WHOLE list of launch records of
np_sgemm_debug_last_launches: kernel, tile, template arguments, S, grid, K_last.  A forced case whose launcher declines runs
another kernel, shows other records and fails.

The cases are data (the tables below); what each must launch comes from gemm_family.tiled_launches, the launchers' host
arithmetic restated — and, where the planner chooses, from np_sgemm_debug_plan.  tests/test_gemm_reference_cpu.py walks the same
tables without a device: the literal flags named here against that arithmetic, and that every instantiation is reached.

For one product whose rows are not float4-loadable the planner also weighs padded copies: np_sgemm_debug_plan_unaligned reports
that decision with the plan, and the planner-chosen cases at offsets (3, 3) take their expectation from it.  Forced stream-K
(-4) cannot be kept from those copies, so its cases other than the aligned 512 x 256 x 24592 run on a window of B (ldb = N + 4):
a window is never padded.  Records are written for 256 CUs."""
import ctypes as C

import numpy as np
import pytest

from numpower_amd import _lib
from tests import gemm_family as gf
from tests.gemm_exact import ALL_OFFSETS, DIAGONAL, Dev, run_tiled, variants
from tests.gemm_family import F_BUF, F_EDGE, F_KTAIL, F_PRIO, F_VEC

pytestmark = pytest.mark.gpu

ALIGNED = ((0, 0),)


@pytest.fixture(scope="module")
def dev(hip):
    return Dev(hip)


def case(kind, m, n, k, **kw):
    """One product call.  batch, gaps (floats between the matrices of A, B, C), ld (lda - K, ldb - N, ldc - N: a window), offsets,
    knobs (gemm_family.Knobs: which setters differ from their defaults), shape / S / variant for the forced forms, codes (setters
    the kind does not imply), flags (the literal template-argument flags of the first record at offsets (0, 0)), refused (the
    forced launcher must decline: the planner's choice runs instead), seam (run every specials() kind there too)."""
    return dict(kind=kind, m=m, n=n, k=k, **kw)


def codes_of(c):
    """The np_sgemm_set_variant codes of a case, in the order they are set."""
    kn, kind = c.get("knobs", {}), c["kind"]
    codes = list(c.get("codes", ()))
    if "kloop" in kn:
        codes.append({0: -31, 1: -33, 2: -32}[kn["kloop"]])
    if "prio_period" in kn:
        codes.append(-(100 + kn["prio_period"]))
    if kn.get("chunk_major") is False:
        codes.append(-25)
    if kind == "dma":
        codes.append(kn.get("variant", 7))
    elif kind == "tile":
        codes.append(c["variant"])
    elif kind == "streamk":
        codes.append(-4)
    elif kind == "dmas":
        codes.append(-(1000 + 100 * c["shape"] + c["S"]))
    elif kind == "kq":
        codes.append(-(2000 + c["shape"]))
    elif kind == "kq_chunks":
        codes.append(-(30000 + 1000 * c["shape"] + c["S"]))
    elif kind == "padded":
        codes += [-6, -3]
    return codes


def geometry(c):
    m, n, k, batch = c["m"], c["n"], c["k"], c.get("batch", 1)
    dl, gaps = c.get("ld", (0, 0, 0)), c.get("gaps", (0, 0, 0))
    lda, ldb, ldc = k + dl[0], n + dl[1], n + dl[2]
    return m, n, k, batch, lda, ldb, ldc, gaps


def plan_of(lib, m, n, k, batch, vec=None):
    """(cfg, tail_rows, S, stream-K taken) of the planner for 256 CUs under the setters in force.  vec: whether the rows are
    float4-loadable (None: K % 4 == N % 4 == 0, aligned operands).  One product whose rows are not is asked of
    np_sgemm_debug_plan_unaligned, which also says whether padded copies would run instead: such a shape is no case of this module."""
    dense_vec = k % 4 == 0 and n % 4 == 0
    vec = dense_vec if vec is None else vec
    if batch == 1 and not vec:
        out = (C.c_double * 5)()
        _lib.check(lib.np_sgemm_debug_plan_unaligned(m, n, k, 256, out))
        assert not out[4], "%s: the planner takes padded copies" % ((m, n, k),)
        return int(out[0]), int(out[1]), int(out[2]), bool(out[3])
    assert vec == dense_vec, "%s batch %d: np_sgemm_debug_plan plans for float4-loadable rows" % ((m, n, k), batch)
    out = (C.c_double * 11)()
    _lib.check(lib.np_sgemm_debug_plan(m, n, k, batch, 256, out))
    return int(out[0]), int(out[1]), int(out[2]), bool(out[4])


def expectation(c, lib, oa=0, ob=0):
    """(records, mask) one call of the case must leave at offsets (oa, ob).  lib: for the planner-chosen cases (host arithmetic: the
    setters of the case must be in force)."""
    m, n, k, batch, lda, ldb, ldc, gaps = geometry(c)
    kn = dict(c.get("knobs", {}))
    if c["kind"] in ("dma", "tile"):
        kn.setdefault("variant", c.get("variant", 7))
    common = dict(batch=batch, lda=lda, ldb=ldb, ldc=ldc, sa=(m * lda + gaps[0]) if batch > 1 else 0, sb=(k * ldb + gaps[1]) if batch > 1 else 0,
                  a_aligned=oa == 0, b_aligned=ob == 0, knobs=gf.Knobs(**kn))
    kind = c["kind"]
    got = None if kind == "plan" else gf.tiled_launches(kind, m, n, k, shape=c.get("shape"), S=c.get("S", 1), variant=c.get("variant"), **common)
    assert (got is None) == (kind == "plan" or bool(c.get("refused"))), "%r: the forced launcher %s" % (c, "declines" if got is None else "takes the shape")
    if got is None:
        assert (lda, ldb, ldc) == (k, n, n)
        vec = k % 4 == 0 and n % 4 == 0 and (oa, ob) == (0, 0)
        got = gf.tiled_launches("plan", m, n, k, plan=plan_of(lib, m, n, k, batch, vec), **common)
    records, folded = got
    if kind == "sub":
        return records, 0
    return records, gf.TILED | (gf.FOLD if folded else 0)


def operands_of(c, seed=7):
    m, n, k, batch = c["m"], c["n"], c["k"], c.get("batch", 1)
    amp = gf.amp_for(k)
    if batch == 1:
        return gf.operands(m, n, k, seed, amp, amp)
    pairs = [gf.operands(m, n, k, seed + b, amp, amp) for b in range(batch)]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def expected_of(A, B):
    return gf.expected(A, B) if A.ndim == 2 else np.stack([gf.expected(a, b) for a, b in zip(A, B)])


def execute(dev, c, label=""):
    """One case, under its setters: every offset pair, then every special at the case's seam."""
    m, n, k, batch, lda, ldb, ldc, gaps = geometry(c)
    window = (lda, ldb, ldc) != (k, n, n)
    offsets = {"all": ALL_OFFSETS, "diagonal": DIAGONAL, "aligned": ALIGNED}[c.get("offsets", "diagonal")]
    A, B = operands_of(c)
    want = expected_of(A, B)
    with variants(dev, *codes_of(c)):
        at = {off: expectation(c, dev.L, *off) for off in offsets}
        masks = {mask for _, mask in at.values()}
        assert len(masks) == 1
        if "flags" in c:
            first = at[0, 0][0][0]
            assert first.flags & (F_VEC | F_EDGE | F_KTAIL | F_PRIO | F_BUF) == c["flags"], "%r: the arithmetic gives %r" % (c, first)
        ld = dict(lda=lda, ldb=ldb, ldc=ldc) if window else {}
        run_tiled(dev, A, B, want, lambda oa, ob: at[oa, ob][0], offsets, masks.pop(), gaps=gaps, label="%s %s" % (label, c["kind"]), **ld)
        if "seam" in c:
            seams = gf.k_seams(k)
            assert c["seam"] in seams and 0 < c["seam"] < k - 1 and batch == 1
            records, mask = at[0, 0]
            for ks, i, j in ((seams[0], 0, 0), (seams[-1], m - 1, n - 1), (c["seam"], m - 1, 0)):
                for kind in gf.SPECIAL_KINDS:
                    A2, B2, cls, want2 = gf.specials(A, B, kind, ks, i, j, ks2=(ks + k // 2) % k, base=want)
                    run_tiled(dev, A2, B2, want2, records, ALIGNED, mask, cls=cls, label="%s special %d at k = %d" % (label, kind, ks), **ld)


# ---- sgemm_dma_kernel<EDGE, KTAIL, PRIO, BUF>: np_sgemm_set_variant(7), (47) with the swizzle -----------------------------------------
# every instantiation, with the flags it must show
DMA_INSTANTIATIONS = [
    case("dma", 257, 129, 50, flags=F_EDGE | F_KTAIL),
    case("dma", 257, 132, 48, flags=F_VEC | F_EDGE | F_BUF, knobs=dict(kloop=2)),
    case("dma", 257, 132, 48, flags=F_VEC | F_EDGE),
    case("dma", 256, 128, 50, flags=F_KTAIL),
    case("dma", 256, 128, 2048, flags=F_VEC | F_PRIO | F_BUF),                                 # PRIO and BUF by default from K = 2048
    case("dma", 256, 128, 80, flags=F_VEC | F_PRIO | F_BUF, knobs=dict(prio_period=4)),
    case("dma", 256, 128, 80, flags=F_VEC | F_PRIO, knobs=dict(prio_period=4, kloop=0)),
    case("dma", 256, 128, 2048, flags=F_VEC | F_PRIO, knobs=dict(kloop=0)),
    case("dma", 256, 128, 80, flags=F_VEC | F_BUF, knobs=dict(prio_period=0, kloop=2)),
    case("dma", 256, 128, 2048, flags=F_VEC, knobs=dict(prio_period=0)),
    case("dma", 256, 128, 80, flags=F_VEC),
]
DMA_K = [case("dma", 256, 128, k, offsets="all" if k == 49 else "diagonal") for k in (4, 5, 7, 15, 16, 17, 31, 33, 47, 48, 49, 80, 81, 272)]
DMA_MN = [case("dma", m, n, k) for m, n in ((1, 4), (255, 127), (257, 129), (257, 130), (300, 131), (512, 256), (513, 260)) for k in (48, 50)]
DMA_RESIDUES = [case("dma", 257, 128 + dn, 48 + dk) for dn in range(4) for dk in range(4)]
DMA_SPECIALS = [case("dma", 257, 130, 50, offsets="aligned", seam=48)]                        # the last K-tile: zero_tail
DMA_SWIZZLE = [case("dma", 2305, 259, 32, knobs=dict(variant=47)), case("dma", 2048, 384, 16, knobs=dict(variant=47))]
DMA_BATCH = [case("dma", 256, 128, 48, batch=3, gaps=(8, 8, 8), knobs=dict(kloop=2), flags=F_VEC | F_BUF, offsets="aligned"),
             case("dma", 256, 128, 48, batch=3, gaps=(5, 6, 7), knobs=dict(kloop=2), flags=0, offsets="aligned"),
             case("dma", 257, 130, 50, batch=3, gaps=(8, 4, 12)), case("dma", 257, 130, 50, batch=3, gaps=(1, 2, 3))]
DMA_WINDOWS = [case("dma", m, n, k, ld=ld) for m, n, k in ((300, 131, 50), (512, 256, 48)) for ld in ((4, 8, 4), (1, 3, 1))]


@pytest.mark.parametrize("table", ["DMA_INSTANTIATIONS", "DMA_K", "DMA_MN", "DMA_RESIDUES", "DMA_SPECIALS", "DMA_SWIZZLE", "DMA_BATCH", "DMA_WINDOWS"])
def test_lds_dma_256x128(table, dev):
    """K across the 16-deep K-tile and the float4 that zero_tail cuts, ragged M / N whose clamped rows and columns must reach no
    stored element, all N % 4 x K % 4 residues, all 8 instantiations, the swizzled tile order with a ragged last band and
    nwg % 8 != 0 (every tile written exactly once: the NaN interior and the canary), batches with gaps, windows."""
    for c in globals()[table]:
        execute(dev, c, table)


# ---- sgemm_streamk_kernel: (-4) ---------------------------------------------------------------------------------------------------------
WINDOW_OF_B = (0, 4, 0)
STREAMK = [
    case("streamk", 512, 256, 24592, flags=F_PRIO, offsets="aligned", seam=384),               # workgroup 1 starts at K-tile 6148 . 1 // 256 = 24: a range edge
    case("streamk", 512, 256, 24592, flags=F_PRIO, ld=WINDOW_OF_B),
    case("streamk", 512, 256, 24597, flags=F_KTAIL, ld=WINDOW_OF_B),
    case("streamk", 500, 250, 24592, flags=F_EDGE | F_KTAIL, ld=WINDOW_OF_B),
    case("streamk", 500, 252, 24592, flags=F_EDGE, ld=WINDOW_OF_B),
    case("streamk", 513, 257, 11008, flags=F_EDGE | F_KTAIL, ld=WINDOW_OF_B, offsets="all"),   # nine ragged tiles on 256 workgroups
    case("streamk", 500, 252, 24592, flags=F_EDGE | F_BUF, ld=WINDOW_OF_B, knobs=dict(kloop=2), offsets="aligned"),
    case("streamk", 512, 256, 24592, flags=F_PRIO | F_BUF, knobs=dict(kloop=2), offsets="aligned"),
    case("streamk", 512, 256, 24592, flags=F_BUF, knobs=dict(kloop=2, prio_period=0), offsets="aligned"),
    case("streamk", 512, 256, 24592, flags=0, knobs=dict(prio_period=0), offsets="aligned"),
]


@pytest.mark.parametrize("index", range(len(STREAMK)))
def test_stream_k(index, dev):
    """Ranges that straddle tiles: every shape asserts from the record's grid that ceil(iters / G) is no multiple of the K-tile
    count, so at least one tile is split between workgroups.  A second, different shape runs directly behind the first (and
    the first again behind that): the finishers put every flag back to zero."""
    c = STREAMK[index]
    m, n, k = c["m"], c["n"], c["k"]
    (record,), _ = gf.tiled_launches("streamk", m, n, k)
    nk = -(-k // 16)
    iters = -(-m // 256) * -(-n // 128) * nk
    assert record.grid_x in (256, 512) and -(-iters // record.grid_x) % nk != 0
    execute(dev, c, "stream-K")
    if index == 0:
        execute(dev, dict(STREAMK[5], offsets="aligned"), "stream-K, behind another shape")
        execute(dev, {key: v for key, v in c.items() if key != "seam"}, "stream-K, again")


# ---- sgemm_dmas_kernel: -(1000 + 100 shape + S) -----------------------------------------------------------------------------------------
def dmas_cases(shape):
    out = []
    S = 1
    while S <= gf.DMAS_MAX_S[shape]:
        out.append(case("dmas", gf.DMAS_BM[shape], gf.DMAS_BN[shape], 64 * S, shape=shape, S=S))                  # one full tile
        out.append(case("dmas", 129, 130, 64 * S + 1, shape=shape, S=S, offsets="all" if S == 2 else "diagonal"))
        S *= 2
    bm, bn = gf.DMAS_BM[shape], gf.DMAS_BN[shape]
    for S in (1, 2):      # KTAIL without EDGE, EDGE without KTAIL (64 x 64 tiles at S = 1 swap both onto eight waves: shape 5)
        out.append(case("dmas", bm, bn, 64 * S + 4, shape=shape, S=S))
        out.append(case("dmas", bm + 8, bn + 4, 64 * S, shape=shape, S=S))
    top = gf.DMAS_MAX_S[shape]
    out.append(case("dmas", 77, 65, 130, shape=shape, S=top))                                                    # the clamp loop: S = 2
    out.append(case("dmas", 200, 136, 520, shape=shape, S=4, batch=3, gaps=(4, 8, 12)))
    return out


DMAS_SPECIALS = [case("dmas", 200, 136, 520, shape=1, S=4, offsets="aligned", seam=160)]       # Kc = 160: an S-chunk edge
# 12 x 12 tiles of 64 x 64, S = 4: 576 workgroups that wait for each other on 512 slots: declined, the planner's choice runs
DMAS_REFUSED = [case("dmas", 768, 768, 256, shape=2, S=4, refused=True)]


@pytest.mark.parametrize("shape", [0, 1, 2, 3, 5])
def test_mid_tiles(shape, dev):
    """Every S the shape allows on one full tile (K = 64 S) and on ragged tiles (129 x 130 x (64 S + 1), where the clamp loop may
    halve S: the record says what ran), a shape that clamps S, a batch of three."""
    for c in dmas_cases(shape):
        execute(dev, c, "mid tiles")


def test_mid_tiles_specials_and_residency(dev):
    for c in DMAS_SPECIALS + DMAS_REFUSED:
        execute(dev, c, "mid tiles")


# ---- sgemm_kq_kernel: -(2000 + shape) ---------------------------------------------------------------------------------------------------
def kq_cases(shape):
    bm, bn = gf.CFG_TILES[gf.FIRST_KQ_CFG + shape]
    out = [case("kq", 2 * bm, 2 * bn, 64, shape=shape, flags=F_VEC, offsets="aligned"),           # VEC, full tiles
           case("kq", 2 * bm + 1, 2 * bn + 4, 60, shape=shape, flags=F_VEC | F_EDGE, offsets="aligned"),  # VEC, ragged
           case("kq", 2 * bm - 3, 2 * bn + 1, 63, shape=shape, flags=F_EDGE),                    # dword loads: odd N, K % 4 != 0
           case("kq", 2 * bm, 2 * bn, 64, shape=shape)]                                          # ... and from an offset alone
    for k in (4, 5, 7, 16, 60, 63, 64, 65, 124, 129):
        out.append(case("kq", bm + 5, bn + 4, k, shape=shape, offsets="all" if (shape, k) == (0, 65) else "diagonal"))
    return out


KQ_SPECIALS = [case("kq", 100, 100, 132, shape=0, offsets="aligned", seam=16)]                 # a quarter of the 64-deep K-tile
KQ_CHUNKS = [case("kq_chunks", m, n, k, shape=shape, S=S, knobs=dict(chunk_major=major))
             for (m, n, k, S), shape in (((33, 35, 2049, 5), 1), ((48, 48, 2051, 7), 0)) for major in (False, True)]
# a remainder chunk of 1 and of 3 elements: the forced plan wants at least 4, declines, and the product falls through to the planner's
# own choice under the same setters — the records name it
KQ_CHUNKS_REFUSED = [case("kq_chunks", m, n, k, shape=shape, S=S, knobs=dict(chunk_major=major), refused=True)
                     for (m, n, k, S), shape in (((33, 35, 1281, 5), 1), ((48, 48, 1923, 7), 0)) for major in (False, True)]
KQ_CHUNKS_SPECIALS = [case("kq_chunks", 48, 48, 2052, shape=0, S=7, offsets="aligned", seam=320)]   # Kc = 320: a K-chunk edge


@pytest.mark.parametrize("shape", range(7))
def test_k_quartered_tiles(shape, dev):
    for c in kq_cases(shape):
        execute(dev, c, "k-quartered")


def test_k_quartered_tiles_over_k_chunks(dev):
    """S K-chunks as the batch of one launch, tile-major (-25) and chunk-major (-26), the remainder chunk riding as the last batch
    entry (K_last in the record), np_reduce_axis folding the partials (FOLD in the mask).  A remainder of 1 .. 3 elements never
    reaches launch_kq: the forced plan wants at least 4 and declines (33 x 35 x 1281 with S = 5, 48 x 48 x 1923 with S = 7), and
    the product runs what the planner chooses instead."""
    for c in KQ_CHUNKS + KQ_CHUNKS_REFUSED + KQ_SPECIALS + KQ_CHUNKS_SPECIALS:
        execute(dev, c, "k-quartered")


# ---- sgemm_kernel / sgemm_pipe_kernel: variants 1 .. 6 ----------------------------------------------------------------------------------
def tile_cases(variant):
    bk = 32 if variant == 2 else 16
    full = (64, 64, 16) if variant == 4 else (128, 128, bk)
    out = [case("tile", *full, variant=variant, flags=F_VEC, offsets="aligned"),
           case("tile", 130, 132, 20, variant=variant, flags=F_VEC | F_EDGE, offsets="all" if variant == 1 else "diagonal"),
           case("tile", 129, 127, 17, variant=variant, flags=F_EDGE),
           case("tile", 128, 128, 8, variant=variant, flags=F_VEC | F_EDGE), case("tile", 65, 63, 5, variant=variant, flags=F_EDGE)]
    if variant == 1:
        out.append(case("tile", 130, 132, 20, variant=1, offsets="aligned", seam=16))
    return out


# N < 4 or K < 4 keeps the LDS-DMA forms out of a batch: the planner's register-staged tiles, dword loads
PLANNER_FALLBACKS = [case("plan", 200, 3, 50, batch=2), case("plan", 100, 100, 3, batch=2)]


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6])
def test_register_staged_tiles(variant, dev):
    for c in tile_cases(variant):
        execute(dev, c, "variant %d" % variant)


def test_planner_fallbacks_of_a_batch(dev):
    for c in PLANNER_FALLBACKS:
        assert plan_of(dev.L, c["m"], c["n"], c["k"], 2)[0] in (1, 2)
        execute(dev, c, "fallback")


# ---- np::sgemm_sub_ld -------------------------------------------------------------------------------------------------------------------
SUB = [case("sub", 128, 128, 16, flags=F_VEC, ld=(0, 0, 0)), case("sub", 256, 128, 32, flags=F_VEC, ld=(4, 8, 12)),
       case("sub", 130, 132, 20, flags=F_VEC | F_EDGE, ld=(4, 4, 8)), case("sub", 129, 127, 17, flags=F_EDGE, ld=(3, 1, 5), offsets="all"),
       case("sub", 200, 72, 64, flags=F_VEC | F_EDGE, ld=(136, 200, 200))]


def test_subtracting_epilogue(dev):
    """C = C0 - A . B on the windows the factorizations use (ldc > N, ragged M, N, K), in its three instantiations; a NaN in C0 stays
    in its own element."""
    for c in SUB:
        m, n, k, _, lda, ldb, ldc, _ = geometry(c)
        A, B = operands_of(c)
        rng = np.random.default_rng(5)
        c0 = rng.integers(-1000, 1001, size=(m, n)).astype(np.float32)
        offsets = ALL_OFFSETS if c.get("offsets") == "all" else DIAGONAL
        at = {off: expectation(c, dev.L, *off) for off in offsets}
        assert at[0, 0][0][0].flags & (F_VEC | F_EDGE) == c["flags"] and at[0, 0][0][0].flags & gf.F_SUB
        run_tiled(dev, A, B, gf.expected_sub(c0, A, B), lambda oa, ob: at[oa, ob][0], offsets, 0, lda=lda, ldb=ldb, ldc=ldc, c0=c0, label="sub")
        holed = c0.copy()
        holed[m - 1, n - 1] = holed[0, 0] = holed[m // 2, 1] = np.nan
        want = gf.expected_sub(np.nan_to_num(holed), A, B)
        want[np.isnan(holed)] = np.nan
        run_tiled(dev, A, B, want, at[0, 0][0], ALIGNED, 0, lda=lda, ldb=ldb, ldc=ldc, c0=holed, label="sub, NaN in C0")


# ---- launch_padded: (-6), (-3) ----------------------------------------------------------------------------------------------------------
PADDED = [case("padded", 257, 131, 50, offsets="all"), case("padded", 300, 130, 33)]


def test_padded_copies(dev):
    """pad_copy_kernel twice, then the aligned kernel with n_store: it computes Np = N rounded up to 4 columns and must store N of
    them — the canary behind column N of every row is the next row's first element, compared like every other float."""
    for c in PADDED:
        records, _ = expectation(c, dev.L)
        assert [r.family for r in records] == [gf.K_PAD_COPY, gf.K_PAD_COPY, gf.K_DMA] and records[2].flags == F_VEC | F_EDGE
        assert (records[0].s, records[1].s) == (-(-c["k"] // 16) * 16, -(-c["n"] // 4) * 4)
        execute(dev, c, "padded")


# ---- the split-K plans of cfg 0 .. 2 with a remainder chunk: (-14), (-20), (-22) -----------------------------------------------------------
SPLITK_CODES = (-14, -20, -22)
# The smallest shapes (M and N on a grid of 64; K in 512, 516, 528, 640, 1028, 1040, 2052, 4100) whose plan for 256 CUs splits every
# tile row and has a remainder chunk, and the smallest that splits only a tail of the tile rows and has one: searched on the host,
# pinned with the plans (cfg, tail_rows, chunks) in tests/test_gemm_reference_cpu.py::test_split_k_plans_pinned
SPLITK_ALL_ROWS = [case("plan", 64, 64, 516, codes=SPLITK_CODES), case("plan", 128, 128, 2052, codes=SPLITK_CODES)]
SPLITK_TAIL_ROWS = [case("plan", 1216, 1728, 1028, codes=SPLITK_CODES)]


def test_split_k_plans(dev):
    """The remainder chunk rides as the last batch entry (K_last in the record); np_reduce_axis folds the partials."""
    for c in SPLITK_ALL_ROWS + SPLITK_TAIL_ROWS:
        execute(dev, c, "split-K")


# ---- the default planner ----------------------------------------------------------------------------------------------------------------
PLANNER = [case("plan", m, n, k) for m, n, k in ((96, 96, 96), (128, 128, 128), (256, 256, 256), (264, 260, 252), (512, 512, 512), (768, 768, 768),
                                                  (1024, 1024, 1024), (1100, 1100, 1100), (2048, 2048, 256), (512, 512, 4096), (100, 100, 10000),
                                                  (1280, 1280, 1280), (1536, 1536, 512))]


@pytest.mark.parametrize("index", range(len(PLANNER)))
def test_default_planner(index, dev):
    """What ran is what np_sgemm_debug_plan says: cfg, tail_rows, S, stream-K taken."""
    execute(dev, PLANNER[index], "planner")


def all_cases():
    """Every case of the module (tests/test_gemm_reference_cpu.py derives each one's records without a device)."""
    out = DMA_INSTANTIATIONS + DMA_K + DMA_MN + DMA_RESIDUES + DMA_SPECIALS + DMA_SWIZZLE + DMA_BATCH + DMA_WINDOWS + STREAMK
    for shape in (0, 1, 2, 3, 5):
        out = out + dmas_cases(shape)
    out = out + DMAS_SPECIALS + DMAS_REFUSED
    for shape in range(7):
        out = out + kq_cases(shape)
    out = out + KQ_SPECIALS + KQ_CHUNKS + KQ_CHUNKS_REFUSED + KQ_CHUNKS_SPECIALS
    for variant in range(1, 7):
        out = out + tile_cases(variant)
    return out + PLANNER_FALLBACKS + SUB + PADDED + SPLITK_ALL_ROWS + SPLITK_TAIL_ROWS + PLANNER
