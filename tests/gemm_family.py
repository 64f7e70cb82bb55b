"""Operands on which every correct matrix product returns the same bits, whatever its order — the exact family behind
tests/test_gemm_reference_cpu.py (the family against numpy in several summation orders and against the oracle's OpenBLAS) and
tests/test_gpu_gemm_exact.py (the thin, few-row and matrix-vector kernels of np_sgemm.hip against the family).  Plain numpy,
seeded, no device.

A tolerance of 1e-6 |A|.|B| on U(-1, 1) data is ~K / 4e6 absolute while one product a.b averages 0.25: from K ~ 10^6 on a kernel
that drops or doubles the element at a chunk edge, or the last K % 4 elements of a row, passes.  Here nothing rounds:

  operands  A (m x k), B (k x n) of nonzero integers +-1 .. +-amp with k . amp_a . amp_b < 2^24: every partial sum of every inner
            product, in every order, on the vector ALU (fmaf) or the fp32 MFMA, is an integer below 2^24, which fp32 holds
            exactly.  A dropped, doubled or mis-paired product moves the result by at least 1.
  specials  NaN / Inf planted at a seam of K and an edge of M / N; the expected CLASS of every element of C (finite, +Inf, -Inf,
            NaN) follows from the planted positions and the signs next to them, not from a float product.
  framed    the host image of an operand at float offset 0 .. 3 inside a NaN-filled allocation; canary: the same for C, a -777
            frame around a NaN interior (an element the kernel does not write stays NaN, one it writes outside shows).

tiled_launches() restates the HOST arithmetic of the launchers behind launch_sgemm_ld (which instantiation, which grid, which
S) and returns the records np_sgemm_debug_last_launches must report; expected_sub() is the exact C0 - A . B of np::sgemm_sub_ld.

path() / gemv_path() restate the dispatcher of np_sgemm.hip (launch_thin_nv, launch_fewrows, launch_skinny, the thin-left branch,
np_sgemv) as arithmetic on a device of `cus` CUs and return the NP_SGEMM_PATH_ mask of include/np_hip_debug.h that
np_sgemm_debug_last_path must report: the GPU tests name the mask of every case, the CPU tier checks the names against this
arithmetic, so an expectation is derived before it is observed.  Peeled products (try_peeled) are outside it.
"""
import math

import numpy as np

EXACT_LIMIT = 1 << 24      # fp32 holds every integer up to here

# NP_SGEMM_PATH_ bits of include/np_hip_debug.h (tests/test_gemm_reference_cpu.py checks them against the header)
THIN_LANES, THIN_MFMA16, THIN_MFMA32, THIN_MFMA32X2, THIN_K_CHUNKS = 0x1, 0x2, 0x4, 0x8, 0x10
FEWROWS_SPLITK1, FEWROWS_SPLITK2, THIN_CHUNKS, FEWROWS, SKINNY, FOLD = 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
THIN_LEFT, PEELED, GEMV_STAGED, GEMV_SHORT_ROWS, GEMV_FEWROWS_CHUNKS = 0x800, 0x1000, 0x2000, 0x4000, 0x8000
GEMV_CHUNKS, GEMV_WAVE, GEMV_WAVE_VEC, TILED = 0x10000, 0x20000, 0x40000, 0x80000
PATH_BITS = {"THIN_LANES": THIN_LANES, "THIN_MFMA16": THIN_MFMA16, "THIN_MFMA32": THIN_MFMA32, "THIN_MFMA32X2": THIN_MFMA32X2,
             "THIN_K_CHUNKS": THIN_K_CHUNKS, "FEWROWS_SPLITK1": FEWROWS_SPLITK1, "FEWROWS_SPLITK2": FEWROWS_SPLITK2,
             "THIN_CHUNKS": THIN_CHUNKS, "FEWROWS": FEWROWS, "SKINNY": SKINNY, "FOLD": FOLD, "THIN_LEFT": THIN_LEFT, "PEELED": PEELED,
             "GEMV_STAGED": GEMV_STAGED, "GEMV_SHORT_ROWS": GEMV_SHORT_ROWS, "GEMV_FEWROWS_CHUNKS": GEMV_FEWROWS_CHUNKS,
             "GEMV_CHUNKS": GEMV_CHUNKS, "GEMV_WAVE": GEMV_WAVE, "GEMV_WAVE_VEC": GEMV_WAVE_VEC, "TILED": TILED}


def LANES(L):
    """The lane-group width of sgemm_thin_kernel / sgemv_short_rows_kernel as np_sgemm_debug_last_path reports it (bits 20 .. 23)."""
    assert L in (1, 2, 4, 8, 16, 32, 64)
    return (L.bit_length()) << 20


def MV(mv):
    """The accumulator count of sgemm_fewrows_kernel / sgemm_thin_left_kernel as the probe reports it (bits 24 .. 27)."""
    assert mv in (1, 2, 4, 8, 16)
    return (mv.bit_length()) << 24


def describe(mask):
    names = [n for n, b in PATH_BITS.items() if mask & b]
    if (mask >> 20) & 15:
        names.append("L=%d" % (1 << (((mask >> 20) & 15) - 1)))
    if (mask >> 24) & 15:
        names.append("MV=%d" % (1 << (((mask >> 24) & 15) - 1)))
    rest = mask & ~(sum(PATH_BITS.values()) | (0xff << 20))
    return "|".join(names) + ("|0x%x?" % rest if rest else "") if mask else "0"


# ---- exact operands -------------------------------------------------------------------------------------------------------------
def amp_for(k, cap=64):
    """The largest amp <= cap with k . amp . amp < 2^24."""
    return max(1, min(cap, math.isqrt((EXACT_LIMIT - 1) // k)))


def _ints(shape, rng, amp):
    mag = rng.integers(1, amp + 1, size=shape, dtype=np.int16)
    return np.where(rng.integers(0, 2, size=shape, dtype=np.int8) == 1, mag, -mag).astype(np.float32)


def operands(m, n, k, seed, amp_a, amp_b):
    """A (m x k), B (k x n): nonzero integers +-1 .. +-amp as fp32.  Refuses a shape that could leave the exact range."""
    if amp_a < 1 or amp_b < 1:
        raise ValueError("operands: amplitudes must be at least 1")
    if k * amp_a * amp_b >= EXACT_LIMIT:
        raise ValueError("operands: k . amp_a . amp_b = %d leaves the exact fp32 range (2^24)" % (k * amp_a * amp_b))
    rng = np.random.default_rng(seed)
    return _ints((m, k), rng, amp_a), _ints((k, n), rng, amp_b)


def vector(k, seed, amp):
    """x (k,) for np_sgemv, the same way; the matrix it meets must keep k . amp_a . amp < 2^24 (expected() checks)."""
    if amp < 1:
        raise ValueError("vector: amp must be at least 1")
    if k * amp >= EXACT_LIMIT:
        raise ValueError("vector: k . amp = %d leaves the exact fp32 range (2^24)" % (k * amp))
    return _ints((k,), np.random.default_rng(seed), amp)


def expected(A, B):
    """The integer product as fp32.  Computed in fp64, where every partial sum (an integer below 2^24 in magnitude: checked on
    |A| . |B|) is exact in any order, so the BLAS behind numpy returns THE integer product; refuses operands that are not integers
    or whose |A| . |B| reaches 2^24.  B may be a vector."""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if not (np.isfinite(A64).all() and np.isfinite(B64).all() and (A64 == np.rint(A64)).all() and (B64 == np.rint(B64)).all()):
        raise ValueError("expected: operands must be finite integers")
    bound = np.abs(A64) @ np.abs(B64)
    if bound.size and bound.max() >= EXACT_LIMIT:
        raise ValueError("expected: |A| . |B| reaches %d: outside the exact fp32 range (2^24)" % int(bound.max()))
    c = A64 @ B64
    ci = np.rint(c).astype(np.int64)
    assert (ci == c).all() and (np.abs(ci) < EXACT_LIMIT).all()
    return ci.astype(np.float32)


def expected_int64(A, B):
    """The same in int64 arithmetic, no floating point anywhere (slow: the CPU tier holds expected() against it)."""
    return (np.asarray(A).astype(np.int64) @ np.asarray(B).astype(np.int64)).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- seams ----------------------------------------------------------------------------------------------------------------------
SEAM_UNITS = (4, 16, 32, 64, 256, 512, 1024, 2048, 4096)


def k_seams(k):
    """Where along K these kernels have seams: both ends, +-1 around every multiple of 4, 16, 32, 64, 256, 512, 1024, 2048 and 4096
    (float4 loads, MFMA steps, LDS chunks, K-chunk lengths and their roundings) up to k, and the last four positions.  (Every unit
    is a multiple of 4: the list is every position but the k = 4 t + 2, which sit strictly inside a float4.)"""
    mult = np.unique(np.concatenate([np.arange(0, k + 1, u, dtype=np.int64) for u in SEAM_UNITS]))
    p = np.concatenate([mult - 1, mult, mult + 1, np.array([0, k - 4, k - 3, k - 2, k - 1], np.int64)])
    return np.unique(p[(p >= 0) & (p < k)]).tolist()


# ---- specials -------------------------------------------------------------------------------------------------------------------
NAN_IN_A, NAN_IN_B, INF_IN_B, INF_TIMES_ZERO, INF_MEETS_MINUS_INF = range(5)
SPECIAL_KINDS = (NAN_IN_A, NAN_IN_B, INF_IN_B, INF_TIMES_ZERO, INF_MEETS_MINUS_INF)
FINITE, PLUS_INF, MINUS_INF, NAN = range(4)      # classes of an element of C


def classify(c):
    c = np.asarray(c)
    return np.where(np.isnan(c), NAN, np.where(c == np.inf, PLUS_INF, np.where(c == -np.inf, MINUS_INF, FINITE))).astype(np.int8)


def specials(A, B, kind, ks, i, j, ks2=None, base=None):
    """Plant `kind` into copies of exact operands: at row i of A / column j of B (the row and column edges are the caller's
    choice), at position ks of K (from k_seams); INF_MEETS_MINUS_INF needs a second position ks2 != ks.  Returns (A', B', cls,
    want): cls the expected class of every element of C, derived from the planted positions and the signs of the elements that
    meet them; want the exact product where cls is FINITE and +-Inf / NaN elsewhere.  base = expected(A, B) if the caller has it
    already.  B may be a vector (j = 0)."""
    A2, B2 = A.copy(), B.copy()
    Bm = B2.reshape(B2.shape[0], -1)            # a view
    m, n = A2.shape[0], Bm.shape[1]
    cls = np.full((m, n), FINITE, np.int8)
    if kind == NAN_IN_A:
        A2[i, ks] = np.nan
        cls[i, :] = NAN                         # NaN . b, b finite and nonzero or not: NaN in the whole row
    elif kind == NAN_IN_B:
        Bm[ks, j] = np.nan
        cls[:, j] = NAN
    elif kind in (INF_IN_B, INF_TIMES_ZERO):
        Bm[ks, j] = np.inf
        if kind == INF_TIMES_ZERO:
            A2[i, ks] = 0.0
        cls[:, j] = np.where(A2[:, ks] > 0, PLUS_INF, MINUS_INF)       # every A[:, ks] is nonzero: a . Inf = +-Inf by a's sign
        if kind == INF_TIMES_ZERO:
            cls[i, j] = NAN                     # IEEE 0 . Inf = NaN, at C[i, j] alone
    elif kind == INF_MEETS_MINUS_INF:
        if ks2 is None or ks2 == ks:
            raise ValueError("specials: INF_MEETS_MINUS_INF needs ks2 != ks")
        Bm[ks, j], Bm[ks2, j] = np.inf, -np.inf
        A2[i, ks2] = abs(A2[i, ks2]) * np.sign(A2[i, ks])             # row i: a . Inf and a' . -Inf of opposite sign meet
        if m > 1:
            r = (i + 1) % m
            A2[r, ks2] = -abs(A2[r, ks2]) * np.sign(A2[r, ks])        # the next row: both products have one sign
        s1, s2 = np.sign(A2[:, ks]), -np.sign(A2[:, ks2])
        cls[:, j] = np.where(s1 != s2, NAN, np.where(s1 > 0, PLUS_INF, MINUS_INF))
    else:
        raise ValueError("specials: unknown kind %r" % (kind,))
    # the finite elements never meet a planted NaN / Inf; they see the exact product of the base operands, moved by the finite
    # entries of A that were planted (the zero, the two aligned signs): integer arithmetic on the rows concerned
    if base is None:
        base = expected(A, B)
    want64 = np.rint(np.asarray(base, np.float64).reshape(m, n)).astype(np.int64)
    B0 = np.asarray(B).reshape(B.shape[0], -1)
    for r, kk in zip(*np.nonzero(np.isfinite(A2) & (A2 != A))):
        want64[r, :] += (np.int64(A2[r, kk]) - np.int64(A[r, kk])) * B0[kk, :].astype(np.int64)
    if np.abs(want64[cls == FINITE]).max(initial=0) >= EXACT_LIMIT:
        raise ValueError("specials: a finite element left the exact fp32 range")
    want = want64.astype(np.float32)
    want = np.where(cls == NAN, np.float32(np.nan), np.where(cls == PLUS_INF, np.float32(np.inf),
                    np.where(cls == MINUS_INF, np.float32(-np.inf), want))).astype(np.float32)
    if B.ndim == 1:
        cls, want = cls[:, 0], want[:, 0]
    return A2, B2, cls, want


# ---- frames ---------------------------------------------------------------------------------------------------------------------
CANARY = np.float32(-777.0)


def framed(array, offset_floats, pad=64):
    """(image, start): `array` flattened at float `pad + offset_floats` of a NaN-filled buffer with `pad` floats of NaN on either
    side (pad a multiple of 4: on a 16-byte aligned allocation the operand's alignment is offset_floats alone)."""
    if pad % 4 or not 0 <= offset_floats <= 3:
        raise ValueError("framed: pad must be a multiple of 4 and the offset 0 .. 3 floats")
    flat = np.ascontiguousarray(array, np.float32).reshape(-1)
    start = pad + offset_floats
    image = np.full(start + flat.size + pad, np.nan, np.float32)
    image[start:start + flat.size] = flat
    return image, start


def canary(size, offset_floats=0, pad=1024):
    """(image, start) for C: `size` floats of NaN inside a frame of -777."""
    if pad % 4 or not 0 <= offset_floats <= 3:
        raise ValueError("canary: pad must be a multiple of 4 and the offset 0 .. 3 floats")
    start = pad + offset_floats
    image = np.full(start + size + pad, CANARY, np.float32)
    image[start:start + size] = np.nan
    return image, start


def frame_intact(image, start, size):
    return bool((image[:start] == CANARY).all() and (image[start + size:] == CANARY).all())


# ---- the dispatcher as arithmetic -----------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def gemv_path(m, n, cus=256, a_aligned=True, x_aligned=True):
    """np_sgemv(M = m rows, N = n columns)."""
    target = cus * 8
    if 4 <= n <= 63 and m >= 262144 and a_aligned:
        pitch = n | 1
        R = max((8192 // pitch) // 256 * 256, 256)
        if (R * pitch + n) * 4 <= 64 * 1024:
            return GEMV_STAGED
    if n <= 256 and m >= 1024:
        L = 1
        while L * 8 < n:
            L *= 2
        return GEMV_SHORT_ROWS | LANES(min(L, 32))
    if 2 <= m <= 16 and n >= 65536:
        return GEMV_FEWROWS_CHUNKS | FOLD
    if m < 2 * target and n >= 16384 and m <= 65535:
        if min(_cdiv(2 * target, m), n // 4096) >= 2:
            return GEMV_CHUNKS | FOLD
    return GEMV_WAVE | (GEMV_WAVE_VEC if n % 4 == 0 and a_aligned and x_aligned else 0)


def thin_chunks(m, n, k, cus=256):
    """(kernel bit, workgroups, K-chunks, chunk length) of the K-chunked launch launch_thin_nv would make for 17 <= m < 2048 rows,
    n <= 64, k >= 16384 — before thin_to_planner() is asked — or None."""
    target = cus * 8
    if 16 < m <= 64 and n > 16 and k >= 16384:
        row_tiles = _cdiv(m, 32)
        chunks = min(_cdiv(target * 8, row_tiles), k // 1024)
        if chunks >= 8:
            kc = _cdiv(_cdiv(k, chunks), 32) * 32
            chunks = _cdiv(k, kc)
            groups = _cdiv(chunks, 4)
            return (FEWROWS_SPLITK1 if n <= 32 else FEWROWS_SPLITK2), row_tiles * groups, chunks, kc
    if 16 < m < 2048 and k >= 16384:
        blocks = _cdiv(m, 64 if n <= 16 else 128)
        chunks = min(_cdiv(target * 2, blocks), k // 2048, 65535)
        if chunks >= 2:
            kc = _cdiv(_cdiv(k, chunks), 64) * 64
            chunks = _cdiv(k, kc)
            kernel = THIN_MFMA16 if n <= 16 else THIN_MFMA32 if n <= 32 else THIN_MFMA32X2
            return kernel | THIN_K_CHUNKS, blocks * chunks, chunks, kc
    return None


def _thin(m, n, k, cus, q, aligned):
    """launch_thin_nv: a mask, or None where it returns 1 (shape not taken)."""
    target = cus * 8
    if n == 1 and m >= 2048 and k >= 256:
        return gemv_path(m, k, cus, aligned, aligned)
    if m >= 2048 and n <= 4 and k * n <= 16384 and (k < 1024 or m >= 65536):
        L = 1
        while L * 8 < k and L < 64:
            L *= 2
        return THIN_LANES | LANES(L)
    if m >= 2048 and (n > 4 or (k >= 1024 and m < 65536)) and n <= 32 and k >= 4:
        kernel = THIN_MFMA16 if n <= 16 else THIN_MFMA32
        blocks = _cdiv(m, 64 if n <= 16 else 128)
        if blocks < target and k >= 1024 and min(_cdiv(target, blocks), k // 512, 65535) >= 2:
            return kernel | THIN_K_CHUNKS | FOLD
        return kernel
    plan = thin_chunks(m, n, k, cus)
    if plan is not None:
        if plan[1] * 4 < q * cus:              # thin_to_planner(): fewer than q / 4 workgroups per CU
            return None
        return plan[0] | FOLD
    if m <= 16 and n <= 8 and k >= 65536:
        return THIN_CHUNKS | FOLD
    return None


def path(m, n, k, cus=256, q=59, aligned=True):
    """np_sgemm(M, N, K) of one dense product, not peeled: the mask, with TILED for everything launch_sgemm takes (whether the
    planner then folds partials of its own is the planner's model: compare with FOLD masked out)."""
    if n <= 32 or (n <= 64 and m < 2048 and k >= 16384):
        mask = _thin(m, n, k, cus, q, aligned)
        if mask is not None:
            return mask
    if m <= 8 and n >= 256 and k >= 256 and k * n >= 6e6:
        col_blocks = _cdiv(n, 256)
        chunks = max(min(_cdiv(cus * 6, col_blocks), k // 16), 1)
        chunk_len = _cdiv(_cdiv(k, chunks), 4) * 4
        return FEWROWS | MV(1 if m == 1 else 2 if m == 2 else 4 if m <= 4 else 8) | (FOLD if _cdiv(k, chunk_len) > 1 else 0)
    if 9 <= m <= 32 and n >= 512 and k >= 512 and k * n >= 16e6:
        col_blocks = _cdiv(n, 128)
        chunks = max(min(_cdiv(cus * 3, col_blocks), int(0.075 * k / m), k // 64), 1)
        chunk_len = _cdiv(_cdiv(k, chunks), 64) * 64
        return SKINNY | (FOLD if _cdiv(k, chunk_len) > 1 else 0)
    if m <= 16 and k <= 64 and n >= 65536:
        return THIN_LEFT | MV(4 if m <= 4 else 8 if m <= 8 else 16)
    return TILED


# ---- the subtracting epilogue -----------------------------------------------------------------------------------------------------
def expected_sub(C0, A, B):
    """C0 - A . B as fp32 for integer C0, A, B with |C0| + |A| . |B| < 2^24: the accumulator (an integer below 2^24 in every order)
    and the one subtraction at the end, or a subtraction per step, are all exact."""
    C64 = np.asarray(C0, np.float64)
    if not (np.isfinite(C64).all() and (C64 == np.rint(C64)).all()):
        raise ValueError("expected_sub: C0 must be finite integers")
    bound = np.abs(C64) + np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64))
    if bound.size and bound.max() >= EXACT_LIMIT:
        raise ValueError("expected_sub: |C0| + |A| . |B| reaches %d: outside the exact fp32 range (2^24)" % int(bound.max()))
    return (C64 - expected(A, B).astype(np.float64)).astype(np.float32)


# ---- the launchers behind launch_sgemm_ld as arithmetic ---------------------------------------------------------------------------
# NP_SGEMM_KERNEL_ / NP_SGEMM_LAUNCH_F_ of include/np_hip_debug.h (tests/test_gemm_reference_cpu.py checks them against the header)
K_TILE, K_PIPE, K_DMA, K_STREAMK, K_DMAS, K_KQ, K_PAD_COPY, K_TILE_SUB = range(1, 9)
KERNELS = {"TILE": K_TILE, "PIPE": K_PIPE, "DMA": K_DMA, "STREAMK": K_STREAMK, "DMAS": K_DMAS, "KQ": K_KQ, "PAD_COPY": K_PAD_COPY,
           "TILE_SUB": K_TILE_SUB}
F_VEC, F_EDGE, F_KTAIL, F_PRIO, F_BUF, F_SUB, F_SWIZZLE, F_CHUNK_MAJOR, F_PIPE_MODE1 = (1 << i for i in range(9))
LAUNCH_FLAGS = {"VEC": F_VEC, "EDGE": F_EDGE, "KTAIL": F_KTAIL, "PRIO": F_PRIO, "BUF": F_BUF, "SUB": F_SUB, "SWIZZLE": F_SWIZZLE,
                "CHUNK_MAJOR": F_CHUNK_MAJOR, "PIPE_MODE1": F_PIPE_MODE1}
LAUNCH_WORDS, LAUNCH_KEPT = 8, 16
DMAS_BM, DMAS_BN, DMAS_MAX_S, DMAS_BK = (128, 128, 64, 128, 128, 64), (128, 64, 64, 128, 64, 64), (16, 8, 4, 16, 8, 4), (16, 32, 32, 32, 32, 32)
KQ_SHAPES = ((3, 3), (2, 2), (4, 4), (3, 2), (4, 2), (4, 3), (5, 3))       # TM, TN in 16-row / 16-column blocks
CFG_TILES = ((256, 128), (128, 128), (64, 64), (128, 128), (128, 64), (64, 64)) + tuple((16 * a, 16 * b) for a, b in KQ_SHAPES)
FIRST_MID_CFG, FIRST_KQ_CFG = 3, 6
STREAMK_MAX_GRID = 1024


class Launch(tuple):
    """One record of np_sgemm_debug_last_launches: (family, bm, bn, bk, shape, flags, s, grid_x, grid_z, k_last); shape -1 = none."""
    __slots__ = ()
    FIELDS = ("family", "bm", "bn", "bk", "shape", "flags", "s", "grid_x", "grid_z", "k_last")

    def __new__(cls, family, bm, bn, bk, shape, flags, s, grid_x, grid_z, k_last):
        return tuple.__new__(cls, (int(family), int(bm), int(bn), int(bk), int(shape), int(flags), int(s), int(grid_x), int(grid_z), int(k_last)))

    family, bm, bn, bk, shape, flags, s, grid_x, grid_z, k_last = (property(lambda self, i=i: self[i]) for i in range(10))

    @classmethod
    def decode(cls, words):
        w = [int(x) for x in words]
        return cls(w[0], w[1] & 0xffff, w[1] >> 16, w[2] & 0xffff, (w[2] >> 16) - 1, w[3], w[4], w[5], w[6], w[7])

    def __repr__(self):
        kernel = {v: n for n, v in KERNELS.items()}.get(self.family, "?%d" % self.family)
        flags = "|".join(n for n, b in LAUNCH_FLAGS.items() if self.flags & b) or "0"
        return "%s(%dx%dx%d shape %d, %s, S %d, grid %d x %d, K_last %d)" % (kernel, self.bm, self.bn, self.bk, self.shape, flags, self.s,
                                                                            self.grid_x, self.grid_z, self.k_last)

    def instantiation(self):
        """What names the template instantiation: kernel, tile, shape and the template-argument flags."""
        keep = F_VEC | F_EDGE | F_KTAIL | F_PRIO | F_BUF | F_SUB | F_PIPE_MODE1
        return (self.family, self.bm, self.bn, self.bk, self.shape, self.flags & keep)


class Knobs:
    """The process-wide switches of np_sgemm.hip a launcher reads, at their defaults (include/np_hip_debug.h)."""

    def __init__(self, **kw):
        self.cus = 256
        self.kloop = 1             # -31: 0, -32: 2, -33: 1
        self.prio_period = 16      # -(100 + p); p != 16 applies at every K
        self.prio_min_k = 2048
        self.mid_waves = True      # -18 / -19
        self.mid_swizzle = True    # -16 / -17
        self.chunk_major = True    # -25 / -26
        self.variant = 0           # g_variant: 0, 1 .. 7, 47
        for name, value in kw.items():
            if not hasattr(self, name):
                raise TypeError("Knobs: no %s" % name)
            setattr(self, name, value)
        if "prio_period" in kw and "prio_min_k" not in kw:
            self.prio_min_k = 2048 if self.prio_period == 16 else 0


class _G:
    """GemmArgs + what launch_sgemm_ld derives: the fields the launchers' conditions read."""

    def __init__(self, m, n, k, lda, ldb, ldc, batch=1, sa=0, sb=0, a_aligned=True, b_aligned=True):
        self.M, self.N, self.K, self.lda, self.ldb, self.ldc, self.batch = m, n, k, lda, ldb, ldc, batch
        self.sa, self.sb, self.a_aligned, self.b_aligned = sa, sb, a_aligned, b_aligned
        self.K_last = self.n_store = self.k_chunks = 0
        self.swizzle = 0

    def copy(self, **kw):
        g = _G.__new__(_G)
        g.__dict__.update(self.__dict__)
        g.__dict__.update(kw)
        return g

    def vec(self):
        return (self.K % 4 == 0 and self.lda % 4 == 0 and self.N % 4 == 0 and self.ldb % 4 == 0 and self.a_aligned and self.b_aligned
                and self.sa % 4 == 0 and self.sb % 4 == 0)


def _flags(vec=False, edge=False, ktail=False, prio=False, buf=False, swizzle=False, chunk_major=False):
    return ((F_VEC if vec else 0) | (F_EDGE if edge else 0) | (F_KTAIL if ktail else 0) | (F_PRIO if prio else 0) | (F_BUF if buf else 0)
            | (F_SWIZZLE if swizzle else 0) | (F_CHUNK_MAJOR if chunk_major else 0))


def _kloop_takes(g, batch, ktail, in_default_set, kn):
    return bool((kn.kloop == 2 or (kn.kloop == 1 and in_default_set)) and not ktail and g.a_aligned and g.b_aligned and g.lda % 4 == 0
                and g.ldb % 4 == 0 and g.lda < 1 << 22 and g.ldb < 1 << 22 and (batch == 1 or (g.sa % 4 == 0 and g.sb % 4 == 0)))


def _launch_tile(g, batch, vec, bm, bn, bk, family=K_TILE, extra=0):
    """launch_sgemm_tile / launch_sgemm_pipe / np::sgemm_sub_ld: <VEC, EDGE> = (1, 0), (1, 1) or (0, 1)."""
    edge = bool(g.M % bm or g.N % bn or g.K % bk or g.K_last % bk)
    return Launch(family, bm, bn, bk, -1, _flags(vec, edge or not vec, swizzle=g.swizzle) | extra, 1, _cdiv(g.M, bm) * _cdiv(g.N, bn), batch, g.K_last)


def _launch_dma(g, batch, vec, kn):
    """launch_cfg(0): sgemm_dma_kernel<EDGE, KTAIL, PRIO, BUF>."""
    tiles_m, tiles_n = _cdiv(g.M, 256), _cdiv(g.N, 128)
    swizzle = g.swizzle or (kn.variant == 0 and tiles_m >= 8)
    edge = bool(g.M % 256 or g.N % 128 or g.n_store)
    ktail = bool(g.K % 16 or g.K_last % 16 or g.N % 4)
    prio = bool(not edge and not ktail and kn.prio_period and g.K >= kn.prio_min_k)
    buf = _kloop_takes(g, batch, ktail, prio, kn)
    return Launch(K_DMA, 256, 128, 16, -1, _flags(vec, edge, ktail, prio, buf, swizzle), 1, tiles_m * tiles_n, batch, g.K_last)


def streamk_grid(m, n, k, cus=256):
    """streamk_model's grid: two workgroups per CU, else one, with ranges of at least 24 K-tiles; the SHORTER modelled time wins,
    which needs the model's two efficiencies (kCfg[0].eff = 0.93 shared by two, eff1 = 0.89) and its 8 us + 3 us per fold.
    0 where stream-K does not apply."""
    tm, tn, nk = _cdiv(m, 256), _cdiv(n, 128), _cdiv(k, 16)
    iters = tm * tn * nk
    ragged = 1.02 if (m % 256 or n % 128 or k % 16) else 1.0
    best, grid = 1e300, 0
    for per_cu in (2, 1):
        G = min(per_cu * cus, STREAMK_MAX_GRID)
        per_wg = _cdiv(iters, G)
        if per_wg < 24:
            continue
        eff = 0.93 / 2.0 if per_cu == 2 else 0.89
        t_kt = 2.0 * 256.0 * 128.0 * 16.0 / (eff * (157.3e12 / 256.0))
        folds = 1.0 if per_wg >= nk else float(_cdiv(nk, per_wg) - 1)
        t = per_wg * t_kt * ragged + 8e-6 + 3e-6 * folds
        if t < best:
            best, grid = t, G
    return grid


def streamk_range_starts(m, n, k, G):
    """Where sgemm_streamk_kernel cuts its K-tiles among G workgroups: workgroup w runs [iters . w / G, iters . (w + 1) / G) (floor),
    iters = tiles . K-tiles, tile-major.  Returns (starts, K-tiles per tile); a start that is no multiple of the K-tile count lies
    inside a tile: the partial before it ends there and the next one begins — a range edge."""
    nk = _cdiv(k, 16)
    iters = _cdiv(m, 256) * _cdiv(n, 128) * nk
    G = min(G, iters)
    return [iters * w // G for w in range(G)], nk


def _launch_streamk(g, G, kn):
    """launch_streamk on G workgroups."""
    tiles_m, tiles_n, nk = _cdiv(g.M, 256), _cdiv(g.N, 128), _cdiv(g.K, 16)
    G = min(G, tiles_m * tiles_n * nk)
    edge = bool(g.M % 256 or g.N % 128 or g.n_store)
    ktail = bool(g.K % 16 or g.N % 4)
    buf = _kloop_takes(g, 1, ktail, False, kn)
    prio = bool(not edge and not ktail and kn.prio_period)
    return Launch(K_STREAMK, 256, 128, 16, -1, _flags(False, edge, ktail, prio, buf), 1, G, 1, 0)


def dmas_plan(shape, m, n, k, batch, S, cus=256):
    """launch_dmas's own arithmetic: (S after the clamp loop, chunk length Kc, tiles) or None where it returns 1 (does not apply)."""
    if shape < 0 or shape > 5 or shape == 4 or n < 4 or k < 4:
        return None
    bm, bn, bk = DMAS_BM[shape], DMAS_BN[shape], DMAS_BK[shape]
    tiles = _cdiv(m, bm) * _cdiv(n, bn)
    if S < 1 or S & (S - 1) or S > DMAS_MAX_S[shape]:
        return None
    Kc = _cdiv(_cdiv(k, S), bk) * bk
    while S > 1 and (Kc < 64 or (S - 1) * Kc >= k):
        S >>= 1
        Kc = _cdiv(_cdiv(k, S), bk) * bk
    if S > 1 and (tiles * S * batch > cus * (1 if shape == 3 else 2) or tiles * batch > 256):
        return None
    return S, (Kc if S > 1 else _cdiv(k, bk) * bk), tiles


def _launch_dmas(shape, g, batch, S, kn):
    if g.K_last:
        return None
    plan = dmas_plan(shape, g.M, g.N, g.K, batch, S, kn.cus)
    if plan is None:
        return None
    S, _, tiles = plan
    bm, bn, bk = DMAS_BM[shape], DMAS_BN[shape], DMAS_BK[shape]
    swizzle = bool(kn.mid_swizzle and S == 1 and _cdiv(g.M, bm) >= 8 and tiles >= 64)
    edge = bool(g.M % bm or g.N % bn or g.n_store)
    ktail = bool(g.K % bk or g.N % 4)
    ran = 5 if shape == 2 and kn.mid_waves and S == 1 and (edge or ktail) else shape      # the DmasShape5 swap
    return Launch(K_DMAS, bm, bn, bk, ran, _flags(False, edge, ktail, swizzle=swizzle), S, tiles * S, batch, 0)


def _launch_kq(shape, g, batch, vec, kn):
    if shape < 0 or shape >= len(KQ_SHAPES) or g.K < 4 or (g.K_last and g.K_last < 4) or g.n_store:
        return None
    bm, bn = 16 * KQ_SHAPES[shape][0], 16 * KQ_SHAPES[shape][1]
    tiles_m, tiles = _cdiv(g.M, bm), _cdiv(g.M, bm) * _cdiv(g.N, bn)
    if (g.M * g.lda + g.K) * 4 >= 1 << 32 or (g.K * g.ldb + g.N) * 4 >= 1 << 32:
        return None
    swizzle = tiles_m >= 8 and tiles >= 64
    grid_x, grid_z, k_chunks = tiles, batch, g.k_chunks
    if k_chunks:
        if k_chunks != batch:
            k_chunks = 0
        else:
            swizzle, grid_x, grid_z = False, tiles * batch, 1
    edge = bool(g.M % bm or g.N % bn)
    return Launch(K_KQ, bm, bn, 64, shape, _flags(vec, edge or not vec, swizzle=swizzle, chunk_major=bool(k_chunks)), k_chunks or 1, grid_x, grid_z,
                  g.K_last)


def _launch_cfg(cfg, g, batch, vec, kn):
    """launch_cfg: the k-quartered tiles fall back on the 64 x 64 LDS-DMA tiles, those on the register-staged kernel of their size."""
    if cfg >= FIRST_KQ_CFG:
        rec = _launch_kq(cfg - FIRST_KQ_CFG, g, batch, vec, kn)
        if rec is not None:
            return rec
        cfg = FIRST_MID_CFG + 2
    if cfg >= FIRST_MID_CFG:
        rec = _launch_dmas(cfg - FIRST_MID_CFG, g, batch, 1, kn)
        if rec is not None:
            return rec
        cfg = 1 if cfg == FIRST_MID_CFG else 2
    if cfg == 0:
        return _launch_dma(g, batch, vec, kn)
    return _launch_tile(g, batch, vec, *((128, 128) if cfg == 1 else (64, 64)), 16)


def split_chunk_length(cfg, k, chunks):
    """The chunk length Kc behind a split-K plan of `chunks` chunks: plan_sgemm tries S = 2 .. 8, 16, 32 .. and rounds ceil(K / S) up
    to the K-tile (16; the k-quartered tiles 64); the plan keeps ceil(K / Kc) chunks.  Refuses where two S give that count with
    different lengths (the cost model would have to say which)."""
    unit = 64 if cfg >= FIRST_KQ_CFG else 16
    found = set()
    S = 2
    while S <= 256:
        Kc = _cdiv(_cdiv(k, S), unit) * unit
        if _cdiv(k, Kc) == chunks:
            found.add(Kc)
        S = S + 1 if S < 8 else S * 2
    if len(found) != 1:
        raise ValueError("split_chunk_length: %d chunks of K = %d: candidates %s" % (chunks, k, sorted(found)))
    return found.pop()


def _launch_plan(cfg, tail_rows, S, g, batch, vec, kn, Kc=None):
    """launch_plan -> (records, folded)."""
    if tail_rows == 0 and cfg >= FIRST_MID_CFG and S > 1:
        rec = _launch_dmas(cfg - FIRST_MID_CFG, g, batch, S, kn)
        if rec is not None:
            return [rec], False
    if tail_rows == 0:
        return [_launch_cfg(cfg, g, batch, vec, kn)], False
    bm = CFG_TILES[cfg][0]
    tm = _cdiv(g.M, bm)
    m1 = (tm - tail_rows) * bm
    m2 = g.M - m1
    records = []
    if m1:
        records.append(_launch_cfg(cfg, g.copy(M=m1), 1, vec, kn))
    if Kc is None:
        Kc = split_chunk_length(cfg, g.K, S)
    full, rem = divmod(g.K, Kc)
    chunks = full + (1 if rem else 0)
    part = g.copy(M=m2, K=Kc, K_last=rem, sa=Kc, sb=Kc * g.ldb, k_chunks=chunks if cfg >= FIRST_KQ_CFG and kn.chunk_major else 0)
    records.append(_launch_cfg(cfg, part, chunks, vec and rem % 4 == 0, kn))
    return records, True


def _pad_copy(items, row_length, kn):
    return Launch(K_PAD_COPY, 0, 0, 0, -1, 0, row_length, min(_cdiv(items, 256), kn.cus * 16), 1, 0)


def tiled_launches(kind, m, n, k, batch=1, lda=None, ldb=None, ldc=None, sa=None, sb=None, a_aligned=True, b_aligned=True, shape=None, S=1,
                   variant=None, plan=None, knobs=None):
    """The records np_sgemm_debug_last_launches must report for one product call behind launch_sgemm_ld, or None where the forced
    launcher returns 1 (the form does not apply and the call goes on to another kernel).  Returns (records, folded).

      "dma"        np_sgemm_set_variant(7) / (47: knobs.variant): launch_cfg(0), sgemm_dma_kernel — sgemm_pipe_kernel where N < 4 or K < 4
      "streamk"    (-4): launch_streamk on streamk_model's grid; None where the model gives none
      "dmas"       (-(1000 + 100 shape + S)): launch_dmas
      "kq"         (-(2000 + shape)): launch_kq on a whole product
      "kq_chunks"  (-(30000 + 1000 shape + S)): the forced K-chunked plan on k-quartered tile `shape`, through launch_plan
      "tile"       variant 1 .. 6: launch_sgemm_tile / launch_sgemm_pipe
      "sub"        np::sgemm_sub_ld
      "padded"     (-6, -3): launch_padded for K < 512, where the only plan of the padded product is one sgemm_dma_kernel launch
      "plan"       the planner's choice plan = (cfg, tail_rows, S, stream-K taken) as np_sgemm_debug_plan reports it
    """
    kn = knobs or Knobs()
    lda, ldb, ldc = lda or k, ldb or n, ldc or n
    sa = (m * lda if batch > 1 else 0) if sa is None else sa
    sb = (k * ldb if batch > 1 else 0) if sb is None else sb
    g = _G(m, n, k, lda, ldb, ldc, batch, sa, sb, a_aligned, b_aligned)
    vec = g.vec()
    if kind == "sub":
        sub_vec = k % 4 == 0 and lda % 4 == 0 and n % 4 == 0 and ldb % 4 == 0 and a_aligned and b_aligned
        return [_launch_tile(g, 1, sub_vec, 128, 128, 16, K_TILE_SUB, F_SUB)], False
    if kind == "dma":
        g.swizzle = 4 if kn.variant == 47 else 0
        if n >= 4 and k >= 4:
            return [_launch_dma(g, batch, vec, kn)], False
        return [_launch_tile(g, batch, vec, 128, 128, 16, K_PIPE, F_PIPE_MODE1)], False
    if kind == "tile":
        if variant in (5, 6):
            return [_launch_tile(g, batch, vec, 128, 128, 16, K_PIPE, F_PIPE_MODE1 if variant == 6 else 0)], False
        bm, bn, bk = {1: (128, 128, 16), 2: (128, 128, 32), 3: (128, 128, 16), 4: (64, 64, 16)}[variant]
        return [_launch_tile(g, batch, vec, bm, bn, bk)], False
    if kind == "dmas":
        rec = _launch_dmas(shape, g, batch, S, kn)
        return None if rec is None else ([rec], False)
    if kind == "kq":
        rec = _launch_kq(shape, g, batch, vec, kn)
        return None if rec is None else ([rec], False)
    if kind == "kq_chunks":
        if not (S >= 2 and batch == 1 and k >= 512 and ldb == n and ldc == n):
            return None
        Kc = _cdiv(_cdiv(k, S), 64) * 64
        chunks = _cdiv(k, Kc)
        if chunks < 2 or k - (chunks - 1) * Kc < 4:
            return None
        return _launch_plan(FIRST_KQ_CFG + shape, _cdiv(m, 16 * KQ_SHAPES[shape][0]), chunks, g, 1, vec, kn, Kc)
    if kind == "streamk":
        G = streamk_grid(m, n, k, kn.cus)
        return ([_launch_streamk(g, G, kn)], False) if G else None
    if kind == "padded":
        Kp, Np = _cdiv(k, 16) * 16, _cdiv(n, 4) * 4
        if vec or batch != 1 or k >= 512 or streamk_grid(m, Np, Kp, kn.cus):
            raise ValueError("tiled_launches: the padded form restated here is one matrix, not float4-loadable, K < 512, no stream-K")
        q = g.copy(K=Kp, N=Np, lda=Kp, ldb=Np, n_store=n, a_aligned=True, b_aligned=True)
        return [_pad_copy(m * Kp // 4, Kp, kn), _pad_copy(Kp * Np // 4, Np, kn), _launch_dma(q, 1, True, kn)], False
    if kind == "plan":
        cfg, tail_rows, chunks, streamk = plan
        if streamk:
            return [_launch_streamk(g, streamk_grid(m, n, k, kn.cus), kn)], False
        return _launch_plan(int(cfg), int(tail_rows), int(chunks), g, batch, vec, kn)
    raise ValueError("tiled_launches: unknown kind %r" % (kind,))
