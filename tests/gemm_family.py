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
