"""What the exact product tests share (tests/test_gpu_gemm_exact.py: the thin, few-row and matrix-vector kernels;
tests/test_gpu_gemm_tiled_exact.py: everything behind launch_sgemm_ld): the device handle with its probes, the variant setter that
is always put back, operands uploaded once per float offset, and the two runners.

run()        one dense product or matrix-vector product at every offset pair: bits, frame, a second call, the whole path mask.
run_tiled()  the same discipline for the tiled kernels: batches with gaps, windows (lda, ldb, ldc), the subtracting epilogue, and
             the whole list of launch records of np_sgemm_debug_last_launches."""
import contextlib
import ctypes as C

import numpy as np

from numpower_amd import _lib
from tests import gemm_family as gf

DIAGONAL = ((0, 0), (3, 3))
ALL_OFFSETS = tuple((a, b) for a in range(4) for b in range(4))


class Dev:
    def __init__(self, hip):
        self.L = _lib.load()
        cus = C.c_int()
        _lib.check(self.L.np_debug_cus(C.byref(cus)))
        assert cus.value == 256, "the masks of this module are written for 256 CUs; np_debug_cus reports %d" % cus.value

    def upload(self, image):
        buf = _lib.DeviceBuffer(image.nbytes)
        assert buf.ptr % 16 == 0
        _lib.check(self.L.np_memcpy_h2d(buf.ptr, image.ctypes.data, image.nbytes))
        return buf

    def download(self, buf, count):
        out = np.empty(count, np.float32)
        _lib.check(self.L.np_memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes))
        return out

    def last_path(self):
        mask = C.c_uint()
        _lib.check(self.L.np_sgemm_debug_last_path(C.byref(mask)))
        return mask.value


@contextlib.contextmanager
def sgemm_variant(dev, code, back):
    _lib.check(dev.L.np_sgemm_set_variant(code))
    try:
        yield
    finally:
        _lib.check(dev.L.np_sgemm_set_variant(back))


class Placed:
    """One operand uploaded at each float offset asked for, once."""

    def __init__(self, dev, array):
        self.dev, self.array, self.at = dev, array, {}

    def ptr(self, offset):
        if offset not in self.at:
            image, start = gf.framed(self.array, offset)
            self.at[offset] = (self.dev.upload(image), start)
        buf, start = self.at[offset]
        return buf.ptr + 4 * start

    def free(self):
        for buf, _ in self.at.values():
            buf.free()


def run(dev, A, B, want, mask, offsets=DIAGONAL, gemv=False, cls=None, label=""):
    """C = A . B (np_sgemm) or y = A . x (np_sgemv, B a vector) at every offset pair: bits against `want` (where cls is given: the
    class of every element against cls, bits wherever the class is not NaN), the frame, a second call, the whole mask, np_sync.
    mask: a value, a function of the two offsets where it depends on the alignment, or a frozenset of values where the planner's
    own model decides between them."""
    m, k = A.shape
    n = 1 if gemv else B.shape[1]
    pa, pb = Placed(dev, A), Placed(dev, B)
    image, start = gf.canary(m * n)
    cbuf = dev.upload(image)
    try:
        for oa, ob in offsets:
            tag = "%s %s offsets A %d, B %d" % (label, (m, n, k), oa, ob)
            a_ptr, b_ptr = pa.ptr(oa), pb.ptr(ob)
            runs = []
            for _ in range(2):
                _lib.check(dev.L.np_memcpy_h2d(cbuf.ptr, image.ctypes.data, image.nbytes))
                if gemv:
                    _lib.check(dev.L.np_sgemv(m, k, a_ptr, b_ptr, cbuf.ptr + 4 * start))
                else:
                    _lib.check(dev.L.np_sgemm(m, n, k, a_ptr, b_ptr, cbuf.ptr + 4 * start))
                got_mask = dev.last_path()
                assert dev.L.np_sync() == 0, tag
                host = dev.download(cbuf, image.size)
                assert gf.frame_intact(host, start, m * n), tag + ": wrote outside C"
                runs.append(host[start:start + m * n].reshape(want.shape).copy())
                expect_mask = mask(oa, ob) if callable(mask) else mask
                if isinstance(expect_mask, frozenset):
                    assert got_mask in expect_mask, "%s: ran %s, the case names one of %s" % (
                        tag, gf.describe(got_mask), sorted(map(gf.describe, expect_mask)))
                else:
                    assert got_mask == expect_mask, "%s: ran %s, the case names %s" % (tag, gf.describe(got_mask), gf.describe(expect_mask))
            got = runs[0]
            assert (gf.bits(got) == gf.bits(runs[1])).all(), tag + ": two calls differ"
            if cls is None:
                bad = np.argwhere(gf.bits(got) != gf.bits(want))
                assert bad.size == 0, "%s: %d elements differ, first at %s: got %r, exact %r" % (
                    tag, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
            else:
                assert (gf.classify(got) == cls).all(), "%s: class map differs at %s" % (tag, np.argwhere(gf.classify(got) != cls)[:4].tolist())
                keep = cls != gf.NAN
                assert (gf.bits(got)[keep] == gf.bits(want)[keep]).all(), tag + ": a finite / infinite element differs"
    finally:
        cbuf.free()
        pa.free()
        pb.free()


_OPERANDS = {}


def exact_operands(m, n, k, seed=7):
    """A, B, A . B for one shape; A is the first m rows of the largest A generated for (k, seed) so far, B one draw per (k, n)."""
    amp = gf.amp_for(k)
    key = (n, k, seed)
    if key not in _OPERANDS or _OPERANDS[key][0].shape[0] < m:
        _OPERANDS.clear()                      # one (n, k) at a time: the big shapes are hundreds of MB
        _OPERANDS[key] = gf.operands(m, n, k, seed, amp, amp)
    A, B = _OPERANDS[key]
    A = A[:m]
    return A, B, gf.expected(A, B)


def with_specials(dev, m, n, k, mask, seam, gemv=False, label=""):
    """Every specials() kind at the first, the last and one boundary position of K, at the row / column edges."""
    seams = gf.k_seams(k)
    assert seam in seams and 0 < seam < k - 1
    amp = gf.amp_for(k)
    A, B = gf.operands(m, n, k, 21, amp, amp)
    if gemv:
        B = B[:, 0].copy()
    base = gf.expected(A, B)
    for ks, i, j in ((seams[0], 0, 0), (seams[-1], m - 1, n - 1), (seam, m - 1, 0)):
        for kind in gf.SPECIAL_KINDS:
            A2, B2, cls, want = gf.specials(A, B, kind, ks, i, j, ks2=(ks + k // 2) % k, base=base)
            run(dev, A2, B2, want, mask, ((0, 0),), gemv=gemv, cls=cls, label="%s special %d at k = %d" % (label, kind, ks))


# ---- the tiled kernels ------------------------------------------------------------------------------------------------------------
# what every np_sgemm_set_variant setter is put back to (include/np_hip_debug.h)
VARIANT_DEFAULTS = (0, -2, -7, -10, -13, -15, -17, -19, -21, -23, -26, -28, -30, -33, -116, -999, -30000)


@contextlib.contextmanager
def variants(dev, *codes):
    """np_sgemm_set_variant(code) for every code, in order; every setter back to its default afterwards, whatever happened."""
    try:
        for code in codes:
            _lib.check(dev.L.np_sgemm_set_variant(code))
        yield
    finally:
        for code in VARIANT_DEFAULTS:
            _lib.check(dev.L.np_sgemm_set_variant(code))


def last_launches(L, capacity=gf.LAUNCH_KEPT):
    """(records, count) of np_sgemm_debug_last_launches into room for `capacity` records: min(count, kept, capacity) records are
    written and not a word behind them (the buffer is one record longer and pre-filled), the count is that of the launches made."""
    fill = 0xdeadbeef
    words = (C.c_uint * (gf.LAUNCH_WORDS * (capacity + 1)))(*([fill] * (gf.LAUNCH_WORDS * (capacity + 1))))
    count = C.c_uint()
    _lib.check(L.np_sgemm_debug_last_launches(words, capacity, C.byref(count)))
    kept = min(count.value, gf.LAUNCH_KEPT, capacity)
    assert all(w == fill for w in words[kept * gf.LAUNCH_WORDS:]), "np_sgemm_debug_last_launches wrote behind record %d" % kept
    return [gf.Launch.decode(words[i * gf.LAUNCH_WORDS:(i + 1) * gf.LAUNCH_WORDS]) for i in range(kept)], count.value


def layout(rows, cols, ld, batch, gap, offset, pad):
    """(size, start, stride, index): `batch` matrices of rows x cols, rows ld floats apart, matrices rows . ld + gap apart, the first
    element at float pad + offset of a buffer with `pad` more floats behind the last one; index[b, i, j] = its place."""
    if pad % 4 or not 0 <= offset <= 3 or ld < cols:
        raise ValueError("layout: pad a multiple of 4, offset 0 .. 3 floats, ld >= cols")
    stride = rows * ld + gap
    start = pad + offset
    index = start + (np.arange(batch)[:, None, None] * stride + np.arange(rows)[None, :, None] * ld + np.arange(cols)[None, None, :])
    return start + (batch - 1) * stride + (rows - 1) * ld + cols + pad, start, stride, index


def run_tiled(dev, A, B, want, records, offsets=DIAGONAL, mask=gf.TILED, lda=None, ldb=None, ldc=None, gaps=(0, 0, 0), c0=None, cls=None,
              label=""):
    """C = A . B behind launch_sgemm_ld — or C = C0 - A . B where c0 is given (np_sgemm_debug_sub_ld) — at every offset pair of A and
    B.  A (batch x m x k) and B (batch x k x n) (or 2-D: one matrix) lie at float offsets inside NaN: the pads, the row gaps of a
    window (lda > k, ldb > n) and the gaps between the matrices of a batch all hold NaN.  C lies inside -777: pads, row gaps
    (ldc > n) and batch gaps; its own elements hold NaN (or C0).  After the call the WHOLE image of C is compared bit for bit with
    the expected one (want where the kernel must write, -777 everywhere else; where cls is given, NaN elements by class), twice,
    the two runs with each other; the whole list of launch records, their count and the mask are asserted, and np_sync is clean.
    records: the expected list, or a function of the two offsets where it depends on the alignment."""
    A3, B3 = (A if A.ndim == 3 else A[None]), (B if B.ndim == 3 else B[None])
    batch, m, k = A3.shape
    n = B3.shape[2]
    want3 = want.reshape(batch, m, n)
    window = lda is not None or ldb is not None or ldc is not None
    lda, ldb, ldc = lda or k, ldb or n, ldc or n
    L = dev.L
    size_c, start_c, stride_c, at_c = layout(m, n, ldc, batch, gaps[2], 0, 1024)
    image = np.full(size_c, gf.CANARY, np.float32)
    image[at_c] = np.nan if c0 is None else c0.reshape(batch, m, n)
    expect = image.copy()
    expect[at_c] = want3
    nan_ok = np.isnan(expect)
    assert cls is not None or c0 is not None or not nan_ok.any()
    cbuf = dev.upload(image)
    placed = {}

    def place(which, mat, ld, gap, offset):
        if (which, offset) not in placed:
            size, start, stride, at = layout(mat.shape[1], mat.shape[2], ld, batch, gap, offset, 64)
            host = np.full(size, np.nan, np.float32)
            host[at] = mat
            placed[which, offset] = (dev.upload(host), start, stride)
        buf, start, stride = placed[which, offset]
        return buf.ptr + 4 * start, stride

    try:
        for oa, ob in offsets:
            tag = "%s %s batch %d ld (%d, %d, %d) gaps %s offsets A %d, B %d" % (label, (m, n, k), batch, lda, ldb, ldc, gaps, oa, ob)
            a_ptr, sa = place("A", A3, lda, gaps[0], oa)
            b_ptr, sb = place("B", B3, ldb, gaps[1], ob)
            c_ptr = cbuf.ptr + 4 * start_c
            expect_records = records(oa, ob) if callable(records) else records
            runs = []
            for _ in range(2):
                _lib.check(L.np_memcpy_h2d(cbuf.ptr, image.ctypes.data, image.nbytes))
                if c0 is not None:
                    assert batch == 1
                    _lib.check(L.np_sgemm_debug_sub_ld(m, n, k, a_ptr, lda, b_ptr, ldb, c_ptr, ldc))
                elif window:
                    assert batch == 1
                    _lib.check(L.np_sgemm_debug_ld(m, n, k, a_ptr, lda, b_ptr, ldb, c_ptr, ldc))
                elif batch > 1:
                    _lib.check(L.np_sgemm_strided_batched(batch, m, n, k, a_ptr, sa, b_ptr, sb, c_ptr, stride_c))
                else:
                    _lib.check(L.np_sgemm(m, n, k, a_ptr, b_ptr, c_ptr))
                got_records, count = last_launches(L)
                assert last_launches(L, 1) == (got_records[:1], count) and last_launches(L, 0) == ([], count), tag      # the count is exact whatever is kept
                got_mask = dev.last_path()
                rc = L.np_sync()
                assert rc == 0, "%s: np_sync returned %d" % (tag, rc)
                runs.append(dev.download(cbuf, image.size))
                assert count == len(expect_records) and got_records == expect_records[:gf.LAUNCH_KEPT], "%s: %d launches %r, the case names %r" % (
                    tag, count, got_records, expect_records)
                assert got_mask == mask, "%s: ran %s, the case names %s" % (tag, gf.describe(got_mask), gf.describe(mask))
            got = runs[0]
            assert (gf.bits(got) == gf.bits(runs[1])).all(), tag + ": two calls differ"
            bad = np.flatnonzero((gf.bits(got) != gf.bits(expect)) & ~(nan_ok & np.isnan(got)))
            if bad.size:
                inside = np.isin(bad[:1], at_c.reshape(-1))[0]
                where = tuple(int(v) for v in np.argwhere(at_c == bad[0])[0]) if inside else "outside C"
                raise AssertionError("%s: %d floats of C's buffer differ, first at float %d (%s): got %r, exact %r" % (
                    tag, bad.size, bad[0], where, got[bad[0]], expect[bad[0]]))
    finally:
        cbuf.free()
        for buf, _, _ in placed.values():
            buf.free()
