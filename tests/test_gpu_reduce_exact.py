"""The device reductions against the exact family (tests/reduce_family.py): every output of every case is compared BIT FOR BIT
with a value computed in integer arithmetic, on inputs where a dropped, doubled or misplaced element always changes the
result, and every case asserts through np_debug_reduce_last_path / np_debug_chain_reduce_last_path that the kernel family it
was written for is the one that ran.

The expected path of a shape is worked out by plan_axis() / plan_all() below: launch_reduce_axis / launch_reduce_all of
np_reduce.hip restated as host arithmetic over the CU count the library reports (np_debug_cus).  A case that NAMES a branch
asserts that branch's bit; where the machine at hand plans the listed shape elsewhere (more CUs), the shape grows until the
plan shows the branch, and the shape used is printed.  A planner change that moves a shape off its path fails here twice: the
restated plan no longer matches the probe, and the named bit is gone.

Through the C ABI (np_reduce_axis, np_reduce_all(_dev), np_fused_chain_reduce*, np_weighted_sums, np_all, np_count_mismatch),
a subset again through NDArray.  NaN / Inf: specials() of the family; min / max follow the reference's rule (np_hip.h,
np_reduce_op): NaN exactly where position 0 of the slice is NaN."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from numpower_amd import _lib
from tests import reduce_family as rf

pytestmark = pytest.mark.gpu

# NP_REDUCE_PATH_* / NP_CHAIN_PATH_* of include/np_hip_debug.h (tests/test_reduce_reference_cpu.py pins the header's side)
ROWS_BLOCK, ROWS_BLOCK_CHUNKED, ROWS_STAGED, ROWS_GROUP, ROWS_WAVE = 0x1, 0x2, 0x4, 0x8, 0x10
COLS_ONE, COLS_TWO, COLS_RECURSE, COLS_XCD, SMALL_INNER, SMALL_INNER_V4 = 0x20, 0x40, 0x80, 0x100, 0x200, 0x400
GENERIC, GENERIC_CHUNKED, ALL_ONE, ALL_TWO = 0x800, 0x1000, 0x2000, 0x4000
CH_FLAT, CH_STATIC_FLAT, CH_ROWS, CH_ROWS_STAGED, CH_STATIC_ROWS = 0x1, 0x2, 0x4, 0x8, 0x10
CH_COLS, CH_STATIC_COLS, CH_SPLIT, CH_TEMPORARY = 0x20, 0x40, 0x80, 0x100


def _ceil(a, b):
    return (a + b - 1) // b


def choose_splits(outer, n, inner4, cus):
    base = _ceil(inner4, 64) * outer
    target = cus * 8 * 3 // 2
    if base >= target:
        return 1
    s = max(1, min(_ceil(target, base), max(n // 64, 1), 65535))
    t = s
    while t > 1 and t + 16 > s:
        if _ceil(n, t) % 2 == 1:
            return t
        t -= 1
    return s


def plan_axis(outer, n, inner, ptr, cus):
    """launch_reduce_axis (np_reduce.hip) as arithmetic: the probe mask of np_reduce_axis on an outer x n x inner array at
    address `ptr` (only its alignment matters; partials are pool blocks, aligned)."""
    target_wg = cus * 8
    if inner == 1:
        if n >= 4096:
            chunks = 1
            if outer < target_wg:
                chunks = max(1, min(_ceil(target_wg, outer), n // 2048, 65535))
            if chunks == 1:
                return ROWS_BLOCK
            chunk_len = _ceil(_ceil(n, chunks), 4) * 4
            return ROWS_BLOCK_CHUNKED | plan_axis(outer, _ceil(n, chunk_len), 1, 0, cus)
        if 4 < n <= 48 and outer * n >= (8 << 20) and ptr % 16 == 0:
            pitch = n | 1
            if max(256, (8192 // pitch) // 256 * 256) * pitch * 4 <= 64 * 1024:
                return ROWS_STAGED
        if 4 < n <= 256:
            return ROWS_GROUP
        if n >= 32:
            return ROWS_WAVE
    elif (inner % 4 == 0 or inner >= 4000) and outer <= 65535 and not (inner <= 128 and n >= 512 and outer * inner < target_wg * 64):
        inner4 = _ceil(inner, 4)
        splits = choose_splits(outer, n, inner4, cus)
        m = COLS_XCD if ((inner * 4) % 128 != 0 or ptr % 128 != 0) and _ceil(inner4, 64) > 1 else 0
        if splits == 1:
            return m | COLS_ONE
        if splits >= 256:
            return m | COLS_RECURSE | plan_axis(outer, splits, inner, 0, cus)
        return m | COLS_TWO
    elif inner <= 128 and n >= 512 and outer <= 65535 and outer * inner < target_wg * 64:
        blocks = max(1, min(target_wg // outer, n // 256))
        rows_per_block = _ceil(n, blocks)
        v4 = ptr % 16 == 0 and (outer == 1 or (n * inner) % 4 == 0)
        if v4:
            rows_per_block = _ceil(rows_per_block, 4) * 4
        return (SMALL_INNER_V4 if v4 else SMALL_INNER) | plan_axis(outer, _ceil(n, rows_per_block), inner, 0, cus)
    outputs, target_threads, chunks = outer * inner, cus * 2048, 1
    if outputs < target_threads and n >= 128:
        chunks = max(1, min(_ceil(target_threads, outputs), n // 32))
    chunks = _ceil(n, _ceil(n, chunks))
    if chunks == 1:
        return GENERIC
    return GENERIC_CHUNKED | plan_axis(outer, chunks, inner, 0, cus)


def plan_all(n, ptr, cus):
    """launch_reduce_all: one launch (the last workgroup folds) up to 256 workgroups, and up to 2^20 elements on at most 128."""
    head = min(n, ((16 - ptr % 16) % 16) // 4)
    nvec = (n - head) // 4
    wanted, cap = _ceil(nvec, 256), cus * 8
    blocks = max(1, wanted) if wanted <= cap else cap | 1
    if n <= (1 << 20) and blocks > 128:
        blocks = 128
    return ALL_ONE if blocks <= 256 else ALL_TWO


# ---- device plumbing -------------------------------------------------------------------------------------------------------

class Dev:
    def __init__(self, hip):
        self.D, self.L = hip, _lib.load()
        cus = C.c_int()
        _lib.check(self.L.np_debug_cus(C.byref(cus)))
        self.cus = cus.value

    def upload(self, x, offset=0):
        """x at `offset` floats into a fresh allocation -> (allocation, view)"""
        flat = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        d = self.D.DeviceArray((flat.size + 4,))
        assert d.ptr % 128 == 0
        v = d.view(offset, flat.shape)
        _lib.check(self.L.np_memcpy_h2d(v.ptr, flat.ctypes.data, flat.nbytes))
        return d, v

    @contextlib.contextmanager
    def held(self, x, offset=0):
        """`with dev.held(x, offset) as view`: upload(), freed on the way out, also after a failed assertion"""
        d, v = self.upload(x, offset)
        try:
            yield v
        finally:
            d.free()

    def poke(self, v, index, value):
        one = np.array([value], np.float32)
        _lib.check(self.L.np_memcpy_h2d(v.ptr + 4 * int(index), one.ctypes.data, 4))

    def mask(self, chain=False):
        m = C.c_uint()
        _lib.check((self.L.np_debug_chain_reduce_last_path if chain else self.L.np_debug_reduce_last_path)(C.byref(m)))
        return m.value

    def reduce_axis(self, op, v, outer, n, inner):
        out = self.D.DeviceArray((outer * inner,))
        _lib.check(self.L.np_reduce_axis(_lib.REDUCE_OPS[op], v.ptr, outer, n, inner, out.ptr, 0))
        got = out.to_host()
        out.free()
        return got, self.mask()

    def reduce_all(self, op, v, n, dev=False):
        if dev:
            out = self.D.DeviceArray((1,))
            _lib.check(self.L.np_reduce_all_dev(_lib.REDUCE_OPS[op], v.ptr, n, out.ptr))
            got = out.to_host()[0]
            out.free()
        else:
            r = C.c_float()
            _lib.check(self.L.np_reduce_all(_lib.REDUCE_OPS[op], v.ptr, n, C.byref(r)))
            got = np.float32(r.value)
        return got, self.mask()

    def chain(self, how, op, v, rows, cols, axis=None):
        """the one-step chain v * 1.0 (flags = 0: plain IEEE, no bit of v changes), reduced: how = host / dev (full) or axis.
        (`positive` would not do: it is |x| here, as in the reference's double_math.c:241-244.)"""
        one = C.c_float(1.0)
        inputs = (C.c_void_p * 2)(v.ptr, C.cast(C.pointer(one), C.c_void_p))
        kinds = (C.c_int * 2)(_lib.NP_FULL, 4)      # NP_HOST_SCALAR
        ops = (_lib.FusedOp * 1)(_lib.FusedOp(_lib.NP_FUSED_BINARY, _lib.BINARY_OPS["multiply"], 1, 0, 0.0, 0.0, 0, 0))
        rop = _lib.REDUCE_OPS[op]
        if how == "host":
            r = C.c_float()
            _lib.check(self.L.np_fused_chain_reduce(inputs, kinds, 2, ops, 1, rop, rows, cols, C.byref(r)))
            got = np.float32(r.value)
        else:
            out = self.D.DeviceArray((1 if how == "dev" else (rows if axis == 1 else cols),))
            if how == "dev":
                _lib.check(self.L.np_fused_chain_reduce_dev(inputs, kinds, 2, ops, 1, rop, rows, cols, out.ptr))
            else:
                _lib.check(self.L.np_fused_chain_reduce_axis(inputs, kinds, 2, ops, 1, rop, rows, cols, axis, out.ptr))
            got = out.to_host()
            out.free()
            if how == "dev":
                got = got[0]
        return got, self.mask(chain=True)


@pytest.fixture(scope="module")
def dev(hip):
    return Dev(hip)


def _check(got, want, what, either_zero=None):
    bad = rf.mismatches(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1), either_zero)
    assert bad.size == 0, "%s: %d of %d outputs differ, first at %d: got %r want %r" % (
        what, bad.size, np.asarray(want).size, bad[0], np.asarray(got).reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])


def _amp(n):
    return 4 if n <= (1 << 20) else 3


# ---- np_reduce_axis --------------------------------------------------------------------------------------------------------

def run_axis_case(dev, outer, n, inner, offset, named, label, reduce=None, probe=True):
    """All five ops over an outer x n x inner array `offset` floats into its allocation: ints (sum, mean, min, max), prods (prod,
    min, max), extremes (min, max at every seam position, dealt over the outputs and over rounds), specials on both (every op,
    twice).  `reduce(op, view) -> (values, mask)` defaults to np_reduce_axis, whose mask must equal the restated plan and hold
    the `named` bits."""
    shape, axis = (outer, n, inner), 1
    if reduce is None:
        def reduce(op, v):
            return dev.reduce_axis(op, v, outer, n, inner)
    pos = rf.positions(n)

    def go(x, ops, what):
        d, v = dev.upload(x, offset)
        try:
            if probe:
                want_mask = plan_axis(outer, n, inner, v.ptr, dev.cus)
                assert want_mask & named == named, "%s: the plan %#x does not hold the named path %#x" % (label, want_mask, named)
            for op in ops:
                raw, mask = reduce(op, v)
                if probe:
                    assert mask == want_mask, "%s %s: probe %#x, restated plan %#x" % (label, op, mask, want_mask)
                got, want = np.asarray(raw).reshape(-1), rf.expected(x, axis, op).reshape(-1)
                _check(got, want, "%s %s %s" % (label, what, op))
                if what.startswith("specials"):
                    again, _ = reduce(op, v)
                    assert np.array_equal(rf.bits(again), rf.bits(raw)), "%s %s %s: two runs differ" % (label, what, op)
        finally:
            d.free()

    big = outer * n * inner > (1 << 21)      # (large arrays: min / max from the extremes alone — every expectation is a pass on the host)
    xi = rf.ints(shape, 1000 + n, _amp(n), axis)
    go(xi, ("sum", "mean") if big else ("sum", "mean", "min", "max"), "ints")
    xp = rf.prods(shape, axis, 2000 + n)
    go(xp, ("prod",) if big else ("prod", "min", "max"), "prods")
    bg = None
    for rnd in range(min(rf.extreme_rounds(shape, axis, pos), 256)):
        xe, bg = rf.extremes(shape, axis, pos, 3000 + n, rnd, bg)
        go(xe, ("min", "max"), "extremes round %d" % rnd)
    outputs = outer * inner
    for rnd in range(1 if outputs >= 2 * len(rf.SPECIAL_KINDS) else len(rf.SPECIAL_KINDS)):
        xs, kinds = rf.specials(xi, axis, pos, 0, rnd)
        go(xs, ("sum", "mean", "min", "max"), "specials(ints) round %d" % rnd)
        xs, kinds = rf.specials(xp, axis, pos, 1, rnd)
        go(xs, ("prod",), "specials(prods) round %d" % rnd)
    if n >= 2 and not big:
        xz = rf.zero_extremes(shape, axis, 4000 + n)
        d, v = dev.upload(xz, offset)
        try:
            got, _ = reduce("min", v)
            _check(got, rf.expected(xz, axis, "min"), label + " zero minimum", np.ones(outputs, bool))
        finally:
            d.free()
        d, v = dev.upload(-xz, offset)
        try:
            got, _ = reduce("max", v)
            _check(got, rf.expected(-xz, axis, "max"), label + " zero maximum", np.ones(outputs, bool))
        finally:
            d.free()


def grown(dev, outer, n, inner, offset, named, grow):
    """The listed shape, or — where this machine plans it elsewhere — the first of its multiples along dimension `grow` whose
    plan holds `named`."""
    shape = [outer, n, inner]
    for _ in range(6):
        if plan_axis(shape[0], shape[1], shape[2], 4 * offset, dev.cus) & named == named:
            break
        assert grow is not None, "shape %r is not planned onto %#x with %d CUs" % (shape, named, dev.cus)
        shape[grow] = shape[grow] * 2 + (shape[grow] % 2)
    else:
        raise AssertionError("no multiple of the shape reaches path %#x with %d CUs" % (named, dev.cus))
    if shape != [outer, n, inner]:
        print("shape grown for %d CUs: %r -> %r" % (dev.cus, (outer, n, inner), tuple(shape)))
    return tuple(shape)


ROW_COUNTS = (1, 3, 255, 256, 257, 3001)

# (outer, n, inner, offset in floats, named path, dimension to grow on a larger machine)
AXIS_CASES = [
    # inner == 1 -------------------------------------------------------------------------------------
    *[(rows, n, 1, 0, GENERIC, None) for n in (1, 2, 3, 4) for rows in (1, 257)],
    *[(rows, n, 1, 0, ROWS_GROUP, None) for n in (5, 16, 17, 32, 33, 64, 65, 128, 129, 256) for rows in ROW_COUNTS],
    # ... and lengths that give EVERY lane of a group an odd number of elements (the loop's single-element tail) and the last
    # lanes one element fewer than the first, for each L = 2 .. 32 (the lengths above leave the tail to lane 0 or to nobody)
    *[(rows, n, 1, 0, ROWS_GROUP, None) for n in (6, 7, 12, 20, 23, 40, 47, 80, 95, 160, 191, 224) for rows in (3, 257)],
    *[(rows, n, 1, 0, ROWS_WAVE, None) for n in (257, 258, 511, 4095) for rows in (1, 3, 257)],
    (2048, 4096, 1, 0, ROWS_BLOCK, 0), (2048, 4099, 1, 0, ROWS_BLOCK, 0),
    (1, 4096, 1, 0, ROWS_BLOCK_CHUNKED, None), (7, 4097, 1, 0, ROWS_BLOCK_CHUNKED, None),
    (3, 300001, 1, 0, ROWS_BLOCK_CHUNKED, None), (1, 1000003, 1, 0, ROWS_BLOCK_CHUNKED, None),
    (3, 300001, 1, 1, ROWS_BLOCK_CHUNKED, None),
    (1700000, 5, 1, 0, ROWS_STAGED, None), (530003, 16, 1, 0, ROWS_STAGED, None), (174763, 48, 1, 0, ROWS_STAGED, None),
    (200000, 47, 1, 0, ROWS_STAGED, None),
    (1700000, 5, 1, 1, ROWS_GROUP, None),          # one float off alignment: must leave the staged path
    # inner > 1 --------------------------------------------------------------------------------------
    (1, 100, 4096, 0, COLS_ONE, None), (64, 100, 64, 0, COLS_ONE, None), (3072, 8, 256, 0, COLS_ONE, 0),
    (1, 300, 4096, 0, COLS_TWO, None), (1, 4001, 256, 0, COLS_TWO, None),
    (1, 20000, 200, 0, COLS_RECURSE, 1),
    (1, 300, 260, 0, COLS_XCD, None), (1, 4001, 260, 0, COLS_XCD, None), (1, 300, 4096, 1, COLS_XCD, None),
    (1, 300, 4001, 0, COLS_XCD | COLS_TWO, None), (1, 2100, 10007, 0, COLS_XCD, None),
    (1, 4001, 3, 0, SMALL_INNER_V4, None), (1, 200000, 2, 0, SMALL_INNER_V4, None), (5, 70000, 3, 0, SMALL_INNER_V4, None),
    (64, 5000, 64, 0, SMALL_INNER_V4, None),
    (2, 1001, 3, 0, SMALL_INNER, None), (1, 4001, 3, 1, SMALL_INNER, None),
    (1, 1001, 1003, 0, GENERIC, None), (7, 5, 3, 0, GENERIC, None),
    (1, 4001, 251, 0, GENERIC_CHUNKED, None), (2, 40000, 17, 0, GENERIC_CHUNKED, None),
    (1, 4001, 250, 0, GENERIC_CHUNKED, None),
    (70001, 4, 8, 0, GENERIC, None),               # outer > 65535 with inner > 1
]


def _case_id(c):
    return "%dx%dx%d+%d-%#x" % c[:5]


@pytest.mark.parametrize("case", AXIS_CASES, ids=_case_id)
def test_reduce_axis_exact(case, dev):
    outer, n, inner, offset, named, grow = case
    outer, n, inner = grown(dev, outer, n, inner, offset, named, grow)
    run_axis_case(dev, outer, n, inner, offset, named, "np_reduce_axis %dx%dx%d+%d" % (outer, n, inner, offset))


def test_misaligned_pointer_leaves_the_staged_path(dev):
    assert plan_axis(1700000, 5, 1, 0, dev.cus) == ROWS_STAGED and plan_axis(1700000, 5, 1, 4, dev.cus) == ROWS_GROUP


@pytest.mark.parametrize("shape,axis", [((257, 33), 1), ((3, 300001), 1), ((4001, 3), 0), ((300, 260), 0), ((2, 1001, 3), 1), ((1001, 1003), 0)])
def test_ndarray_axis_reductions_exact(shape, axis, hip):
    """The same family through NDArray (host layer -> C ABI): sum / mean / min / max / prod over an axis, NaN rule included."""
    from numpower_amd.ndarray import NDArray
    n = shape[axis]
    pos = rf.positions(n)
    xi = rf.ints(shape, 77, 4, axis)
    xs, _ = rf.specials(xi, axis, pos, 0, 0)
    xp = rf.prods(shape, axis, 78)
    xe, _ = rf.extremes(shape, axis, pos, 79)
    for x, ops in ((xi, ("sum", "mean", "min", "max")), (xs, ("sum", "mean", "min", "max")), (xp, ("prod",)), (xe, ("min", "max"))):
        g = NDArray.array(x).gpu()
        for op in ops:
            got = getattr(NDArray, op)(g, axis).cpu().numpy()
            _check(got, rf.expected(x, axis, op), "NDArray.%s(%r, %d)" % (op, shape, axis))


# ---- np_reduce_all / np_reduce_all_dev -------------------------------------------------------------------------------------

ALL_SIZES = [*range(1, 10), 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1,
             2 ** 20 + 5, 4200003]


def _seam_positions(n, offset):
    """element positions in the head, in the tail and in the last vector of the last workgroup of reduce_all_pass1"""
    head = min(n, (4 - offset % 4) % 4)
    nvec = (n - head) // 4
    p = set(range(head)) | set(range(head + 4 * nvec, n)) | {0, n - 1, n // 2}
    if nvec:
        p.update(range(head + 4 * (nvec - 1), head + 4 * nvec))
        p.update(range(head, head + 4))
    return sorted(q for q in p if 0 <= q < n)


@pytest.mark.parametrize("n", ALL_SIZES)
def test_reduce_all_exact(n, dev):
    xi, xp = rf.ints((n,), 500 + n, _amp(n)), rf.prods((n,), None, 600 + n)
    want_i = {op: rf.expected(xi, None, op) for op in ("sum", "mean", "min", "max")}
    want_p = {op: rf.expected(xp, None, op) for op in ("prod", "min", "max")}
    pos = rf.positions(n)
    bg = np.random.default_rng(n).uniform(-0.96875, 0.96875, n).astype(np.float32)
    bg[bg == 0.0] = 0.5
    for offset in range(4):
        label = "np_reduce_all n=%d+%d" % (n, offset)
        for x, want in ((xi, want_i), (xp, want_p)):
            with dev.held(x, offset) as v:
                want_mask = plan_all(n, v.ptr, dev.cus)
                for op in want:
                    for on_dev in (False, True):
                        got, mask = dev.reduce_all(op, v, n, on_dev)
                        _check(got, want[op], "%s %s dev=%d" % (label, op, on_dev))
                        assert mask == want_mask, "%s %s: probe %#x, restated plan %#x" % (label, op, mask, want_mask)
        # one 2.0 and one -2.0 walked over every seam position (the dealing of extremes() with a single output), poked on the device
        with dev.held(bg, offset) as v:
            seams = sorted(set(pos) | set(_seam_positions(n, offset)))
            for k, hi in enumerate(seams):
                lo = seams[(k + max(1, len(seams) // 2)) % len(seams)]
                if lo == hi:
                    lo = (hi + 1) % n
                dev.poke(v, hi, 2.0)
                if n > 1:
                    dev.poke(v, lo, -2.0)
                got, _ = dev.reduce_all("max", v, n)
                assert got == 2.0, "%s: the maximum at %d was not seen (%r)" % (label, hi, got)
                got, _ = dev.reduce_all("min", v, n)
                assert got == (-2.0 if n > 1 else 2.0), "%s: the minimum at %d was not seen (%r)" % (label, lo, got)
                dev.poke(v, hi, bg[hi])
                dev.poke(v, lo, bg[lo])
        # specials at the seams: every kind at every seam position up to 65537 elements.  Beyond that each expectation is a pass
        # over the array on the host, so the large sizes take one offset each (n % 4: it leaves a head and, but for 2^20 itself,
        # a tail) and plant every kind twice, walking the positions of the last vector of the last workgroup and of the tail
        # behind it — the two-launch form runs at these sizes only
        if n > 65537 and offset != n % 4:
            continue
        seams = _seam_positions(n, offset)
        if n > 65537:
            head = (4 - offset % 4) % 4
            nvec = (n - head) // 4
            seams = list(range(head + 4 * (nvec - 1), n))       # the last vector and the tail behind it
        rounds = len(rf.SPECIAL_KINDS) * (len(seams) if n <= 65537 else 2)
        for rnd in range(rounds):
            for base, ops, seed in ((xi, ("sum", "mean", "min", "max"), 0), (xp, ("prod",), 3)):
                xs, kind = rf.specials(base, None, seams, seed, rnd)
                with dev.held(xs, offset) as v:
                    for op in ops:
                        got, _ = dev.reduce_all(op, v, n, rnd % 2 == 1)
                        _check(got, rf.expected(xs, None, op), "%s specials kind %d round %d %s" % (label, int(kind), rnd, op))
                        again, _ = dev.reduce_all(op, v, n, rnd % 2 == 1)
                        assert rf.bits(again) == rf.bits(got), "%s %s: two runs differ" % (label, op)


def test_reduce_all_both_launch_forms_ran(dev):
    """Both sides of the one-launch / two-launch boundary and of the n <= 2^20 workgroup cap are among ALL_SIZES."""
    masks = {n: plan_all(n, 0, dev.cus) for n in ALL_SIZES}
    assert masks[2 ** 20] == ALL_ONE and masks[4200003] == ALL_TWO and masks[1] == ALL_ONE
    if dev.cus * 8 >= 1025:
        assert masks[2 ** 20 + 5] == ALL_TWO      # 1025 workgroups: past the cap's reach by five elements


def test_ndarray_full_reductions_exact(hip):
    from numpower_amd.ndarray import NDArray
    for shape in ((9,), (257, 33), (1025, 1025)):
        n = int(np.prod(shape))
        xi = rf.ints(shape, 91, 4)
        xs, _ = rf.specials(xi, None, [0, 1, n - 1], 0, 0)      # NaN in position 0
        xl, _ = rf.specials(xi, None, [0, 1, n - 1], 1, 0)      # NaN later only
        xp = rf.prods(shape, None, 92)
        for x, ops in ((xi, ("sum", "mean", "min", "max")), (xs, ("sum", "min", "max")), (xl, ("sum", "min", "max")), (xp, ("prod",))):
            g = NDArray.array(x).gpu()
            for op in ops:
                _check(np.float32(getattr(NDArray, op)(g)), rf.expected(x, None, op), "NDArray.%s(%r)" % (op, shape))


# ---- chain reductions: the one-step chain x * 1.0 over the same family --------------------------------------------------

# (rows, cols, axis, named chain path)
CHAIN_AXIS_CASES = [
    (3001, 257, 1, CH_ROWS), (300, 4099, 1, CH_ROWS), (129, 64, 1, CH_ROWS), (5000, 256, 1, CH_ROWS),
    (3, 1000003, 1, CH_ROWS | CH_SPLIT),               # a few very long rows cut over several workgroups
    (900001, 10, 1, CH_ROWS_STAGED), (180001, 47, 1, CH_ROWS_STAGED),
    # rows of 49 ... 512 floats of an array of >= 2^23 elements that the lane groups pack badly go through the same kernel in slabs of
    # a few rows: 160 rows and a thread per row; 80 rows, 2 lanes per row; 16 rows, 16 lanes per row
    (168001, 50, 1, CH_ROWS_STAGED), (84001, 100, 1, CH_ROWS_STAGED), (16801, 501, 1, CH_ROWS_STAGED),
    (3001, 15, 1, CH_TEMPORARY), (100, 300, 1, CH_TEMPORARY),          # rows shorter than 16 floats; fewer than 128 rows of a small array
    (4001, 257, 0, CH_COLS | CH_SPLIT), (40, 4099, 0, CH_COLS), (4001, 256, 0, CH_COLS | CH_SPLIT), (40, 4096, 0, CH_COLS),
    (31, 4096, 0, CH_TEMPORARY), (4001, 31, 0, CH_TEMPORARY), (4001, 124, 0, CH_TEMPORARY),   # fewer than 32 rows / 32 column slots
]


@pytest.mark.parametrize("case", CHAIN_AXIS_CASES, ids=lambda c: "%dx%d-axis%d-%#x" % c)
def test_chain_reduce_axis_exact(case, dev):
    rows, cols, axis, named = case
    outer, n, inner = (rows, cols, 1) if axis == 1 else (1, rows, cols)
    seen = set()

    def reduce(op, v):
        got, mask = dev.chain("axis", op, v, rows, cols, axis)
        seen.add(mask)
        return got, mask
    run_axis_case(dev, outer, n, inner, 0, 0, "np_fused_chain_reduce_axis %dx%d axis %d" % (rows, cols, axis), reduce, probe=False)
    # (a sum may run as a compiled chain, np_fused_static.hip, in the same geometry: its bit stands for the interpreter's)
    as_interpreter = {(m & ~(CH_STATIC_ROWS | CH_STATIC_COLS)) | (CH_ROWS if m & CH_STATIC_ROWS else 0) | (CH_COLS if m & CH_STATIC_COLS else 0)
                      for m in seen}
    assert as_interpreter == {named} and named in seen, "chain probe %r, expected %#x" % (sorted(map(hex, seen)), named)


def test_chain_on_a_staged_shape_off_alignment_takes_the_temporary(dev):
    """The staged kernel needs input 0 on 16 bytes: one float off, the chain is stored and np_reduce_axis reduces it."""
    rows, cols = 900001, 10
    x = rf.ints((rows, cols, 1), 1900, 3, 1)
    with dev.held(x, 1) as v:
        for op in ("sum", "mean", "min", "max"):
            got, mask = dev.chain("axis", op, v, rows, cols, 1)
            _check(got, rf.expected(x, 1, op), "np_fused_chain_reduce_axis %dx%d one float off %s" % (rows, cols, op))
            assert mask == CH_TEMPORARY, hex(mask)


@pytest.mark.parametrize("n", [1, 7, 1025, 65537, 2 ** 20 + 1, 4200003])
def test_chain_reduce_full_exact(n, dev):
    xi, xp = rf.ints((n,), 700 + n, _amp(n)), rf.prods((n,), None, 800 + n)
    xe, _ = rf.extremes((n,), None, rf.positions(n), 900 + n)
    xl, _ = rf.specials(xi, None, [n // 2, n - 1], 1, 0)          # NaN later only: never wins
    xf, _ = rf.specials(xi, None, [n // 2, n - 1], 3, 0)          # +Inf alone
    x0, _ = rf.specials(xi, None, [n // 2, n - 1], 0, 0)          # NaN in position 0: the result of min / max
    xa, _ = rf.specials(xi, None, [n // 2, n - 1], 2, 0)          # all NaN
    rows, cols = (n // 7, 7) if n % 7 == 0 else (1, n)
    for x, ops in ((xi, ("sum", "mean", "min", "max")), (xp, ("prod",)), (xe, ("min", "max")), (xl, ("sum", "mean", "min", "max")),
                   (xf, ("sum", "mean", "min", "max")), (x0, ("sum", "min", "max")), (xa, ("min", "max"))):
        for offset in (0, 1):
            with dev.held(x, offset) as v:
                for op in ops:
                    for how in ("host", "dev"):
                        got, mask = dev.chain(how, op, v, rows, cols)
                        _check(got, rf.expected(x, None, op), "np_fused_chain_reduce(%s) n=%d+%d %s" % (how, n, offset, op))
                        assert mask in (CH_FLAT, CH_STATIC_FLAT), hex(mask)


# ---- np_weighted_sums ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ALL_SIZES)
def test_weighted_sums_exact(n, dev):
    a, w = rf.ints((n,), 40 + n, 3), rf.ints((n,), 41 + n, 2)
    aw = int((a.astype(np.int64) * w.astype(np.int64)).sum())
    assert int((np.abs(a).astype(np.int64) * np.abs(w).astype(np.int64)).sum()) < rf.EXACT_LIMIT
    want = (np.float32(aw), rf.expected(w, None, "sum"))
    for offset in range(4):
        with dev.held(a, offset) as va, dev.held(w, offset) as vw:
            s_aw, s_w = C.c_float(), C.c_float()
            _lib.check(dev.L.np_weighted_sums(va.ptr, vw.ptr, n, C.byref(s_aw), C.byref(s_w)))
            _check(np.float32(s_aw.value), want[0], "np_weighted_sums n=%d+%d sum a w" % (n, offset))
            _check(np.float32(s_w.value), want[1], "np_weighted_sums n=%d+%d sum w" % (n, offset))


# ---- flags: np_all (flags = 0), np_count_mismatch (both modes) -------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 7, 8, 9, 1000, 100003, 4200003])
def test_flag_reductions_see_one_defect_anywhere(n, dev):
    L = dev.L
    ones = np.ones(n, np.float32)
    r = C.c_int()
    def verdicts(va, vb):
        _lib.check(L.np_all(va.ptr, n, 0, C.byref(r)))
        all_ok = r.value
        _lib.check(L.np_count_mismatch(0, va.ptr, vb.ptr, n, 0.0, 0.0, C.byref(r)))
        differ = r.value
        _lib.check(L.np_count_mismatch(1, va.ptr, vb.ptr, n, 1e-5, 1e-8, C.byref(r)))
        return all_ok, differ, r.value
    for offset in range(4):
        with dev.held(ones, offset) as va, dev.held(ones, offset) as vb:
            assert verdicts(va, vb) == (1, 0, 0), "n=%d+%d: a defect reported where there is none" % (n, offset)
            for p in sorted(set(rf.positions(n)) | set(_seam_positions(n, offset))):
                dev.poke(va, p, 0.0)
                got = verdicts(va, vb)
                assert got == (0, 1, 1), "n=%d+%d: the defect at %d gave (all, mismatches, violations) = %r" % (n, offset, p, got)
                dev.poke(va, p, 1.0)
            assert verdicts(va, vb) == (1, 0, 0)
