"""argmax / argmin by closed form — the exact family behind tests/test_argreduce_reference_cpu.py (the family against the oracle
and numpy, the plans pinned by hand) and tests/test_gpu_argreduce_exact.py (np_argreduce.hip against the family).  Plain numpy,
seeded, no device.

expected()   the reference's two loops (src/ndmath/calculation.c:9-72) as array operations.  argmax: a NaN in position 0 gives 0,
             later NaNs never win, else the first maximum.  argmin: the first NaN anywhere wins, else the first minimum.  -0 == +0.
plan()       np_argreduce's planner and launch_arg_fold restated on the host: the record np_debug_argreduce_last_record returns.  The
             operand's ADDRESS is an argument: addr % 16 decides rows_aligned, addr % 128 rows_are_lines.
points()     where along the axis, and in which output, the seams of the planned kernel lie: the scalar head and tail of
             arg_scan_contig, the first / last / second-to-last trip of each of the four accumulators in the first and the last lane,
             both sides of every slab, chunk, wave-row and 64-group tile boundary, the three row loops of argreduce_cols_tile.
families     winner_at, ties, permutation, nan_rules, constants: small integers and special values only, several outputs packed into
             one launch so that each row / column meets a different position.  Every family returns launches (label, x, want) with
             want = expected(x); winner_at and ties also carry the index by construction and assert that expected() agrees.
"""
import collections

import numpy as np

# ---- the record (include/np_hip_debug.h: NP_ARG_*) ---------------------------------------------------------------------------
RECORD_WORDS = 16
KERNEL, TEMPLATE, GRID_X, GRID_Y, GRID_Z, CHUNKS, CHUNK_LEN, XCD_RUNS, FOLD, FOLD_COLS, FOLD_GRID_X, FOLD_GRID_Y, FOLD_GRID_Z = range(13)
NONE, ROWS_GROUP, ROWS_WAVE, ROWS, SMALL_INNER, SMALL_INNER4, COLS_TILE, CHUNKS_KERNEL, GENERIC = range(9)
KERNEL_NAMES = {NONE: "NONE", ROWS_GROUP: "ROWS_GROUP", ROWS_WAVE: "ROWS_WAVE", ROWS: "ROWS", SMALL_INNER: "SMALL_INNER",
                SMALL_INNER4: "SMALL_INNER4", COLS_TILE: "COLS_TILE", CHUNKS_KERNEL: "CHUNKS", GENERIC: "GENERIC"}
FOLD_NONE, FOLD_THREAD, FOLD_BLOCK, FOLD_COLS_KERNEL = range(4)
FOLD_NAMES = {FOLD_NONE: "NONE", FOLD_THREAD: "THREAD", FOLD_BLOCK: "BLOCK", FOLD_COLS_KERNEL: "COLS_KERNEL"}

Knobs = collections.namedtuple("Knobs", "cols_wg_per_cu flat_wg_per_cu xcd_runs_off", defaults=(0, 0, 0))
DEFAULT_CODES = [4000000, 4100000, 4200000]


def codes(knobs):
    """The np_reduce_set_variant codes that set the knobs."""
    return [4000000 + knobs.cols_wg_per_cu, 4100000 + knobs.flat_wg_per_cu, 4200000 + (1 if knobs.xcd_runs_off else 0)]


def _cdiv(a, b):
    return (a + b - 1) // b


def capped_grid(wanted, cap):
    """np::capped_grid (np_internal.h): a capped grid is made odd."""
    if wanted <= cap:
        return max(wanted, 1)
    return cap | 1


def plan_fold(outputs, chunks, inner):
    """launch_arg_fold: (fold, COLS, grid)."""
    if inner >= 192 and chunks > 8 and outputs // inner <= 65535:
        outer = outputs // inner
        cols = 64 if _cdiv(inner, 64) * outer >= 64 else (16 if _cdiv(inner, 16) * outer >= 64 else 4)
        return FOLD_COLS_KERNEL, cols, (_cdiv(inner, cols), outer, 1)
    if chunks > 64 and outputs <= 0x7FFFFFFF:
        return FOLD_BLOCK, 0, (outputs, 1, 1)
    return FOLD_THREAD, 0, (_cdiv(outputs, 256), 1, 1)


def _rec(kernel, targ, grid, chunks, chunk_len, xcd_runs, fold=(FOLD_NONE, 0, (0, 0, 0))):
    words = [kernel, targ, grid[0], grid[1], grid[2], chunks, chunk_len, xcd_runs, fold[0], fold[1]] + list(fold[2])
    return tuple(int(w) & 0xFFFFFFFF for w in words) + (0,) * (RECORD_WORDS - len(words))


def plan(outer, axis_len, inner, addr, cus, knobs=Knobs()):
    """The record of np_argreduce(is_max, addr, outer, axis_len, inner, out) on a device of `cus` CUs; None where nothing is
    launched (an empty output, a refusal)."""
    n = axis_len
    if outer == 0 or inner == 0 or n == 0 or n > 0xFFFFFF00:
        return None
    if inner == 1 and n <= 256 and outer >= 1024:
        L = 1
        while L * 8 < n:
            L *= 2
        blocks = _cdiv(outer * L, 256)
        if blocks <= 0x7FFFFFFF:
            return _rec(ROWS_GROUP, L, (blocks, 1, 1), 1, n, 0)
    if inner == 1 and n <= 32768 and outer >= cus * 16 and _cdiv(outer, 4) <= 0x7FFFFFFF:
        return _rec(ROWS_WAVE, 0, (_cdiv(outer, 4), 1, 1), 1, n, 0)
    if inner == 1:
        target = capped_grid(cus * 8 + 1, cus * 8)
        chunks = 1
        if outer < target:
            chunks = min(_cdiv(target, outer), _cdiv(n, 4096))
        if outer * chunks > 0x7FFFFFFF:
            return None
        return _rec(ROWS, 0, (outer * chunks, 1, 1), chunks, _cdiv(n, chunks), 0, plan_fold(outer, chunks, 1))
    total = outer * inner
    groups4 = inner % 4 == 0 and inner <= 256
    if (groups4 or inner <= 64) and n * inner >= 4096 and outer <= 65535:
        per_cu = knobs.flat_wg_per_cu if knobs.flat_wg_per_cu > 0 else (2 if outer == 1 else 8)
        blocks = _cdiv(cus * per_cu, outer)
        min_rows = _cdiv(4096, inner)
        blocks = max(min(blocks, max(n // min_rows, 1)), 1)
        rows_per_block = (_cdiv(n, blocks) + 3) // 4 * 4
        if rows_per_block * inner < 1 << 31:
            blocks = _cdiv(n, rows_per_block)
            return _rec(SMALL_INNER4 if groups4 else SMALL_INNER, 0, (blocks, outer, 1), blocks, rows_per_block, 0,
                        plan_fold(total, blocks, inner))
    if inner >= 192 and outer <= 65535 and n >= 16:
        tiles = _cdiv(_cdiv(inner, 4), 64)
        chunks = 1
        rows_aligned = inner % 4 == 0 and addr % 16 == 0
        per_cu = knobs.cols_wg_per_cu if knobs.cols_wg_per_cu > 0 else (2 if rows_aligned else 8)
        base_wg, target_wg = tiles * outer, cus * per_cu
        if base_wg < target_wg:
            chunks = max(min(target_wg // base_wg, max(n // 64, 1)), 1)
        chunk_len = _cdiv(n, chunks)
        if chunks > 1 and chunk_len % 2 == 0:
            chunk_len += 1
        chunks = _cdiv(n, chunk_len)
        if tiles <= 0x7FFFFFFF and chunks <= 65535:
            rows_are_lines = (inner * 4) % 128 == 0 and addr % 128 == 0
            xcd_runs = 1 if (not rows_are_lines and tiles > 1 and tiles * chunks * outer < 1 << 31 and not knobs.xcd_runs_off) else 0
            if chunks == 1:
                return _rec(COLS_TILE, 1, (tiles, 1, outer), 1, chunk_len, xcd_runs)
            return _rec(COLS_TILE, 0, (tiles, chunks, outer), chunks, chunk_len, xcd_runs, plan_fold(total, chunks, inner))
    target_threads = cus * 2048
    if total < target_threads and n >= 128:
        chunks = min(_cdiv(target_threads, total), n // 32)
        chunk_len = _cdiv(n, chunks)
        chunks = _cdiv(n, chunk_len)
        if chunks > 1:
            blocks = min(_cdiv(total * chunks, 256), cus * 16)
            return _rec(CHUNKS_KERNEL, 0, (blocks, 1, 1), chunks, chunk_len, 0, plan_fold(total, chunks, inner))
    return _rec(GENERIC, 0, (min(_cdiv(total, 256), cus * 16), 1, 1), 1, n, 0)


def instantiation(rec):
    """The kernel instantiations of a record: 'COLS_TILE<FINAL=0>+FOLD_COLS<16>'."""
    if rec is None:
        return "NONE"
    k = KERNEL_NAMES[rec[KERNEL]]
    if rec[KERNEL] == ROWS_GROUP:
        k += "<L=%d>" % rec[TEMPLATE]
    elif rec[KERNEL] == COLS_TILE:
        k += "<FINAL=%d>" % rec[TEMPLATE]
    if rec[FOLD] == FOLD_COLS_KERNEL:
        k += "+FOLD_COLS<%d>" % rec[FOLD_COLS]
    elif rec[FOLD] != FOLD_NONE:
        k += "+FOLD_" + FOLD_NAMES[rec[FOLD]]
    return k


def describe(rec):
    if rec is None:
        return "no launch"
    return "%s grid=(%d,%d,%d) chunks=%d chunk_len=%d xcd_runs=%d fold_grid=(%d,%d,%d)" % (
        (instantiation(rec),) + tuple(rec[GRID_X:GRID_Z + 1]) + (rec[CHUNKS], rec[CHUNK_LEN], rec[XCD_RUNS]) + tuple(rec[FOLD_GRID_X:FOLD_GRID_Z + 1]))


# ---- the reference ------------------------------------------------------------------------------------------------------------

def _slices(x, axis):
    x = np.asarray(x, np.float32)
    if axis is None:
        return x.reshape(1, x.size, 1), ()
    axis = axis % x.ndim
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    return x.reshape(outer, x.shape[axis], inner), tuple(x.shape[:axis]) + tuple(x.shape[axis + 1:])


def expected(x, axis, is_max):
    """float_argmax / float_argmin along `axis` (None: the flat array), float32 indices like the device's."""
    v, oshape = _slices(x, axis)
    nan = np.isnan(v)
    if is_max:
        # `*ip > mp` is false for a NaN on either side: a later NaN never wins, a NaN in position 0 is never replaced
        key = np.where(nan, -np.inf, v)
        idx = np.argmax(key, axis=1)
        idx = np.where(nan[:, 0, :], 0, idx)
    else:
        # `!(mp <= *ip)` is true for the first NaN met, and the loop stops there
        idx = np.where(nan.any(axis=1), np.argmax(nan, axis=1), np.argmin(np.where(nan, np.inf, v), axis=1))
    return idx.astype(np.float32).reshape(oshape)


# ---- where the seams are --------------------------------------------------------------------------------------------------------

def head_of(addr, count):
    """arg_scan_contig's scalar head: the elements in front of the first 16-byte boundary."""
    return min(((16 - addr % 16) % 16) // 4, count)


def scan_positions(count, head, stride, tids):
    """Positions of `count` contiguous elements that arg_scan_contig(STRIDE = stride) treats differently from their neighbours, for
    the lanes `tids`: accumulator s2 of lane t owns the vectors t + (4 j + s2) stride."""
    nvec = (count - head) // 4
    p = {0, 1, count - 1, head - 1, head, head + 4 * nvec - 1}
    p.update(range(head + 4 * nvec, count))          # the <= 3 tail elements
    p.update(range(0, head))                          # the head lanes
    for t in tids:
        for s2 in range(4):
            first = t + s2 * stride
            if first >= nvec:
                continue
            last = first + (nvec - 1 - first) // (4 * stride) * (4 * stride)
            for v in {first, last, max(last - 4 * stride, first)}:
                p.update((head + 4 * v, head + 4 * v + 3))
    return sorted(q for q in p if 0 <= q < count)


def _flat_points(r0, rows, inner, group, n):
    """A slab of the flat walks: `rows` rows from r0 of `inner` columns, walked by T lanes with vectors of 4 floats (group = 1:
    argreduce_small_inner) or of one float4 column group (group = 4: argreduce_small_inner4 — the same arithmetic on flat
    elements).  Points (row, column)."""
    cnt = rows * inner
    nvec = cnt // 4
    unit = inner if group == 1 else inner // 4
    T = (256 // unit) * unit
    pts = set()
    for t in (0, 1, T - 1):
        for s2 in range(4):
            first = t + s2 * T
            if first >= nvec:
                continue
            last = first + (nvec - 1 - first) // (4 * T) * (4 * T)
            for v in {first, last, max(last - 4 * T, first)}:
                for e in (4 * v, 4 * v + 3):
                    pts.add((r0 + e // inner, e % inner))
    for e in range(4 * nvec, cnt):                   # the leftover elements of argreduce_small_inner
        pts.add((r0 + e // inner, e % inner))
    for e in (0, cnt - 1, 4 * nvec - 1, 4 * min(T, nvec) - 1, 4 * min(T, nvec) % cnt):
        pts.add((r0 + e // inner, e % inner))
    return {(a, j) for a, j in pts if 0 <= a < n}


def _tile_rows(a0, a1):
    """argreduce_cols_tile: wave w walks rows a0 + w, + 4, ... in loops of 8, 4 and 1 rows per trip: the first and last row of each
    loop, per wave."""
    rows = {a0, a1 - 1}
    for w in range(4):
        a = a0 + w
        if a >= a1:
            continue
        rows.add(a)
        while a + 28 < a1:
            rows.update((a, a + 4, a + 28))
            a += 32
        while a + 12 < a1:
            rows.update((a, a + 12))
            a += 16
        while a < a1:
            rows.add(a)
            a += 4
    return rows


def points(rec, outer, n, inner, addr):
    """[(slots, a)]: position a of the axis is a seam for the outputs `slots` (a list of flat output indices o * inner + j; None =
    for any output)."""
    k = rec[KERNEL]
    out = [(None, a) for a in (0, 1, n - 1, n // 2)]
    if k == ROWS_WAVE or k == ROWS:
        stride = 64 if k == ROWS_WAVE else rec[CHUNKS] * 256
        by_head = collections.defaultdict(list)
        for o in range(outer):
            by_head[head_of(addr + 4 * o * n, n)].append(o)
        for head, rows in by_head.items():
            nvec = (n - head) // 4
            # the first and the last lane, both sides of a wave and of a workgroup, and the lane at which the vectors run out
            tids = sorted({t for t in (0, 1, 63, 64, 255, 256, stride - 1, nvec % stride - 1, nvec % stride) if 0 <= t < stride})
            out += [(rows, a) for a in scan_positions(n, head, stride, tids)]
    elif k in (SMALL_INNER, SMALL_INNER4):
        rpb, blocks = rec[CHUNK_LEN], rec[CHUNKS]
        for b in range(blocks):                      # every slab: both sides of its boundaries and its own seams
            r0 = b * rpb
            r1 = min(n, r0 + rpb)
            out += [(None, a) for a in (r0 - 1, r0, r1 - 1) if 0 <= a < n]
            for a, j in sorted(_flat_points(r0, r1 - r0, inner, 1 if k == SMALL_INNER else 4, n)):
                out.append(([o * inner + j for o in range(outer)], a))
    elif k == COLS_TILE:
        cl, chunks = rec[CHUNK_LEN], rec[CHUNKS]
        cols = sorted({c for c in (0, 3, 4, 252, 255, 256, 259, 511, 512, inner - 4, inner - 3, inner - 2, inner - 1) if 0 <= c < inner})
        out += [(None, a) for c in range(1, chunks) for a in (c * cl - 1, c * cl)]       # both sides of every chunk boundary
        for c in sorted({0, 1, chunks - 1} & set(range(chunks))):
            a0 = c * cl
            a1 = min(n, a0 + cl)
            rows = sorted(_tile_rows(a0, a1) | ({a0 - 1} if a0 else set()))
            out += [(None, a) for a in rows]
            for j in cols:
                out += [([o * inner + j for o in range(outer)], a) for a in rows]
    elif k == CHUNKS_KERNEL:
        cl, chunks = rec[CHUNK_LEN], rec[CHUNKS]
        for c in range(chunks):                      # every chunk
            a0 = c * cl
            a1 = min(n, a0 + cl)
            last4 = a0 + 1 + (a1 - a0 - 1) // 4 * 4
            out += [(None, a) for a in (a0 - 1, a0, a0 + 1, a0 + 4, a0 + 5, last4 - 1, last4, a1 - 1) if 0 <= a < n]
    if n <= 600:
        out += [(None, a) for a in range(n)]
    return out


def pack(pts, outputs, n):
    """Launches: each a position per output (an int64 array of `outputs`), so that every point of `pts` is met in one of them.
    Outputs a launch has no point for take positions of their own ((5 m + 3 l) mod n), so no output is ever idle."""
    seen, uniq = set(), []
    for slots, a in pts:
        key = (None if slots is None else tuple(slots), a)
        if key not in seen and 0 <= a < n:
            seen.add(key)
            uniq.append((slots, a))
    launches = []                                     # [position per output, -1 = free]
    nxt = collections.defaultdict(int)                # per slot list: the launch to try next
    for slots, a in [p for p in uniq if p[0] is not None]:
        key = tuple(slots)
        while True:
            l = nxt[key]
            if l == len(launches):
                launches.append(np.full(outputs, -1, np.int64))
            free = [m for m in slots if launches[l][m] < 0]
            if free:
                launches[l][free[0]] = a
                break
            nxt[key] += 1
    l = 0
    for slots, a in [p for p in uniq if p[0] is None]:
        while True:
            if l == len(launches):
                launches.append(np.full(outputs, -1, np.int64))
            free = np.flatnonzero(launches[l] < 0)
            if free.size:
                launches[l][free[0]] = a
                break
            l += 1
    for l, pos in enumerate(launches):
        free = np.flatnonzero(pos < 0)
        pos[free] = (5 * free + 3 * l) % n
    return launches


# ---- the data ---------------------------------------------------------------------------------------------------------------------

def _put(x, pos, value):
    """x[o, pos[o * inner + j], j] = value (a scalar or one value per output)."""
    outer, n, inner = x.shape
    m = np.arange(outer * inner)
    x[m // inner, pos, m % inner] = value


def _launch(label, x, is_max, by_construction=None):
    want = expected(x, 1, is_max).reshape(-1)
    if by_construction is not None:
        assert (want == by_construction.astype(np.float32)).all(), "%s: expected() disagrees with the construction" % label
    return label, x, want


def winner_at(rec, outer, n, inner, addr, is_max, background):
    """A constant background with one strictly better element per output, at every point of points().  background 'finite' = 3.0
    with the winner 4.0 / 2.0; 'identity' = -Inf / +Inf (what the accumulators start from) with the winner 0.0."""
    sign = 1.0 if is_max else -1.0
    bg, win = (3.0, 3.0 + sign) if background == "finite" else (-sign * np.inf, 0.0)
    out = []
    for l, pos in enumerate(pack(points(rec, outer, n, inner, addr), outer * inner, n)):
        x = np.full((outer, n, inner), bg, np.float32)
        _put(x, pos, win)
        out.append(_launch("winner_at[%s] launch %d" % (background, l), x, is_max, pos))
    return out


def ties(rec, outer, n, inner, addr, is_max, background="finite"):
    """The best value at two or three positions per output, drawn from different parts of points(): the earliest wins."""
    sign = 1.0 if is_max else -1.0
    bg, win = (3.0, 3.0 + sign) if background == "finite" else (-sign * np.inf, 0.0)
    launches = pack(points(rec, outer, n, inner, addr), outer * inner, n)
    out = []
    for l, pos in enumerate(launches):
        other = launches[(l + 1) % len(launches)][::-1] if len(launches) > 1 else (pos[::-1] + n // 2) % n
        other = np.where(other == pos, (pos + max(n // 2, 1)) % n, other)     # two different positions wherever the axis has two
        third = (pos + other + 1 + n // 3) % n
        x = np.full((outer, n, inner), bg, np.float32)
        _put(x, pos, win)
        _put(x, other, win)
        m = np.arange(outer * inner)
        x[(m // inner)[m % 2 == 1], third[m % 2 == 1], (m % inner)[m % 2 == 1]] = win        # three on the odd outputs
        first = np.where(m % 2 == 1, np.minimum(np.minimum(pos, other), third), np.minimum(pos, other))
        out.append(_launch("ties[%s] launch %d" % (background, l), x, is_max, first))
    return out


def constants(rec, outer, n, inner, addr, is_max):
    """All-equal, all -Inf, all +Inf, and mixtures of -0.0 and +0.0: index 0 everywhere."""
    out = []
    zero = np.zeros(outer * inner, np.int64)
    for name, value in (("2.5", 2.5), ("-inf", -np.inf), ("+inf", np.inf)):
        out.append(_launch("constant %s" % name, np.full((outer, n, inner), value, np.float32), is_max, zero))
    for first in (0.0, -0.0):
        x = np.full(outer * n * inner, first, np.float32)
        e = np.arange(x.size)
        x[(e * 7 // 3) % 2 == 1] = -first
        x = x.reshape(outer, n, inner)
        x[:, 0, :] = first
        out.append(_launch("zeros, %r first" % first, x, is_max, zero))
    return out


def permutation(rec, outer, n, inner, addr, is_max, seed=0):
    """Every element of a slice is a distinct integer 0 .. n - 1 (n <= 2^24): any mis-indexed read changes some answer.  Two
    launches: seeded shuffles, and the ramp running against the function (the winner is the LAST element of every slice)."""
    rng = np.random.default_rng(1000 + seed)
    x = np.broadcast_to(np.arange(n, dtype=np.float32)[None, :, None], (outer, n, inner))
    out = [_launch("permutation shuffled", rng.permuted(x, axis=1).astype(np.float32), is_max)]
    ramp = np.ascontiguousarray(x if is_max else -x)
    out.append(_launch("permutation ramp", ramp, is_max, np.full(outer * inner, n - 1)))
    return out


QNAN_NEG, QNAN_PAYLOAD, SNAN = 0xFFC00000, 0x7FC12345, 0x7FA00001


def nan_rules(rec, outer, n, inner, addr, is_max):
    """Per output one of nine NaN patterns (m mod 9) on a background of 3.0 with one 9.0 and one -9.0, the positions drawn from
    points(): 0 NaN in position 0 alone; 1 with +Inf (argmin: -Inf) later; 2 with a second NaN later; 3 one NaN at p > 0 right
    beside the extreme; 4 two NaNs, both after the extremes; 5 two NaNs, both before the extremes; 6 all NaN; 7 a negative NaN
    at p; 8 a NaN with a payload at p and a signalling one later."""
    launches = pack(points(rec, outer, n, inner, addr), outer * inner, n)
    out = []
    M = outer * inner
    m = np.arange(M)
    o, j = m // inner, m % inner
    for l, pos in enumerate(launches):
        other = launches[(l + 1) % len(launches)][::-1] if len(launches) > 1 else (pos[::-1] + n // 2) % n
        x = np.full((outer, n, inner), 3.0, np.float32)
        xb = x.view(np.uint32)
        lo, hi = np.minimum(pos, other), np.maximum(pos, other)
        kind = m % 9 if n >= 4 else np.where(m % 2 == 0, 0, 6)
        # the two extremes: at lo and hi for most kinds
        ext = 9.0 if is_max else -9.0
        for kd in (0, 1, 2, 7, 8):
            s = kind == kd
            x[o[s], hi[s], j[s]] = ext
            x[o[s], lo[s], j[s]] = -ext if kd != 7 else 3.0
        s = kind == 0
        x[o[s], 0, j[s]] = np.nan
        s = kind == 1
        x[o[s], 0, j[s]] = np.nan
        x[o[s], np.maximum(hi[s], 1), j[s]] = np.inf if is_max else -np.inf
        s = kind == 2
        x[o[s], 0, j[s]] = np.nan
        x[o[s], np.maximum(lo[s], 1), j[s]] = np.nan
        if n >= 4:
            s = kind == 3                                 # NaN at p >= 1, the extreme right in front of it
            p3 = np.maximum(pos, 1)
            x[o[s], p3[s] - 1, j[s]] = ext
            x[o[s], p3[s], j[s]] = np.nan
            s = kind == 4                                 # extremes at 0 / 1, NaNs behind
            x[o[s], 0, j[s]] = -ext
            x[o[s], 1, j[s]] = ext
            x[o[s], np.maximum(lo[s], 2), j[s]] = np.nan
            x[o[s], np.maximum(hi[s], 2), j[s]] = np.nan
            s = kind == 5                                 # NaNs first, the extremes at the end
            x[o[s], np.minimum(lo[s], n - 3), j[s]] = np.nan
            x[o[s], np.minimum(hi[s], n - 3), j[s]] = np.nan
            x[o[s], n - 2, j[s]] = ext
            x[o[s], n - 1, j[s]] = -ext
        s = kind == 6
        x[o[s], :, j[s]] = np.nan
        if n >= 4:
            s = kind == 7
            xb[o[s], np.maximum(lo[s], 1), j[s]] = QNAN_NEG
            s = kind == 8
            xb[o[s], np.maximum(lo[s], 1), j[s]] = QNAN_PAYLOAD
            xb[o[s], np.maximum(hi[s], 1), j[s]] = SNAN
        out.append(_launch("nan_rules launch %d" % l, x, is_max))
    return out


FAMILIES = {"winner_finite": lambda *a: winner_at(*a, "finite"), "winner_identity": lambda *a: winner_at(*a, "identity"),
            "ties": ties, "ties_identity": lambda *a: ties(*a, "identity"), "constants": constants, "permutation": permutation,
            "nan_rules": nan_rules}
