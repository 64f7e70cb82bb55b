"""The exact family of the layout kernels (np_layout.hip: np_transpose2d, np_permute, np_strided_copy, np_copy2d).  No device, numpy
only; tests/test_layout_reference_cpu.py checks this file against numpy and by hand, tests/test_gpu_layout_exact.py checks the
kernels against it.

Patterns.  words(n, salt): element i holds the bit pattern uint32(BASES[(salt + i) % 8] + i // 8).  The eight bases are +0 (then
the positive denormals), 0x80000000 (-0, then the negative denormals), +Inf (then signalling NaN payloads), -Inf (then negative
signalling NaNs), the first quiet NaN of either sign (then their payloads), 1.0 and the last denormals before the smallest
normal.  One run of consecutive integers uint32(salt + i) cannot hold all of these (they lie 2^22 and more apart), which is why
the index is dealt over eight runs and the salt only turns the deal: every operand of 16 elements or more holds each special
value itself, whatever the salt; specials() says which.  Every element of an operand is distinct, so a mismatch names its source index (source_index()).  A layout kernel moves
bits: every comparison is on uint32 views, and no word is ever looked at as a float.

Frames.  An operand lives inside a larger allocation at a chosen float offset; every other word of the allocation holds a canary
(0xC0DE.... around outputs, 0xBADD.... around inputs) that no operand contains.  expect() returns the WHOLE output allocation, the
canaries with the permuted pattern laid in: a kernel that writes one float outside its output, or reads one outside its input
and stores it, fails the comparison.

Plans.  plan_transpose2d / plan_permute / plan_strided_copy / plan_copy2d restate the dispatcher of np_layout.hip as host
arithmetic over the extents, the two addresses (only their alignment matters), the CU count and the variant knobs (Knobs), and
return the record np_debug_layout_last_record must report (include/np_hip_debug.h: NP_LAYOUT_*), or None where the call launches
nothing.  fuse() is the axis-fusion pass on its own."""
from dataclasses import dataclass

import numpy as np

# NP_LAYOUT_* of include/np_hip_debug.h (tests/test_layout_reference_cpu.py pins them against the header)
RECORD_WORDS = 16
FAMILY, FORM, ORDER, GRID_X, GRID_Y, GRID_Z, EXTRA = 0, 1, 2, 3, 4, 5, 6
MEMCPY, INTERLEAVE, SKINNY, TILE, WALIGN, PLANE, GATHER, COPY2D = 1, 2, 3, 4, 5, 6, 7, 8
FAMILY_NAMES = {0: "NONE", MEMCPY: "MEMCPY", INTERLEAVE: "INTERLEAVE", SKINNY: "SKINNY", TILE: "TILE", WALIGN: "WALIGN", PLANE: "PLANE",
                GATHER: "GATHER", COPY2D: "COPY2D"}
MAX_ND = 8

BASES = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x3F800000, 0x007FFFF8], np.uint64)
OUT_CANARY, IN_CANARY = 0xC0DE0000, 0xBADD0000
MAX_WORDS = 1 << 25          # i // 8 < 2^22, the least distance of two bases: every word stays inside its base's run
OUT_TAIL, IN_TAIL = 64, 8    # canary words behind an output / an input


def words(n, salt=0):
    if n < 0 or salt < 0 or n > MAX_WORDS:
        raise ValueError("words(): %d elements leave the runs of the bases" % n)
    i = np.arange(n, dtype=np.uint64)
    return (BASES[(i + np.uint64(salt)) % 8] + i // 8).astype(np.uint32)


def source_index(word, salt=0):
    """The element index that holds `word` in words(., salt), or None for a word no operand holds (a canary, a made-up value)."""
    for b, base in enumerate(BASES.tolist()):
        j = int(word) - base
        if 0 <= j < MAX_WORDS // 8:
            return j * 8 + (b - salt) % 8
    return None


def specials(w):
    """Which of the special values a uint32 array holds."""
    w = np.asarray(w, np.uint32)
    exp, man = (w >> 23) & 0xFF, w & 0x7FFFFF
    return {"denormal": bool(((exp == 0) & (man != 0)).any()), "-0": bool((w == 0x80000000).any()),
            "+inf": bool((w == 0x7F800000).any()), "-inf": bool((w == 0xFF800000).any()),
            "qnan": bool(((exp == 0xFF) & (man >= 0x400000)).any()),
            "snan": bool(((exp == 0xFF) & (man != 0) & (man < 0x400000)).any())}


def canary(n, base=OUT_CANARY):
    return (base | (np.arange(n, dtype=np.uint32) & 0xFFFF)).astype(np.uint32)


def framed_input(payload, offset, tail=IN_TAIL):
    """The allocation image of an input: `payload` at float `offset`, input canaries everywhere else."""
    payload = np.asarray(payload, np.uint32).reshape(-1)
    image = canary(offset + payload.size + tail, IN_CANARY)
    image[offset:offset + payload.size] = payload
    return image


def framed_output(payload, offset, tail=OUT_TAIL):
    """The allocation image an output must equal after the call: `payload` at float `offset`, output canaries everywhere else."""
    payload = np.asarray(payload, np.uint32).reshape(-1)
    image = canary(offset + payload.size + tail)
    image[offset:offset + payload.size] = payload
    return image


def blank_output(n, offset, tail=OUT_TAIL):
    """The allocation image of an output of n floats at `offset` before the call: canaries only."""
    return canary(offset + n + tail)


def expect(shape, perm, salt=0, out_offset=0, tail=OUT_TAIL):
    """The whole output allocation of out = transpose(in, perm), in = words(prod(shape), salt) as `shape`."""
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    x = words(n, salt).reshape(shape)
    return framed_output(np.ascontiguousarray(np.transpose(x, perm)), out_offset, tail)


def expect_strided(buffer, base, shape, strides, out_offset=0, tail=OUT_TAIL):
    """The whole output allocation of np_strided_copy: out[i0, i1, ..] = buffer[base + sum(i_d * strides[d])]."""
    index = np.full(tuple(shape), base, np.int64)
    for d, (extent, stride) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[d] = extent
        index = index + (np.arange(extent, dtype=np.int64) * stride).reshape(sh)
    assert index.min() >= 0 and index.max() < buffer.size
    return framed_output(np.asarray(buffer, np.uint32)[index.reshape(-1)], out_offset, tail)


# ---- the dispatcher restated -------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Knobs:
    """The state np_layout_set_variant leaves behind.  tile: the plain codes (0 default; 64 / 128 force the tile and switch the
    interleave, skinny, write-aligned and plane kernels off; 1 no write-aligned form; 3, 4 np_permute without the plane path; 5 no
    interleave; 6 the plane path with W = 1 only; 7 write-aligned tiles of 64 always).  walign64_below: 7000 + N.  walign_order:
    17000 + k (-1 = 17003, by size).  tile_order: 17010 + k (-1 = 17013).  plane_order: 17020 + k (-1 = 17023)."""
    tile: int = 0
    walign64_below: int = 1200
    walign_order: int = -1
    tile_order: int = -1
    plane_order: int = -1

    def codes(self):
        """The np_layout_set_variant calls that establish this state."""
        return [self.tile, 7000 + self.walign64_below, 17000 + (3 if self.walign_order < 0 else self.walign_order),
                17010 + (3 if self.tile_order < 0 else self.tile_order), 17020 + (3 if self.plane_order < 0 else self.plane_order)]


DEFAULT_CODES = [0, 8200, 17003, 17013, 17023]
assert Knobs().codes() == DEFAULT_CODES


def _ceil(a, b):
    return (a + b - 1) // b


def record(family, form=0, order=0, grid=(0, 0, 0), extra=()):
    r = [family, form, order] + list(grid) + list(extra)
    assert len(r) <= RECORD_WORDS
    return tuple(int(v) & 0xFFFFFFFF for v in r + [0] * (RECORD_WORDS - len(r)))


def describe(rec):
    """A record as one readable line (the log of the GPU tests, failure messages)."""
    if rec is None:
        return "no launch"
    fam, form, order, gx, gy, gz = rec[:6]
    x = rec[6:]
    s = FAMILY_NAMES.get(fam, "?%d" % fam)
    if fam == INTERLEAVE:
        s += "<R=%d,%s>" % (form & 0xFF, "to_interleaved" if form >> 8 else "to_planes")
    elif fam == SKINNY:
        s += "<TALL=%d>" % form
    elif fam == TILE:
        s += "<%d,VEC=%d> order=%d tiles=%dx%d pitch=%d/%d nbatch=%d" % (form & 0xFF, form >> 8, order, x[0], x[1], x[2], x[3], x[4])
    elif fam == WALIGN:
        s += "<%d> order=%d tiles=%dx%d pitch=%d/%d nbatch=%d" % (form, order, x[0], x[1], x[2], x[3], x[4])
    elif fam == PLANE:
        s += "<W=%d> A=%d B=%d E=%d ta=%d tb=%d tiles=%dx%d pitch=%d xcd_runs=%d" % ((form,) + tuple(x[:9]))
    elif fam == GATHER:
        s += "<u%d,W=%d>" % (form & 0xFF, form >> 8)
    elif fam == COPY2D:
        s += "<V=%d>" % form
    return s + " grid=(%d,%d,%d)" % (gx, gy, gz)


def instantiation(rec):
    """The kernel instantiation a record names (the table of the log: instantiation -> test id)."""
    return "none" if rec is None else describe(rec).split(" ")[0] + (" order=%d" % rec[2] if rec[0] in (TILE, WALIGN) else
                                                                      " xcd_runs=%d" % rec[2] if rec[0] == PLANE else "")


@dataclass
class PlaneBatch:
    in_pitch: int
    out_pitch: int
    bshape: list
    bin: list
    bout: list


def walign_order(rows, cols, k):
    return k.walign_order if k.walign_order >= 0 else (1 if rows * cols < 60_000_000 else 0)


def plan_planes(a_in, a_out, batch, rows, cols, pb, cus, k=Knobs()):
    """transpose_planes: `batch` planes of rows x cols, pitched as pb says."""
    vec = rows % 4 == 0 and cols % 4 == 0 and a_in % 16 == 0 and a_out % 16 == 0 and pb.in_pitch % 4 == 0 and pb.out_pitch % 4 == 0
    vec_batch = vec and all(i % 4 == 0 and o % 4 == 0 for i, o in zip(pb.bin, pb.bout))
    tile = k.tile if k.tile in (64, 128) else (128 if _ceil(rows, 128) * _ceil(cols, 128) * batch >= cus * 4 else 64)
    walign = (k.tile not in (1, 64, 128) and tile == 128 and pb.out_pitch % 32 != 0 and a_out % 128 == 0 and rows >= 256 and cols >= 64
              and rows + 31 < 0x7FFFFFFF)
    walign = walign and all(e == 1 or o % 32 == 0 for e, o in zip(pb.bshape, pb.bout))
    extra = lambda tx, ty: (tx, ty, pb.in_pitch, pb.out_pitch, len(pb.bshape))
    if walign and (k.tile == 7 or (k.walign64_below and _ceil(cols, 128) * _ceil(rows + 31, 128) * batch < k.walign64_below)):
        tx, ty = _ceil(cols, 64), _ceil(rows + 31, 64)
        if tx * ty <= 0x7FFFFFFF:
            return record(WALIGN, 64, walign_order(rows, cols, k), (tx * ty, 1, batch), extra(tx, ty))
    if walign:
        tx, ty = _ceil(cols, 128), _ceil(rows + 31, 128)
        if tx * ty <= 0x7FFFFFFF:
            return record(WALIGN, 128, walign_order(rows, cols, k), (tx * ty, 1, batch), extra(tx, ty))
    tx, ty = _ceil(cols, tile), _ceil(rows, tile)
    return record(TILE, tile | (1 if vec_batch else 0) << 8, 1 if k.tile_order > 0 else 0, (tx * ty, 1, batch), extra(tx, ty))


def plan_transpose2d(batch, rows, cols, a_in, a_out, cus, k=Knobs()):
    """np_transpose2d(in, out, batch, rows, cols); a_in / a_out: the two addresses."""
    if batch == 0 or rows == 0 or cols == 0:
        return None
    if k.tile == 0 and a_in % 16 == 0 and a_out % 16 == 0:
        if 2 <= rows <= 4 and cols % 4 == 0 and cols >= 1024:
            return record(INTERLEAVE, rows | 1 << 8, 0, (_ceil(cols, 2048), batch, 1))
        if 2 <= cols <= 4 and rows % 4 == 0 and rows >= 1024:
            return record(INTERLEAVE, cols, 0, (_ceil(rows, 2048), batch, 1))
    if (rows <= 16 or cols <= 16) and k.tile in (0, 5):
        tall = cols <= rows
        return record(SKINNY, 1 if tall else 0, 0, (min(_ceil(rows if tall else cols, 256), cus * 32), batch, 1))
    pb = PlaneBatch(cols, rows, [batch], [rows * cols], [rows * cols])
    return plan_planes(a_in, a_out, batch, rows, cols, pb, cus, k)


def fuse(shape, perm):
    """The fusion pass of np_permute: extent-1 axes dropped, input axes that stay adjacent and in order in the output fused.
    Returns (fused shape, fused perm)."""
    ndim = len(shape)
    pos = [0] * ndim
    for o in range(ndim):
        pos[perm[o]] = o
    fshape, first_pos, prev = [], [], -1
    for i in range(ndim):
        if shape[i] == 1:
            continue
        fused = prev >= 0 and pos[i] > pos[prev] and all(shape[perm[o]] == 1 for o in range(pos[prev] + 1, pos[i]))
        if fused:
            fshape[-1] *= shape[i]
        else:
            fshape.append(shape[i])
            first_pos.append(pos[i])
        prev = i
    order = sorted(range(len(fshape)), key=lambda g: first_pos[g])
    return tuple(fshape), tuple(order)


def plan_gather(out_shape, in_stride, n, cus):
    """launch_gather: out_shape / in_stride per OUTPUT axis."""
    last = len(out_shape) - 1
    vec4 = last >= 0 and in_stride[last] == 1 and out_shape[last] % 4 == 0 and out_shape[last] >= 32
    vec4 = vec4 and all(s % 4 == 0 for s in in_stride[:last])
    if vec4:
        n //= 4
    return record(GATHER, (32 if n < (1 << 31) else 64) | (4 if vec4 else 1) << 8, 0, (min(_ceil(n, 256), cus * 16), 1, 1))


def plan_permute(shape, perm, a_in, a_out, cus, k=Knobs()):
    """np_permute(in, out, ndim, shape, perm)."""
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    if n == 0:
        return None
    shape, perm = fuse(shape, perm)
    ndim = len(shape)
    if all(perm[i] == i for i in range(ndim)):
        return record(MEMCPY)
    if ndim >= 2 and perm[ndim - 1] == ndim - 2 and perm[ndim - 2] == ndim - 1 and all(perm[i] == i for i in range(ndim - 2)):
        batch = int(np.prod(shape[:ndim - 2], dtype=np.int64))
        if batch <= 65535 and shape[ndim - 2] <= 65535 * 64:
            return plan_transpose2d(batch, shape[ndim - 2], shape[ndim - 1], a_in, a_out, cus, k)
    in_strides = [0] * ndim
    s = 1
    for i in range(ndim - 1, -1, -1):
        in_strides[i] = s
        s *= shape[i]
    nd, E = ndim, 1
    if nd >= 3 and perm[nd - 1] == nd - 1 and shape[nd - 1] < 32 and k.tile in (0, 6):
        E = shape[nd - 1]
        nd -= 1
    if nd >= 2 and perm[nd - 1] != nd - 1 and k.tile in (0, 6):
        ax_a, ax_b = perm[nd - 1], nd - 1
        out_strides = [0] * ndim
        t = 1
        for i in range(ndim - 1, -1, -1):
            out_strides[i] = t
            t *= shape[perm[i]]
        A, B, a_stride, b_out = shape[ax_a], shape[ax_b], in_strides[ax_a], 0
        pb = PlaneBatch(0, 0, [], [], [])
        batch = 1
        for o in range(nd):
            ia = perm[o]
            if ia == ax_b:
                b_out = out_strides[o]
            elif ia != ax_a:
                pb.bshape.append(shape[ia])
                pb.bin.append(in_strides[ia])
                pb.bout.append(out_strides[o])
                batch *= shape[ia]
        pb.in_pitch, pb.out_pitch = a_stride, b_out
        if E == 1 and A >= 64 and B >= 64 and batch <= 65535:
            return plan_planes(a_in, a_out, batch, A, B, pb, cus, k)
        w4 = E % 4 == 0 and a_in % 16 == 0 and a_out % 16 == 0 and k.tile != 6
        if w4:
            E //= 4
        cap, pad = (1024, 128) if w4 else (4096, 512)
        side = 64
        while side > 1 and side * side * E > cap:
            side -= 1
        tb_max = min(B, side)
        if A < side:
            tb_max = max(1, min(cap // (A * E), 256, B))
        tiles_b = _ceil(B, tb_max)
        tb = _ceil(B, tiles_b)
        row = tb * E
        pitch = (row | 1) if (E == 1 or w4) else (_ceil(row, 64) * 64 + E)
        ta_max = max(1, min(cap // row, (cap + pad) // pitch, 256, A))
        tiles_a = _ceil(A, ta_max)
        ta = _ceil(A, tiles_a)
        blocks = tiles_a * tiles_b * batch
        if blocks <= 0x7FFFFFFF and ta * pitch <= cap + pad and tb * E > 1 and ta * E > 1:
            xcd = k.plane_order if k.plane_order >= 0 else (0 if w4 else 1)
            return record(PLANE, 4 if w4 else 1, xcd, (blocks, 1, 1), (A, B, E, ta, tb, tiles_a, tiles_b, pitch, xcd))
    return plan_gather([shape[perm[i]] for i in range(ndim)], [in_strides[perm[i]] for i in range(ndim)], n, cus)


def plan_strided_copy(shape, strides, cus):
    """np_strided_copy(in, out, ndim, shape, strides): no fusion, a memcpy when the strides are the contiguous ones."""
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    if n == 0:
        return None
    expect_stride, contiguous = 1, True
    for i in range(len(shape) - 1, -1, -1):
        if shape[i] != 1 and strides[i] != expect_stride:
            contiguous = False
        expect_stride *= shape[i]
    if contiguous:
        return record(MEMCPY)
    return plan_gather(list(shape), list(strides), n, cus)


def plan_copy2d(dst_pitch, src_pitch, width, rows, cus):
    """np_copy2d(dst, dst_pitch, src, src_pitch, width, rows)."""
    if width == 0 or rows == 0:
        return None
    if dst_pitch == width and src_pitch == width:
        return record(MEMCPY)
    vec = width % 4 == 0
    units = (width // 4 if vec else width) * rows
    return record(COPY2D, 4 if vec else 1, 0, (min(_ceil(units, 256), cus * 32), 1, 1))
