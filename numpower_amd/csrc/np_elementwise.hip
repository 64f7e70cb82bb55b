// Elementwise kernels of libnp_hip.so: binary ops with fused scalar/row/column broadcast, the
// unary float_* family, and fill.  HBM-bound streaming kernels: 16 B per lane per access
// (global_load/store_dwordx4), UNROLL independent accesses in flight per lane, an uncapped grid
// (every lane moves UNROLL float4 and retires), non-temporal loads and stores.  No LDS, no MFMA:
// nothing here has reuse.
//
// Reference behaviour restated (file:line relative to the reference tree):
//   binary ops      src/ndmath/arithmetics.c:160-926  (+ CUDA kernels cuda_math.cu:593-633)
//   broadcast       src/ndarray.c:1172-1294           (materialised there, index math here)
//   unary ops       src/ndmath/double_math.c:9-265    (+ CUDA kernels cuda_math.cu:207-585)
//   fill            cuda_math.cu:829,912
#include <math.h>

#include "np_internal.h"
#include "np_elementwise_ops.h"

// Bit-level parity with the reference's CPU results needs every multiply, add and divide rounded
// on its own: no implicit FMA contraction anywhere in this file (the two places where the
// reference's build DOES fuse — mod's AVX body and the rsqrt Newton step — say so with an
// explicit __fmaf_rn).  `/` and sqrtf are IEEE-correct under hipcc's defaults; the __f*_rn
// helpers are plain operators in this ROCm, kept only as documentation of intent.
#pragma clang fp contract(off)

namespace {


// Row length of a broadcast whose float4s may straddle rows (cols % 4 != 0): `cols` = 0 means "not
// ragged" (the fast path below), else the per-element (row, col) come from fast_div.
template <typename I>
struct Ragged {
    I cols;
    unsigned m, s1, s2;
    // A ROW operand too long to stay cached (X + r with 7 x 10^7: each of the 7 result rows re-reads the 40 MB vector,
    // 4.8 TB/s where X + col runs 6.3): rowblock_rows = rows of the result switches the work order from row-major to
    // column blocks, XCD by XCD — workgroup w (dispatched to XCD w % 8) takes 256 float4 slots of column block
    // (w / 8 / rows) * 8 + w % 8 in row (w / 8) % rows: the workgroups that need the same 4 KiB piece of the vector follow
    // each other on ONE XCD and find it in that XCD's L2 (sharing it across consecutive workgroups, i.e. across the eight
    // private L2s, changed nothing: profiles/r04/misc_sweep.log).  wspace = rows x column blocks (rounded up to 8) x 256
    // work items.  0 = off (the plain order).
    unsigned rowblock_rows;
    I wspace;
};

template <typename I>
__device__ __forceinline__ I ragged_row(const Ragged<I> &r, I e) {
    if constexpr (sizeof(I) == 4) return (I)fast_div((unsigned)e, r.m, r.s1, r.s2);
    return e / r.cols;
}

// Operand fetch for the vector path: `v` is the float4 index into the rows x cols output,
// cols4 = cols / 4.  With cols % 4 == 0 a float4 never straddles a row: ROW is one float4 load, COL
// one scalar.  Otherwise (rg.cols != 0, a uniform branch) each of the four elements gets its own
// row / column index; the row / column vector itself is cache-resident.
template <int KIND, bool NT, typename I>
__device__ __forceinline__ v4f fetch4(const float *p, I v, I cols4, float splat, const Ragged<I> &rg) {
    if constexpr (KIND == NP_FULL) return ld4<NT>(p + (size_t)v * 4);
    if constexpr (KIND == NP_SCALAR) return v4f{splat, splat, splat, splat};
    if constexpr (KIND == NP_ROW) {
        if (rg.cols == 0) return *(const v4f_u *)(p + (size_t)(v % cols4) * 4);
        // ragged: ONE division per float4 (the position of its first element), then a dword-aligned float4 load when the
        // four elements stay in one row — all but one float4 in cols / 4 — and a walk with wrap-around for the others
        const I e0 = v * 4;
        I c = e0 - ragged_row(rg, e0) * rg.cols;
        if (c + 3 < rg.cols) return *(const v4f_u *)(p + (size_t)c);
        v4f r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = p[(size_t)c];
            c = c + 1 == rg.cols ? (I)0 : c + 1;
        }
        return r;
    }
    if constexpr (KIND == NP_COL) {
        if (rg.cols == 0) {
            const float s = p[(size_t)(v / cols4)];
            return v4f{s, s, s, s};
        }
        // (one division per float4 + a walk, as for ROW above, measured 2 % slower here than four divisions: the column
        // operand needs no second load in the common case either way — tools/ragged_ab.py)
        v4f r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = p[(size_t)ragged_row(rg, (I)(v * 4 + k))];
        return r;
    }
    return v4f{0, 0, 0, 0};
}

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

// Vector path: each lane handles UNROLL float4 per trip, spaced one grid apart so that every
// wave-level access is a contiguous 1 KiB segment.
template <int OP, int AK, int BK, bool QUIRK, int UNROLL, bool NT, typename I, bool POWREG = false>
__global__ __launch_bounds__(256) void binary_vec_kernel(const float *__restrict__ a,
                                                         const float *__restrict__ b,
                                                         float *__restrict__ out, I nvec, I cols4,
                                                         I tail_start, I n, I body_end, float ha,
                                                         float hb, Ragged<I> rg) {
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    // scalar operands: device pointer, or (null pointer) a value handed over by the host
    float sa = 0.0f, sb = 0.0f;
    if constexpr (AK == NP_SCALAR) sa = a ? a[0] : ha;
    if constexpr (BK == NP_SCALAR) sb = b ? b[0] : hb;
    // pow: every wave stages its own copy of the log2 table (512 B) in LDS — no workgroup barrier: a wave's
    // LDS operations complete in order, so its reads below see its own writes
    constexpr bool LDSTAB = OP == NP_POW && !POWREG;
    __shared__ PowLogEntry pow_tab_lds[LDSTAB ? 4 : 1][LDSTAB ? 32 : 1];
    PowTabLds pow_tab = (PowTabLds)&pow_tab_lds[LDSTAB ? (threadIdx.x >> 6) : 0][0];
    PowTabRegs pow_regs{0, 0};
    if constexpr (LDSTAB) {
        const unsigned lane = threadIdx.x & 63u;
        if (lane < 32u) pow_tab_lds[threadIdx.x >> 6][lane] = kPowLogTab[lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (POWREG) pow_regs.load(threadIdx.x & 63u);

    // POWREG: the loop and the arithmetic run with the whole wave active (the table lives in its lanes); lanes past
    // the end compute 1^1 and store nothing
    constexpr bool ROWBLOCK = (AK == NP_ROW || BK == NP_ROW) && sizeof(I) == 4 && OP != NP_POW;
    const I limit = ROWBLOCK && rg.rowblock_rows ? rg.wspace : nvec;
    // work item -> float4 slot (see Ragged::rowblock_rows); ok = the slot exists
    auto slot_of = [&](I w, bool &ok) -> I {
        if constexpr (ROWBLOCK) {
            if (rg.rowblock_rows) {   // uniform
                const unsigned wg = __builtin_amdgcn_readfirstlane((unsigned)w >> 8);   // a workgroup's 256 items share it
                const unsigned j = wg >> 3, grp = j / rg.rowblock_rows, row = j - grp * rg.rowblock_rows;
                const unsigned c = (grp * 8u + (wg & 7u)) * 256u + ((unsigned)w & 255u);
                ok = w < limit && c < (unsigned)cols4;
                return (I)(row * (unsigned)cols4 + c);
            }
        }
        ok = w < nvec;
        return w;
    };
    auto more = [&](I base) { return POWREG ? __builtin_amdgcn_ballot_w64(base < nvec) != 0ull : base < limit; };
    for (I base = tid; more(base); base += stride * UNROLL) {
        v4f va[UNROLL], vb[UNROLL];
        I slot[UNROLL];
        bool live[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            slot[u] = slot_of(base + (I)u * stride, live[u]);
            const I v = slot[u];
            if constexpr (POWREG) va[u] = vb[u] = v4f{1.0f, 1.0f, 1.0f, 1.0f};
            if (live[u]) {
                va[u] = fetch4<AK, NT, I>(a, v, cols4, sa, rg);
                vb[u] = fetch4<BK, NT, I>(b, v, cols4, sb, rg);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const I v = slot[u];
            if constexpr (POWREG) {
                const float px[4] = {va[u][0], va[u][1], va[u][2], va[u][3]};
                const float py[4] = {vb[u][0], vb[u][1], vb[u][2], vb[u][3]};
                float pr[4];
                pow_n<4>(px, py, pr, pow_regs);
                if (live[u]) st4<NT>(out + (size_t)v * 4, v4f{pr[0], pr[1], pr[2], pr[3]});
            } else if (live[u]) {
                v4f r;
                const I e = v * 4;
                if constexpr (OP == NP_POW) {
                    const float px[4] = {va[u][0], va[u][1], va[u][2], va[u][3]};
                    const float py[4] = {vb[u][0], vb[u][1], vb[u][2], vb[u][3]};
                    float pr[4];
                    pow_n<4>(px, py, pr, pow_tab);
                    r = v4f{pr[0], pr[1], pr[2], pr[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        r[k] = binary_apply<OP, QUIRK>(va[u][k], vb[u][k], (e + k) < body_end);
                }
                st4<NT>(out + (size_t)v * 4, r);
            }
        }
    }
    // ragged tail (n % 4 elements): FULL/SCALAR operand kinds, or a ragged broadcast
    if (blockIdx.x == 0) {
        const I i = tail_start + threadIdx.x;
        if (i < n) {
            auto at = [&](const float *p, int kind, float splat) -> float {
                if (kind == NP_SCALAR) return splat;
                if (kind == NP_FULL) return p[i];
                const I row = ragged_row(rg, i);
                return kind == NP_ROW ? p[(size_t)(i - row * rg.cols)] : p[(size_t)row];
            };
            out[i] = binary_apply<OP, QUIRK>(at(a, AK, sa), at(b, BK, sb), i < body_end);
        }
    }
}

// Scalar path: any operand kinds, any shape/alignment.
template <int OP, bool QUIRK, typename I>
__global__ __launch_bounds__(256) void binary_scalar_kernel(const float *__restrict__ a, int ak,
                                                            const float *__restrict__ b, int bk,
                                                            float *__restrict__ out, I n, I cols,
                                                            I body_end, float ha, float hb) {
    const I stride = (I)gridDim.x * blockDim.x;
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float x, y;
        switch (ak) {
            case NP_FULL: x = a[i]; break;
            case NP_SCALAR: x = a ? a[0] : ha; break;
            case NP_ROW: x = a[i % cols]; break;
            default: x = a[i / cols]; break;
        }
        switch (bk) {
            case NP_FULL: y = b[i]; break;
            case NP_SCALAR: y = b ? b[0] : hb; break;
            case NP_ROW: y = b[i % cols]; break;
            default: y = b[i / cols]; break;
        }
        out[i] = binary_apply<OP, QUIRK>(x, y, i < body_end);
    }
}

template <int OP, int UNROLL, bool NT, typename I>
__global__ __launch_bounds__(256) void unary_vec_kernel(const float *in, float *out, I nvec,
                                                        I tail_start, I n, float p0, float p1) {
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    for (I base = tid; base < nvec; base += stride * UNROLL) {
        v4f vx[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const I v = base + (I)u * stride;
            if (v < nvec) vx[u] = ld4<NT>(in + (size_t)v * 4);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const I v = base + (I)u * stride;
            if (v < nvec) {
                v4f r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = unary_apply<OP>(vx[u][k], p0, p1);
                st4<NT>(out + (size_t)v * 4, r);
            }
        }
    }
    if (blockIdx.x == 0) {
        const I i = tail_start + threadIdx.x;
        if (i < n) out[i] = unary_apply<OP>(in[i], p0, p1);
    }
}

template <int OP, typename I>
__global__ __launch_bounds__(256) void unary_scalar_kernel(const float *in, float *out, I n,
                                                           float p0, float p1) {
    const I stride = (I)gridDim.x * blockDim.x;
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = unary_apply<OP>(in[i], p0, p1);
}

template <typename I>
__global__ __launch_bounds__(256) void fill_kernel(float *__restrict__ out, float value, I n,
                                                   I head, I nvec) {
    // head = elements before the first 16-byte boundary, then nvec float4, then the rest
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    const v4f v{value, value, value, value};
    for (I i = tid; i < nvec; i += stride) __builtin_nontemporal_store(v, (v4f *)(out + head + (size_t)i * 4));
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) out[threadIdx.x] = value;
        const I t = head + nvec * 4 + threadIdx.x;
        if (t < n) out[t] = value;
    }
}

// ------------------------------------------------------------------------------------------
// launch configuration
// ------------------------------------------------------------------------------------------

// Plain device-to-device copy of 4-byte words (np::device_copy): the same float4 / non-temporal stream
// as the unary kernels; hipMemcpyAsync's blit reaches 5.1-5.3 TB/s on large buffers, this 6.0-6.4.
template <typename I>
__global__ __launch_bounds__(256) void copy_vec_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                       I nvec, I n) {
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    for (I base = tid; base < nvec; base += 2 * stride) {
        const I v1 = base + stride;
        const v4f x0 = ld4<true>(in + (size_t)base * 4);
        v4f x1{0, 0, 0, 0};
        if (v1 < nvec) x1 = ld4<true>(in + (size_t)v1 * 4);
        st4<true>(out + (size_t)base * 4, x0);
        if (v1 < nvec) st4<true>(out + (size_t)v1 * 4, x1);
    }
    if (blockIdx.x == 0) {
        const I t = nvec * 4 + threadIdx.x;
        if (t < n) out[t] = in[t];
    }
}

// out[i][j] = 0 + a[i] * b[j]: cblas_sger on a zeroed matrix (linalg.c:741-742) — the "0 +" matters
// only for the sign of zero products (-0 + +0 = +0).  Write-bound: 4 B/elem.
template <bool VEC, typename I>
__global__ __launch_bounds__(256) void outer_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                    float *__restrict__ out, I rows, I cols) {
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        const I cols4 = cols / 4, nvec = rows * cols4;
        for (I v = tid; v < nvec; v += stride) {
            const I i = v / cols4, j4 = v - i * cols4;
            const float x = a[i];
            const v4f y = *(const v4f *)(b + (size_t)j4 * 4);
            v4f r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = __fmaf_rn(x, y[k], 0.0f);
            __builtin_nontemporal_store(r, (v4f *)(out + (size_t)v * 4));
        }
    } else {
        const I n = rows * cols;
        for (I e = tid; e < n; e += stride) {
            const I i = e / cols;
            out[e] = __fmaf_rn(a[i], b[e - i * cols], 0.0f);
        }
    }
}

// The vector kernels' launch shape is what was measured fastest on MI355X for 1e8-float streams
// (tools/explore/add_bw.hip; profiles/r01/add_bw_explore.log, profiles/r01/ew_ab.log): no grid cap —
// every lane moves UNROLL = 2 float4 and retires, ~49k workgroups keep the dispatcher ahead of the
// memory system — with non-temporal loads and stores.  Capping the grid at a few workgroups per
// CU and grid-striding was 3-8 % slower, cached (non-nt) accesses 5-10 % slower, UNROLL 1/4/8
// 1-8 % slower than 2 on random data (add 6.28, exp 6.60, add+row 6.47 TB/s at UNROLL 2).
constexpr int kVecUnroll = 2;

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// FULL (op) ROW with whole float4 columns (cols % 4 == 0, at least one workgroup of them): a lane owns ONE float4 column of a
// block of RPT rows — the row operand's four values are loaded once and stay in registers, the RPT loads of the full operand
// are independent and in flight together, one multiply-high division per lane.  binary_vec_kernel's flat walk pays a 32-bit
// modulo and a second (cache-resident) load per float4 for the same result (profiles/r04/bcast2d_ab.log).  Same binary_apply, same bits.  blockIdx.x = column block (fastest: neighbouring workgroups stream
// neighbouring memory), blockIdx.y strides over the row blocks.
template <int OP, bool QUIRK, bool ROW_IS_A, int RPT>
__global__ __launch_bounds__(256) void binary_rows2d_kernel(const float *__restrict__ full, const float *__restrict__ row,
                                                            float *__restrict__ out, unsigned rows, unsigned cols, unsigned body_end,
                                                            unsigned items, unsigned div_m, unsigned div_s1, unsigned div_s2) {
    // work item = (row block, float4 column), column fastest, no padding of the last column block: ONE multiply-high division
    // per lane (for RPT float4s) instead of a modulo per float4
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= items) return;
    const unsigned cols4 = cols / 4, rb = fast_div(id, div_m, div_s1, div_s2), c0 = (id - rb * cols4) * 4, r0 = rb * RPT;
    const v4f rv = *(const v4f_u *)(row + c0);
    v4f x[RPT];
#pragma unroll
    for (int u = 0; u < RPT; ++u)
        if (r0 + u < rows) x[u] = ld4<true>(full + (size_t)(r0 + u) * cols + c0);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        if (r0 + u < rows) {
            const unsigned e = (r0 + u) * cols + c0;
            v4f r;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                r[k] = ROW_IS_A ? binary_apply<OP, QUIRK>(rv[k], x[u][k], (e + k) < body_end) : binary_apply<OP, QUIRK>(x[u][k], rv[k], (e + k) < body_end);
            st4<true>(out + (size_t)(r0 + u) * cols + c0, r);
        }
    }
}

// ---- binary dispatch ----

template <int OP, int AK, int BK, bool QUIRK, typename I>
int launch_binary_vec(const float *a, const float *b, float *out, size_t n, size_t cols,
                      size_t body_end, float ha, float hb) {
    const I nvec = (I)(n / 4), cols4 = (I)(cols / 4), tail = (I)(n / 4 * 4);
    unsigned grid = np::grid_for(n / 4 + 1, kVecUnroll, 0);
    hipStream_t s = np::stream();
    // FULL (op) ROW on whole float4 columns: the 2-D form (binary_rows2d_kernel; variant 8100: off).  Rows shorter than one
    // workgroup of float4s and vectors too long to stay cached (the column-block order below) keep the flat walk.
    if constexpr (((AK == NP_ROW && BK == NP_FULL) || (AK == NP_FULL && BK == NP_ROW)) && OP != NP_POW && sizeof(I) == 4) {
        // (measured in alternation, profiles/r04/bcast2d_ab.log: row (op) X +8-10 % everywhere; X (op) row +-1 % on rows of a few
        // thousand floats — the flat walk's modulo and second load are hidden there — and +2-4 % on rows of 10^5 and more)
        if (cols % 32 == 0 && cols >= 1024 && (AK == NP_ROW || cols >= 65536) && cols < (size_t(1) << 22) && n / cols >= 2 && np::g_ew_variant == 0 &&
            !np::g_bcast2d_off) {
            constexpr int RPT = 2;   // (as binary_vec_kernel's two float4 per lane: fatter lanes stream slower on this machine, 8 rows per lane lost 4 %)
            const size_t rows = n / cols, row_blocks = (rows + RPT - 1) / RPT, items = row_blocks * (cols / 4);   // (< 2^31: n is)
            unsigned dm, d1, d2;
            fast_div_magic(cols / 4, dm, d1, d2);
            const unsigned grid2 = (unsigned)((items + 255) / 256);
            if constexpr (AK == NP_ROW)
                binary_rows2d_kernel<OP, QUIRK, true, RPT><<<grid2, 256, 0, s>>>(b, a, out, (unsigned)rows, (unsigned)cols, (unsigned)body_end,
                                                                                   (unsigned)items, dm, d1, d2);
            else
                binary_rows2d_kernel<OP, QUIRK, false, RPT><<<grid2, 256, 0, s>>>(a, b, out, (unsigned)rows, (unsigned)cols, (unsigned)body_end,
                                                                                    (unsigned)items, dm, d1, d2);
            NP_LAUNCH_CHECK("binary_rows2d_kernel");
            return NP_OK;
        }
    }
    Ragged<I> rg{0, 0, 0, 0, 0, 0};
    // a ROW operand of >= 16 MB under a result of several rows: column-block order (Ragged::rowblock_rows; variant 8000: off).
    // 7 x 10^7 4.79 -> 5.71 TB/s, 3 x 3*10^7 4.84 -> 5.73; an 8 MB vector (40 x 2*10^6) is served by the Infinity Cache either
    // way and loses 2 % to the index arithmetic (tools/rowblock_ab.py, profiles/r04/rowblock_ab.log)
    if ((AK == NP_ROW || BK == NP_ROW) && OP != NP_POW && sizeof(I) == 4 && cols % 4 == 0 && cols >= (size_t(1) << 22) && n / cols >= 2 &&
        n / cols < (size_t(1) << 16) && np::g_ew_variant != 8000) {
        const size_t rows = n / cols, col_blocks = ((cols / 4 + 255) / 256 + 7) / 8 * 8;
        if (rows * col_blocks * 256 < (size_t(1) << 31)) {
            rg.rowblock_rows = (unsigned)rows;
            rg.wspace = (I)(rows * col_blocks * 256);
            grid = np::grid_for(rows * col_blocks * 256, kVecUnroll, 0);
        }
    }
    if ((AK == NP_ROW || AK == NP_COL || BK == NP_ROW || BK == NP_COL) && cols % 4 != 0) {
        rg.cols = (I)cols;
        if (cols > 1 && cols <= 0xffffffffull) fast_div_magic(cols, rg.m, rg.s1, rg.s2);   // (cols == 1: q = n)
    }
    // (the full unroll x nt sweep lives in tools/explore/add_bw.hip; only its winner is instantiated)
    if (OP == NP_POW && np::g_ew_variant != 9000) {   // the log2 table in registers (9000: the per-wave LDS copy, tools/pow_grid_ab.py)
        if constexpr (OP == NP_POW)
            binary_vec_kernel<OP, AK, BK, QUIRK, kVecUnroll, true, I, true><<<grid, 256, 0, s>>>(a, b, out, nvec, cols4, tail, (I)n,
                                                                                                (I)body_end, ha, hb, rg);
    } else {
        binary_vec_kernel<OP, AK, BK, QUIRK, kVecUnroll, true, I><<<grid, 256, 0, s>>>(a, b, out, nvec, cols4, tail, (I)n,
                                                                                      (I)body_end, ha, hb, rg);
    }
    NP_LAUNCH_CHECK("binary_vec_kernel");
    return NP_OK;
}

template <int OP, bool QUIRK, typename I>
int launch_binary_scalar(const float *a, int ak, const float *b, int bk, float *out, size_t n,
                         size_t cols, size_t body_end, float ha, float hb) {
    const unsigned grid = np::grid_for(n, 4, 16);
    binary_scalar_kernel<OP, QUIRK, I>
        <<<grid, 256, 0, np::stream()>>>(a, ak, b, bk, out, (I)n, (I)cols, (I)body_end, ha, hb);
    NP_LAUNCH_CHECK("binary_scalar_kernel");
    return NP_OK;
}

template <int OP, bool QUIRK, typename I>
int dispatch_binary_kinds(const float *a, int ak, const float *b, int bk, float *out, size_t rows,
                          size_t cols, size_t body_end, float ha, float hb) {
    const size_t n = rows * cols;
    // vector path: no alignment requirement (ld4 / st4 are dword-aligned float4 accesses) and no
    // row-length requirement (ragged broadcasts index per element, see fetch4)
    const bool vec = n >= 4;
    if (vec) {
#define NP_BK(AK_, BK_)                                                                     \
    if (ak == AK_ && bk == BK_)                                                             \
        return launch_binary_vec<OP, AK_, BK_, QUIRK, I>(a, b, out, n, cols, body_end, ha, hb)
        NP_BK(NP_FULL, NP_FULL);
        NP_BK(NP_FULL, NP_SCALAR);
        NP_BK(NP_SCALAR, NP_FULL);
        NP_BK(NP_FULL, NP_ROW);
        NP_BK(NP_ROW, NP_FULL);
        NP_BK(NP_FULL, NP_COL);
        NP_BK(NP_COL, NP_FULL);
#undef NP_BK
    }
    return launch_binary_scalar<OP, QUIRK, I>(a, ak, b, bk, out, n, cols, body_end, ha, hb);
}

template <int OP, bool QUIRK>
int dispatch_binary_index(const float *a, int ak, const float *b, int bk, float *out, size_t rows,
                          size_t cols, size_t body_end, float ha, float hb) {
    const size_t n = rows * cols;
    if (n < (size_t(1) << 31)) {
        if (body_end > n) body_end = n;
        return dispatch_binary_kinds<OP, QUIRK, uint32_t>(a, ak, b, bk, out, rows, cols, body_end, ha, hb);
    }
    return dispatch_binary_kinds<OP, QUIRK, uint64_t>(a, ak, b, bk, out, rows, cols, body_end, ha, hb);
}

template <int OP>
int dispatch_binary_quirk(const float *a, int ak, const float *b, int bk, float *out, size_t rows,
                          size_t cols, unsigned flags, size_t body_end, float ha, float hb) {
    constexpr bool has_quirk = (OP == NP_MULTIPLY || OP == NP_MOD || OP == NP_EQUAL || OP == NP_NOT_EQUAL);
    if constexpr (has_quirk) {
        if (flags & NP_QUIRK_AVX_BODY)
            return dispatch_binary_index<OP, true>(a, ak, b, bk, out, rows, cols, body_end, ha, hb);
    }
    return dispatch_binary_index<OP, false>(a, ak, b, bk, out, rows, cols, 0, ha, hb);
}

// ---- unary dispatch ----

template <int OP, typename I>
int launch_unary(const float *in, float *out, size_t n, float p0, float p1) {
    hipStream_t s = np::stream();
    if (n >= 4) {   // any alignment: see ld4 / st4
        const I nvec = (I)(n / 4), tail = (I)(n / 4 * 4);
        const unsigned grid = np::grid_for(n / 4 + 1, kVecUnroll, 0);
        unary_vec_kernel<OP, kVecUnroll, true, I><<<grid, 256, 0, s>>>(in, out, nvec, tail, (I)n, p0, p1);
        NP_LAUNCH_CHECK("unary_vec_kernel");
        return NP_OK;
    }
    const unsigned grid = np::grid_for(n, 4, 16);
    unary_scalar_kernel<OP, I><<<grid, 256, 0, s>>>(in, out, (I)n, p0, p1);
    NP_LAUNCH_CHECK("unary_scalar_kernel");
    return NP_OK;
}

template <int OP>
int dispatch_unary(const float *in, float *out, size_t n, float p0, float p1) {
    if (n < (size_t(1) << 31)) return launch_unary<OP, uint32_t>(in, out, n, p0, p1);
    return launch_unary<OP, uint64_t>(in, out, n, p0, p1);
}

}  // namespace

namespace np {
int g_ew_variant = 0;   // see np_elementwise_set_variant
int g_bcast2d_off = 0;

unsigned grid_for(size_t work_items, int per_thread, int blocks_per_cu) {
    const size_t threads = (work_items + per_thread - 1) / per_thread;
    size_t blocks = (threads + 255) / 256;
    if (blocks_per_cu > 0) {
        const size_t cap = (size_t)np::num_cus() * blocks_per_cu;
        if (blocks > cap) blocks = cap;
    }
    if (blocks > 0x7fffffffu) blocks = 0x7fffffffu;
    if (blocks < 1) blocks = 1;
    // a lane's UNROLL accesses are one grid apart: keep that distance off the powers of two (2^27 elements would
    // put them exactly 256 MiB apart, on the same HBM channel — np::capped_grid has the measurement)
    if (blocks >= 64) blocks |= 1;
    return (unsigned)blocks;
}

int device_copy(void *dst, const void *src, size_t bytes) {
    const size_t n = bytes / 4;
    const unsigned grid = grid_for(n / 4 + 1, 2, 0);
    if (n < (size_t(1) << 31))
        copy_vec_kernel<uint32_t><<<grid, 256, 0, np::stream()>>>((const float *)src, (float *)dst, (uint32_t)(n / 4), (uint32_t)n);
    else
        copy_vec_kernel<uint64_t><<<grid, 256, 0, np::stream()>>>((const float *)src, (float *)dst, (uint64_t)(n / 4), (uint64_t)n);
    NP_LAUNCH_CHECK("copy_vec_kernel");
    return NP_OK;
}
}  // namespace np

extern "C" {

int np_elementwise_set_variant(int variant) {
    if (variant == 8100 || variant == 8101) {   // 8100: broadcasts on the flat kernels as before round 4's 2-D forms (A/B), 8101: back
        np::g_bcast2d_off = variant == 8100;
        return NP_OK;
    }
    np::g_ew_variant = variant;
    return NP_OK;
}

int np_binary(int op, const float *a, int a_kind, const float *b, int b_kind, float *out,
              size_t rows, size_t cols, unsigned flags, size_t body_end) {
    if (op < 0 || op >= NP_BINARY_OP_COUNT)
        return np::fail(NP_ERR_INVALID, "np_binary: unknown op %d", op);
    if (a_kind < NP_FULL || a_kind > NP_HOST_SCALAR || b_kind < NP_FULL || b_kind > NP_HOST_SCALAR)
        return np::fail(NP_ERR_INVALID, "np_binary: unknown operand kind (%d, %d)", a_kind, b_kind);
    if (rows == 0 || cols == 0) return NP_OK;
    if (!a || !b || !out) return np::fail(NP_ERR_INVALID, "np_binary: null pointer");
    if (int rc = np::ensure_init()) return rc;
    // host scalars travel by value (kernel argument); the kernels see kind SCALAR + null pointer
    float ha = 0.0f, hb = 0.0f;
    if (a_kind == NP_HOST_SCALAR) { ha = *a; a = nullptr; a_kind = NP_SCALAR; }
    if (b_kind == NP_HOST_SCALAR) { hb = *b; b = nullptr; b_kind = NP_SCALAR; }
    switch (op) {
        case NP_ADD: return dispatch_binary_quirk<NP_ADD>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_SUBTRACT: return dispatch_binary_quirk<NP_SUBTRACT>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_MULTIPLY: return dispatch_binary_quirk<NP_MULTIPLY>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_DIVIDE: return dispatch_binary_quirk<NP_DIVIDE>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_MOD: return dispatch_binary_quirk<NP_MOD>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_POW:
            // `$a ** 2`: x * x is the correctly rounded square (what powf returns in all but its rare
            // non-correctly-rounded cases) and has the same zeros / infinities / NaNs, at the cost of an add
            if (a_kind == NP_FULL && b_kind == NP_SCALAR && !b && hb == 2.0f)
                return dispatch_binary_quirk<NP_MULTIPLY>(a, NP_FULL, a, NP_FULL, out, rows, cols, 0u, 0, 0.0f, 0.0f);
            return dispatch_binary_quirk<NP_POW>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_EQUAL: return dispatch_binary_quirk<NP_EQUAL>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_NOT_EQUAL: return dispatch_binary_quirk<NP_NOT_EQUAL>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_GREATER: return dispatch_binary_quirk<NP_GREATER>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_GREATER_EQUAL: return dispatch_binary_quirk<NP_GREATER_EQUAL>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_LESS: return dispatch_binary_quirk<NP_LESS>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_LESS_EQUAL: return dispatch_binary_quirk<NP_LESS_EQUAL>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_MAXIMUM: return dispatch_binary_quirk<NP_MAXIMUM>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        case NP_MINIMUM: return dispatch_binary_quirk<NP_MINIMUM>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
        default: return dispatch_binary_quirk<NP_ARCTAN2>(a, a_kind, b, b_kind, out, rows, cols, flags, body_end, ha, hb);
    }
}

int np_unary(int op, const float *in, float *out, size_t n, float p0, float p1) {
    if (op < 0 || op >= NP_UNARY_OP_COUNT)
        return np::fail(NP_ERR_INVALID, "np_unary: unknown op %d", op);
    if (n == 0) return NP_OK;
    if (!in || !out) return np::fail(NP_ERR_INVALID, "np_unary: null pointer");
    if (int rc = np::ensure_init()) return rc;
    // float_round: factor = powf(10, decimals), evaluated once with the host libm (the same
    // glibc powf the reference calls per element, double_math.c:255).
    if (op == NP_ROUND) p0 = powf(10.0f, p0);
#define NP_U(OP_) case OP_: return dispatch_unary<OP_>(in, out, n, p0, p1)
    switch (op) {
        NP_U(NP_ABS); NP_U(NP_SQRT); NP_U(NP_EXP); NP_U(NP_EXP2); NP_U(NP_EXPM1); NP_U(NP_LOG);
        NP_U(NP_LOG2); NP_U(NP_LOG10); NP_U(NP_LOG1P); NP_U(NP_LOGB); NP_U(NP_SIN); NP_U(NP_COS);
        NP_U(NP_TAN); NP_U(NP_ARCSIN); NP_U(NP_ARCCOS); NP_U(NP_ARCTAN); NP_U(NP_DEGREES);
        NP_U(NP_RADIANS); NP_U(NP_SINH); NP_U(NP_COSH); NP_U(NP_TANH); NP_U(NP_ARCSINH);
        NP_U(NP_ARCCOSH); NP_U(NP_ARCTANH); NP_U(NP_RINT); NP_U(NP_FIX); NP_U(NP_FLOOR);
        NP_U(NP_CEIL); NP_U(NP_TRUNC); NP_U(NP_SINC); NP_U(NP_NEGATE); NP_U(NP_SIGN); NP_U(NP_CLIP);
        NP_U(NP_ROUND); NP_U(NP_RSQRT); NP_U(NP_POSITIVE); NP_U(NP_RECIPROCAL);
        default: break;
    }
#undef NP_U
    return np::fail(NP_ERR_INVALID, "np_unary: unknown op %d", op);
}

int np_outer(const float *a, size_t m, const float *b, size_t n, float *out) {
    if (m == 0 || n == 0) return NP_OK;
    if (!a || !b || !out) return np::fail(NP_ERR_INVALID, "np_outer: null pointer");
    if (int rc = np::ensure_init()) return rc;
    const size_t total = m * n;
    const bool vec = n % 4 == 0 && aligned16(b) && aligned16(out);
    const unsigned grid = np::grid_for(vec ? total / 4 : total, vec ? 2 : 4, 0);
    hipStream_t s = np::stream();
    if (total < (size_t(1) << 31)) {
        if (vec)
            outer_kernel<true, uint32_t><<<grid, 256, 0, s>>>(a, b, out, (uint32_t)m, (uint32_t)n);
        else
            outer_kernel<false, uint32_t><<<grid, 256, 0, s>>>(a, b, out, (uint32_t)m, (uint32_t)n);
    } else {
        if (vec)
            outer_kernel<true, uint64_t><<<grid, 256, 0, s>>>(a, b, out, (uint64_t)m, (uint64_t)n);
        else
            outer_kernel<false, uint64_t><<<grid, 256, 0, s>>>(a, b, out, (uint64_t)m, (uint64_t)n);
    }
    NP_LAUNCH_CHECK("outer_kernel");
    return NP_OK;
}

int np_fill(float *dev_ptr, float value, size_t n) {
    if (n == 0) return NP_OK;
    if (!dev_ptr) return np::fail(NP_ERR_INVALID, "np_fill: null pointer");
    if (int rc = np::ensure_init()) return rc;
    // peel to a 16-byte boundary (row views start anywhere)
    size_t head = ((16 - ((uintptr_t)dev_ptr & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    const unsigned grid = np::grid_for(nvec + 1, 2, 0);   // write-only stream: uncapped grid, non-temporal stores
    if (n < (size_t(1) << 31))
        fill_kernel<uint32_t><<<grid, 256, 0, np::stream()>>>(dev_ptr, value, (uint32_t)n,
                                                              (uint32_t)head, (uint32_t)nvec);
    else
        fill_kernel<uint64_t><<<grid, 256, 0, np::stream()>>>(dev_ptr, value, (uint64_t)n,
                                                              (uint64_t)head, (uint64_t)nvec);
    NP_LAUNCH_CHECK("fill_kernel");
    return NP_OK;
}

}  // extern "C"
