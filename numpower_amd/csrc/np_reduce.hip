// Reductions of libnp_hip.so: full reductions (sum / prod / min / max / mean) and single-axis
// reductions over a contiguous array viewed as outer x axis_len x inner.  (argmax / argmin: np_argreduce.hip;
// moments, weighted sums, mismatch counts and all(): np_stats.hip.)
//
// HBM-bound: every input element is read exactly once with 16-byte lane accesses; cross-lane
// combines use wave64 shuffles (DPP / ds_bpermute), cross-wave combines go through LDS, and
// cross-workgroup combines are a deterministic second pass over per-workgroup partials (no float
// atomics: the reference's atomicAdd kernels, cuda_math.cu:777-828, are order-nondeterministic
// and its prod kernel is wrong).
//
// Reference behaviour restated:
//   NDArray_Sum_Float / NDArray_Float_Prod / NDArray_Mean_Float   src/ndmath/arithmetics.c:36-102
//   NDArray_Min / NDArray_Max                                      src/ndarray.c:752-772,939-959
//   reduce() / _reduce() / apply_reduce()                          src/ndarray.c:523-578,394-429,358-368
// The reference accumulates strictly left to right in fp32; the tree order used here differs in
// rounding (it is closer to the exact sum).  tests/ pin both against an fp64 accumulation.
#include <float.h>
#include <math.h>

#include "np_internal.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_u __attribute__((aligned(4)));   // float4 access that only assumes dword alignment

using namespace np::dev;   // r_identity / r_combine / wave_reduce / block_reduce (np_internal.h)

int g_small_inner_dword = 0;    // reduce_small_inner: 1 = the dword walk of rounds 1-5 (np_reduce_set_variant(4300001): A/B)
// np_debug_reduce_last_path: the NP_REDUCE_PATH_* bits of what the last np_reduce_axis / np_reduce_all(_dev) call launched, its
// recursion on partials included.  A plain process global, cleared at the top of those entry points.
unsigned g_last_path = 0;

// ------------------------------------------------------------------------------------------
// full reduction
// ------------------------------------------------------------------------------------------

// pass 1: each workgroup reduces a grid-strided share of the input to one partial.
// `in` must be 16-byte aligned at in + head; head/tail elements are folded in by block 0.
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_all_pass1(const float *__restrict__ in,
                                                        float *__restrict__ partials, I n, I head,
                                                        I nvec, unsigned *__restrict__ ticket,
                                                        float *__restrict__ out, float mean_count) {
    __shared__ float lds4[4];
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    const float id = r_identity<OP>();
    // 4 independent float4 accumulators = 16 loads-worth of ILP per lane
    v4f acc0{id, id, id, id}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    const float *base = in + head;
    I v = tid;
    for (; v + 3 * stride < nvec; v += 4 * stride) {
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + stride) * 4));
        const v4f x2 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + 2 * stride) * 4));
        const v4f x3 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + 3 * stride) * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc0[k] = r_combine<OP>(acc0[k], x0[k]);
            acc1[k] = r_combine<OP>(acc1[k], x1[k]);
            acc2[k] = r_combine<OP>(acc2[k], x2[k]);
            acc3[k] = r_combine<OP>(acc3[k], x3[k]);
        }
    }
    if (v < nvec) {
        // what is left — at most three vectors per lane — is issued together too: one load per iteration was three memory round
        // trips one behind the other at the very end of every workgroup (~5 % of a 10^8-element pass, a third of a 10^6-element one)
        const I v1 = v + stride, v2 = v + 2 * stride;
        const bool h1 = v1 < nvec, h2 = v2 < nvec;
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v * 4));
        v4f x1{id, id, id, id}, x2 = x1;
        if (h1) x1 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v1 * 4));
        if (h2) x2 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v2 * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc0[k] = r_combine<OP>(acc0[k], x0[k]);
            if (h1) acc1[k] = r_combine<OP>(acc1[k], x1[k]);
            if (h2) acc2[k] = r_combine<OP>(acc2[k], x2[k]);
        }
    }
    float r = id;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r = r_combine<OP>(r, r_combine<OP>(r_combine<OP>(acc0[k], acc1[k]),
                                          r_combine<OP>(acc2[k], acc3[k])));
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) r = r_combine<OP>(r, in[threadIdx.x]);
        const I t = head + nvec * 4 + threadIdx.x;
        if (t < n) r = r_combine<OP>(r, in[t]);
    }
    r = block_reduce<OP>(r, lds4);
    fold_in_last_workgroup<OP>(r, partials, ticket, out, mean_count, lds4, n ? in : nullptr);   // ticket == nullptr: pass 2 folds
}

// pass 2: one workgroup folds the partials; MEAN divides by the element count at the end
// (`value / numElements`, arithmetics.c:89, numpower.c:2659).  `first`: position 0 of the input the partials came from, for
// the NaN rule of NP_MIN / NP_MAX (r_first_nan); nullptr when the caller has none.
template <int OP>
__global__ __launch_bounds__(256) void reduce_all_pass2(const float *__restrict__ partials, int np,
                                                        float *__restrict__ out, float count,
                                                        const float *__restrict__ first = nullptr) {
    __shared__ float lds4[4];
    // thread t folds partials t, t + 256, ... in that order; eight loads are in flight before the first is used (one load -> add
    // round trip per iteration was ~6 us for the 2049 partials of a 10^8-element reduction); lanes past the end fold the identity,
    // which changes no bit (x + 0, x * 1, min(x, +inf), max(x, -inf))
    float r = r_identity<OP>(), p0 = 0.0f;
    for (int base = 0; base < np; base += 8 * (int)blockDim.x) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * (int)blockDim.x + (int)threadIdx.x;
            v[u] = i < np ? partials[i] : r_identity<OP>();
        }
        if (base == 0) p0 = v[0];   // thread 0: partial 0
#pragma unroll
        for (int u = 0; u < 8; ++u) r = r_combine<OP>(r, v[u]);
    }
    r = block_reduce<OP>(r, lds4);
    if (threadIdx.x == 0) {
        if constexpr (OP == NP_MEAN) r = __fdiv_rn(r, count);
        // (a NaN partial 0: the chain kernels' way of handing over the NaN of position 0, fold_in_last_workgroup)
        out[0] = r_first_nan<OP>(r_first_nan<OP>(r, first), &p0);
    }
}

template <int OP, typename I>
int launch_reduce_all(const float *in, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    size_t head = ((16 - ((uintptr_t)in & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    // enough workgroups to fill the chip (8 per CU), but never more than one per 4 KiB of input
    size_t blocks = np::capped_grid((nvec + 255) / 256, np::stream_cap());
    // (A/B, np_reduce_set_variant(3000000 + N): a few MB on N fat workgroups, so that one ticket and one fold load per thread do)
    // (up to 2^20 elements: at 4 M the 128 workgroups — half the CUs — take longer to stream 16 MB than the second launch costs:
    // 15.1 against 12.2 us, profiles/r05/reduce_small_ab_final.log)
    if (np::g_small_reduce_blocks && n <= (size_t(1) << 20) && blocks > np::g_small_reduce_blocks) blocks = np::g_small_reduce_blocks;
    np::Scratch partials;
    if (int rc = partials.alloc(blocks * sizeof(float))) return rc;
    // small grids: the last workgroup to finish folds the partials, no second launch (np_internal.h)
    unsigned *ticket = np::fold_ticket(blocks);
    reduce_all_pass1<OP, I><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)partials.ptr, (I)n, (I)head, (I)nvec,
                                                           ticket, dev_out, (float)n);
    NP_LAUNCH_CHECK("reduce_all_pass1");
    g_last_path |= ticket ? NP_REDUCE_PATH_ALL_ONE_LAUNCH : NP_REDUCE_PATH_ALL_TWO_LAUNCHES;
    if (ticket) return NP_OK;
    reduce_all_pass2<OP><<<1, 256, 0, s>>>((const float *)partials.ptr, (int)blocks, dev_out,
                                           (float)n, n ? in : nullptr);
    NP_LAUNCH_CHECK("reduce_all_pass2");
    return NP_OK;
}

}  // namespace

namespace np {
// Fold `n` per-workgroup partials (a few thousand at most) into one device float with ONE one-block launch — what a
// first pass that already reduced per workgroup needs behind it (np_reduce_all_dev on the partials would be a
// first pass of its own plus this: two launches, ~10 us, for 16 KB).
int fold_partials(int op, const float *partials, size_t n, float *dev_out) {
    if (n > 0x7fffffffu) return np::fail(NP_ERR_INVALID, "fold_partials: too many partials");
    hipStream_t s = np::stream();
    switch (op) {
        case NP_SUM: reduce_all_pass2<NP_SUM><<<1, 256, 0, s>>>(partials, (int)n, dev_out, 1.0f); break;
        case NP_PROD: reduce_all_pass2<NP_PROD><<<1, 256, 0, s>>>(partials, (int)n, dev_out, 1.0f); break;
        case NP_MIN: reduce_all_pass2<NP_MIN><<<1, 256, 0, s>>>(partials, (int)n, dev_out, 1.0f); break;
        case NP_MAX: reduce_all_pass2<NP_MAX><<<1, 256, 0, s>>>(partials, (int)n, dev_out, 1.0f); break;
        default: return np::fail(NP_ERR_INVALID, "fold_partials: unknown reduction %d", op);
    }
    NP_LAUNCH_CHECK("reduce_all_pass2");
    return NP_OK;
}
}  // namespace np

namespace {

template <int OP>
int dispatch_reduce_all(const float *in, size_t n, float *dev_out) {
    if (n < (size_t(1) << 31)) return launch_reduce_all<OP, uint32_t>(in, n, dev_out);
    return launch_reduce_all<OP, uint64_t>(in, n, dev_out);
}

// ------------------------------------------------------------------------------------------
// axis reduction, inner >= 4: "column" reduce
// ------------------------------------------------------------------------------------------
//
// View: in[outer][axis_len][inner] — any inner: rows need not start on a 16-byte boundary (dword-aligned float4
// accesses), and the last group of a row with inner % 4 != 0 handles its 1-3 columns one by one.
// A workgroup owns a tile of 64 float4 columns (256 floats of
// the inner dimension) and one of `splits` contiguous chunks of the axis; its 4 waves walk
// interleaved rows of the chunk (each wave-level load is one contiguous 1 KiB segment of a row),
// keep ROWS_IN_FLIGHT independent loads in flight, and combine through LDS at the end.
// out_partial[outer][splits][inner]; with splits == 1 this is the final result.
//
// FINAL applies the epilogue: MIN / MAX -> the NaN rule of position 0 (first / first_axis: the array the caller was given and
// its axis length; r_first_nan); MEAN -> divide by axis_len; PROD with the AVX-body quirk ->
// zero results take the sign the reference's repeated Multiply_Float leaves behind
// (arithmetics.c:403,410-412): -0.0f for inner index < body_end, +0.0f after it.
template <int OP, bool FINAL, typename I>
__global__ __launch_bounds__(256) void reduce_axis_cols(const float *__restrict__ in,
                                                        float *__restrict__ out, I axis_len,
                                                        I inner, I splits, float mean_div,
                                                        int prod_quirk, I body_end, unsigned xcd_runs = 0,
                                                        const float *__restrict__ first = nullptr, I first_axis = 0) {
    __shared__ v4f lds[3][64];
    const I inner4 = (inner + 3) / 4;   // column groups per row; the last one may hold fewer than 4 columns
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned tile = blockIdx.x, split_u = blockIdx.y, o_u = blockIdx.z;
    if (xcd_runs) {
        // rows that are not whole 128-byte lines: neighbouring tiles share a line at each end of their 1 KiB piece of a row;
        // dealt to the XCDs in eight contiguous runs they share it in ONE L2 instead of fetching it twice (round 6, first
        // measured on argreduce_cols_tile: 9973^2 fetched 1.14 x its bytes, 1.08 x this way; np_sgemm.hip's tile_coords bijection)
        const unsigned T = gridDim.x, S = gridDim.y, W = T * S * gridDim.z;
        const unsigned L = blockIdx.x + T * (blockIdx.y + S * blockIdx.z);
        const unsigned q = W / 8, r = W % 8, xcd = L % 8, idx = L / 8;
        const unsigned unit = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        tile = unit % T;
        split_u = (unit / T) % S;
        o_u = unit / (T * S);
    }
    const I col4 = (I)tile * 64 + lane;
    const I split = split_u;
    const I o = o_u;
    const I chunk = (axis_len + splits - 1) / splits;
    const I r0 = split * chunk;
    I r1 = r0 + chunk;
    if (r1 > axis_len) r1 = axis_len;
    const float id = r_identity<OP>();
    v4f acc0{id, id, id, id}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    const I valid = col4 < inner4 ? (inner - col4 * 4 < 4 ? inner - col4 * 4 : (I)4) : (I)0;   // columns this lane owns
    if (valid > 0) {
        // A ragged last group (valid < 4) loads whole float4s like everyone else — the 1-3 extra floats are the start
        // of the next row and are never stored — except on the very last row of the array, where they would lie past
        // the buffer: that one row it reads element by element.
        const bool past_end = valid < 4 && o == (I)gridDim.z - 1 && r1 == axis_len;
        const I r1v = past_end ? r1 - 1 : r1;
        const size_t row_stride = (size_t)inner;
        const float *p = in + (size_t)o * axis_len * row_stride + (size_t)col4 * 4;
        I r = r0 + wave;
        for (; r + 12 < r1v; r += 16) {
            const v4f x0 = __builtin_nontemporal_load((const v4f_u *)(p + (size_t)r * row_stride));
            const v4f x1 = __builtin_nontemporal_load((const v4f_u *)(p + (size_t)(r + 4) * row_stride));
            const v4f x2 = __builtin_nontemporal_load((const v4f_u *)(p + (size_t)(r + 8) * row_stride));
            const v4f x3 = __builtin_nontemporal_load((const v4f_u *)(p + (size_t)(r + 12) * row_stride));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc0[k] = r_combine<OP>(acc0[k], x0[k]);
                acc1[k] = r_combine<OP>(acc1[k], x1[k]);
                acc2[k] = r_combine<OP>(acc2[k], x2[k]);
                acc3[k] = r_combine<OP>(acc3[k], x3[k]);
            }
        }
        for (; r < r1v; r += 4) {
            const v4f x0 = *(const v4f_u *)(p + (size_t)r * row_stride);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc0[k] = r_combine<OP>(acc0[k], x0[k]);
        }
        if (past_end && r == r1v) {   // this wave's turn in the interleave falls on the last row
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((I)k < valid) acc0[k] = r_combine<OP>(acc0[k], p[(size_t)r * row_stride + k]);
        }
    }
    v4f acc;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        acc[k] = r_combine<OP>(r_combine<OP>(acc0[k], acc1[k]), r_combine<OP>(acc2[k], acc3[k]));
    if (wave > 0) lds[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && valid > 0) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const v4f t = lds[w][lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = r_combine<OP>(acc[k], t[k]);
        }
        if constexpr (FINAL) {
            if constexpr (OP == NP_MEAN) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __fdiv_rn(acc[k], mean_div);
            }
            if constexpr (OP == NP_PROD) {
                if (prod_quirk) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (acc[k] == 0.0f) acc[k] = (col4 * 4 + k < body_end) ? -0.0f : 0.0f;
                }
            }
            if constexpr (OP == NP_MIN || OP == NP_MAX) {
                if (first) {   // position 0 of each column's slice in the ORIGINAL array (this launch may fold partials)
                    const float *f0 = first + (size_t)o * first_axis * (size_t)inner + (size_t)col4 * 4;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((I)k < valid) acc[k] = r_first_nan<OP>(acc[k], f0 + k);
                }
            }
        }
        float *q = out + ((size_t)o * splits + split) * (size_t)inner + (size_t)col4 * 4;
        if (valid == 4) {
            *(v4f_u *)q = acc;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((I)k < valid) q[k] = acc[k];
        }
    }
}

// ------------------------------------------------------------------------------------------
// axis reduction, generic: one thread per output element, sequential over the axis.
// Used for ragged inner sizes (inner % 4 != 0, misaligned views) and tiny problems.
// ------------------------------------------------------------------------------------------
// The axis may be cut into `chunks` pieces of `chunk_len` rows (out[outer][chunks][inner], a later
// pass folds the chunks): with few outputs and a long axis that is what puts enough threads on the
// machine.  The epilogue (MEAN division, PROD zero sign) runs only when chunks == 1.
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_axis_generic(const float *__restrict__ in,
                                                           float *__restrict__ out, I outer,
                                                           I axis_len, I inner, float mean_div,
                                                           int prod_quirk, I body_end, I chunks,
                                                           I chunk_len, const float *__restrict__ first = nullptr,
                                                           I first_axis = 0) {
    const I total = outer * chunks * inner;
    const I stride = (I)gridDim.x * blockDim.x;
    for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const I oc = idx / inner, j = idx - oc * inner;
        const I o = oc / chunks, c = oc - o * chunks;
        const I a0 = c * chunk_len;
        I a1 = a0 + chunk_len;
        if (a1 > axis_len) a1 = axis_len;
        const float *p = in + (size_t)o * axis_len * inner + j;
        float r = r_identity<OP>();
        I a = a0;
        if (a < a1) r = p[(size_t)a++ * inner];
        // 4 independent loads in flight per thread
        float r1 = r_identity<OP>(), r2 = r1, r3 = r1;
        for (; a + 3 < a1; a += 4) {
            const float x0 = p[(size_t)a * inner], x1 = p[(size_t)(a + 1) * inner];
            const float x2 = p[(size_t)(a + 2) * inner], x3 = p[(size_t)(a + 3) * inner];
            r = r_combine<OP>(r, x0);
            r1 = r_combine<OP>(r1, x1);
            r2 = r_combine<OP>(r2, x2);
            r3 = r_combine<OP>(r3, x3);
        }
        for (; a < a1; ++a) r = r_combine<OP>(r, p[(size_t)a * inner]);
        r = r_combine<OP>(r_combine<OP>(r, r1), r_combine<OP>(r2, r3));
        if (chunks == 1) {
            if constexpr (OP == NP_MEAN) r = __fdiv_rn(r, mean_div);
            if constexpr (OP == NP_PROD) {
                if (prod_quirk && r == 0.0f) r = (j < body_end) ? -0.0f : 0.0f;
            }
            r = r_first_nan<OP>(r, first ? first + (size_t)o * first_axis * inner + j : nullptr);
        }
        out[idx] = r;
    }
}

// ------------------------------------------------------------------------------------------
// axis reduction, small inner (2..128 columns: column sums of an N x 3 point cloud): the generic
// kernel would give each of the few columns ONE thread.  Here a workgroup reads its slab of rows as
// flat memory (coalesced dword loads); with T = (256 / inner) * inner active threads and a stride
// of T the column of a thread never changes (t % inner), so it accumulates in a register; LDS folds
// the T / inner partials of each column.  out[outer][blocks][inner].
// ------------------------------------------------------------------------------------------
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_small_inner(const float *__restrict__ in,
                                                          float *__restrict__ out, I axis_len,
                                                          I inner, I rows_per_block) {
    __shared__ float lds[256];
    const unsigned T = (256u / (unsigned)inner) * (unsigned)inner;
    const I o = blockIdx.y, b = blockIdx.x;
    const I r0 = b * rows_per_block;
    I r1 = r0 + rows_per_block;
    if (r1 > axis_len) r1 = axis_len;
    const size_t cnt = (size_t)(r1 - r0) * inner;
    const float *p = in + ((size_t)o * axis_len + r0) * inner;
    const float id = r_identity<OP>();
    float a0 = id, a1 = id, a2 = id, a3 = id;
    if (threadIdx.x < T) {
        size_t e = threadIdx.x;
        for (; e + 3 * (size_t)T < cnt; e += 4 * (size_t)T) {
            const float x0 = p[e], x1 = p[e + T], x2 = p[e + 2 * (size_t)T], x3 = p[e + 3 * (size_t)T];
            a0 = r_combine<OP>(a0, x0);
            a1 = r_combine<OP>(a1, x1);
            a2 = r_combine<OP>(a2, x2);
            a3 = r_combine<OP>(a3, x3);
        }
        for (; e < cnt; e += T) a0 = r_combine<OP>(a0, p[e]);
    }
    lds[threadIdx.x] = r_combine<OP>(r_combine<OP>(a0, a1), r_combine<OP>(a2, a3));
    __syncthreads();
    if (threadIdx.x < (unsigned)inner) {
        float r = lds[threadIdx.x];
        for (unsigned k = threadIdx.x + (unsigned)inner; k < T; k += (unsigned)inner) r = r_combine<OP>(r, lds[k]);
        out[((size_t)o * gridDim.x + b) * inner + threadIdx.x] = r;
    }
}

// The same slab walked with FLOAT4 loads (round 6; the form np_argreduce's small-inner kernels took in round 5: N x 3 argmax 6.1 TB/s
// where this sum ran 4.8).  A thread's vector v = t + j T starts at flat element 4 t + 4 j T, and 4 j T is a whole number of rows
// (T is a multiple of inner): component k of thread t stays in column (4 t + k) % inner for the whole walk.  Four loads in flight, four
// times the bytes of the dword walk above.  Needs the slab to start on a 16-byte boundary: `in` aligned, rows_per_block % 4 == 0 and
// (outer == 1 or axis_len * inner % 4 == 0) — the host checks; else the dword kernel.  out[outer][blocks][inner].
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_small_inner_v4(const float *__restrict__ in, float *__restrict__ out, I axis_len,
                                                             I inner, I rows_per_block) {
    __shared__ float lds[1024];
    const unsigned T = (256u / (unsigned)inner) * (unsigned)inner;
    const I o = blockIdx.y, b = blockIdx.x;
    const I r0 = b * rows_per_block;
    const I r1 = axis_len - r0 < rows_per_block ? axis_len : r0 + rows_per_block;
    const size_t cnt = (size_t)(r1 - r0) * inner, nvec = cnt >> 2;
    const float *p = in + ((size_t)o * axis_len + r0) * inner;
    const float id = r_identity<OP>();
    const unsigned t = threadIdx.x;
    if (t < T) {
        v4f a0{id, id, id, id}, a1 = a0, a2 = a0, a3 = a0;
        size_t v = t;
        for (; v + 3 * (size_t)T < nvec; v += 4 * (size_t)T) {
            const v4f x0 = __builtin_nontemporal_load((const v4f *)(p + v * 4));
            const v4f x1 = __builtin_nontemporal_load((const v4f *)(p + (v + T) * 4));
            const v4f x2 = __builtin_nontemporal_load((const v4f *)(p + (v + 2 * (size_t)T) * 4));
            const v4f x3 = __builtin_nontemporal_load((const v4f *)(p + (v + 3 * (size_t)T) * 4));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[k] = r_combine<OP>(a0[k], x0[k]);
                a1[k] = r_combine<OP>(a1[k], x1[k]);
                a2[k] = r_combine<OP>(a2[k], x2[k]);
                a3[k] = r_combine<OP>(a3[k], x3[k]);
            }
        }
        if (v < nvec) {   // at most three vectors are left per lane: issued together
            const bool h1 = v + T < nvec, h2 = v + 2 * (size_t)T < nvec;
            const v4f x0 = __builtin_nontemporal_load((const v4f *)(p + v * 4));
            v4f x1{id, id, id, id}, x2 = x1;
            if (h1) x1 = __builtin_nontemporal_load((const v4f *)(p + (v + T) * 4));
            if (h2) x2 = __builtin_nontemporal_load((const v4f *)(p + (v + 2 * (size_t)T) * 4));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[k] = r_combine<OP>(a0[k], x0[k]);
                a1[k] = r_combine<OP>(a1[k], x1[k]);
                a2[k] = r_combine<OP>(a2[k], x2[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) lds[4 * t + k] = r_combine<OP>(r_combine<OP>(a0[k], a1[k]), r_combine<OP>(a2[k], a3[k]));
    }
    __syncthreads();
    // entry e = m * inner + c (m < 4 T / inner) belongs to column c: halve the m range until one entry per column is left
    for (unsigned mcur = 4 * T / (unsigned)inner; mcur > 1;) {
        const unsigned half = (mcur + 1) / 2;
        for (unsigned idx = t; idx < (mcur - half) * (unsigned)inner; idx += 256) lds[idx] = r_combine<OP>(lds[idx], lds[idx + half * (unsigned)inner]);
        __syncthreads();
        mcur = half;
    }
    if (t < (unsigned)inner) {
        float r = lds[t];
        for (size_t e = 4 * nvec; e < cnt; ++e)                 // the <= 3 leftover elements of the slab
            if (e % inner == t) r = r_combine<OP>(r, p[e]);
        out[((size_t)o * gridDim.x + b) * inner + t] = r;
    }
}

// ------------------------------------------------------------------------------------------
// axis reduction, inner == 1: "row" reduce.  LPR lanes cooperate on one row (LPR = 64: one wave
// per row; 256: one workgroup per row), reading the row with coalesced accesses.
// ------------------------------------------------------------------------------------------
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_rows_wave(const float *__restrict__ in,
                                                        float *__restrict__ out, I rows, I len,
                                                        float mean_div, int prod_quirk,
                                                        const float *__restrict__ first = nullptr, I first_axis = 0) {
    const int lane = threadIdx.x & 63;
    const I row = (I)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *p = in + (size_t)row * len;
    const float id = r_identity<OP>();
    float r = id;
    // peel to 16-byte alignment, then float4
    I head = (I)(((16 - ((uintptr_t)p & 15u)) & 15u) / 4);
    if (head > len) head = len;
    if ((I)lane < head) r = p[lane];
    const I nvec = (len - head) / 4;
    v4f acc{id, id, id, id};
    for (I v = lane; v < nvec; v += 64) {
        const v4f x = *(const v4f *)(p + head + (size_t)v * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = r_combine<OP>(acc[k], x[k]);
    }
    r = r_combine<OP>(r, r_combine<OP>(r_combine<OP>(acc[0], acc[1]), r_combine<OP>(acc[2], acc[3])));
    const I t = head + nvec * 4 + lane;
    if (t < len) r = r_combine<OP>(r, p[t]);
    r = wave_reduce<OP>(r);
    if (lane == 0) {
        if constexpr (OP == NP_MEAN) r = __fdiv_rn(r, mean_div);
        // inner == 1: the reference multiplies one-element slices, i.e. always in the scalar tail,
        // which turns a zero product of either sign into +0.0 (arithmetics.c:410-412)
        if constexpr (OP == NP_PROD) {
            if (prod_quirk && r == 0.0f) r = 0.0f;
        }
        out[row] = r_first_nan<OP>(r, first ? first + (size_t)row * first_axis : nullptr);
    }
}

// Short rows (5 .. ~500 elements): L lanes per row (L = 2 .. 32, a power of two), 64 / L rows per wave.
// A wave per row would use 8 of its 64 lanes on a 33-element row (0.7 TB/s); a thread per row reads
// with a large stride.  Lanes of a group read the row interleaved (coalesced inside the group,
// neighbouring groups read neighbouring rows) and fold with xor-shuffles.
template <int OP, int L, typename I>
__global__ __launch_bounds__(256) void reduce_rows_group(const float *__restrict__ in, float *__restrict__ out,
                                                         I rows, I len, float mean_div, int prod_quirk,
                                                         const float *__restrict__ first = nullptr, I first_axis = 0) {
    const I row = ((I)blockIdx.x * 256 + threadIdx.x) / L;
    const unsigned l = threadIdx.x % L;
    float r = r_identity<OP>();
    if (row < rows) {
        const float *p = in + (size_t)row * len;
        float r1 = r;
        I j = l;
        for (; j + L < len; j += 2 * L) {
            r = r_combine<OP>(r, p[j]);
            r1 = r_combine<OP>(r1, p[j + L]);
        }
        if (j < len) r = r_combine<OP>(r, p[j]);
        r = r_combine<OP>(r, r1);
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) r = r_combine<OP>(r, __shfl_xor(r, off, 64));
    if (l == 0 && row < rows) {
        if constexpr (OP == NP_MEAN) r = __fdiv_rn(r, mean_div);
        if constexpr (OP == NP_PROD) {
            if (prod_quirk && r == 0.0f) r = 0.0f;   // see reduce_rows_wave
        }
        out[row] = r_first_nan<OP>(r, first ? first + (size_t)row * first_axis : nullptr);
    }
}


// Short rows, very many of them (a 10^7 x 10 matrix summed along axis 1 — softmax denominators): the lanes of
// reduce_rows_group read 4 bytes each at the row stride, N load instructions per wave for what is one contiguous span.
// Here a workgroup copies a contiguous slab of R rows into LDS with coalesced float4 loads and every thread folds its
// rows out of LDS (row pitch len | 1 words: an even pitch would put a wave's lanes on a few banks).  Needs a 16-byte
// aligned input and R * len % 4 == 0 (R is a multiple of 256).  Same technique as sgemv_staged_rows_kernel (np_sgemm.hip).
template <int OP>
__global__ __launch_bounds__(256) void reduce_rows_staged(const float *__restrict__ in, float *__restrict__ out,
                                                          size_t rows_total, unsigned len, unsigned R, unsigned magic,
                                                          float mean_div, int prod_quirk,
                                                          const float *__restrict__ first = nullptr, size_t first_axis = 0) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const unsigned pitch = len | 1u;
    const size_t row0 = (size_t)blockIdx.x * R;
    const unsigned rows = (unsigned)(rows_total - row0 < R ? rows_total - row0 : R);
    const unsigned total = rows * len;
    const float *src = in + row0 * len;
    const unsigned nvec = total / 4;
    for (unsigned v = threadIdx.x; v < nvec; v += 256) {
        const v4f a = __builtin_nontemporal_load((const v4f *)(src + (size_t)v * 4));
        const unsigned e = v * 4;
        unsigned r = __umulhi(e, magic);   // e / len (magic = ceil(2^32 / len), exact for e < 2^16)
        unsigned c = e - r * len;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            slab[r * pitch + c] = a[k];
            if (++c == len) { c = 0; ++r; }
        }
    }
    for (unsigned e = nvec * 4 + threadIdx.x; e < total; e += 256) {
        const unsigned r = __umulhi(e, magic);
        slab[r * pitch + (e - r * len)] = src[e];
    }
    __syncthreads();
    for (unsigned r = threadIdx.x; r < rows; r += 256) {
        const float *p = slab + r * pitch;
        float a0 = r_identity<OP>(), a1 = a0;
        unsigned c = 0;
        for (; c + 1 < len; c += 2) {
            a0 = r_combine<OP>(a0, p[c]);
            a1 = r_combine<OP>(a1, p[c + 1]);
        }
        if (c < len) a0 = r_combine<OP>(a0, p[c]);
        float v = r_combine<OP>(a0, a1);
        if constexpr (OP == NP_MEAN) v = __fdiv_rn(v, mean_div);
        if constexpr (OP == NP_PROD) {
            if (prod_quirk && v == 0.0f) v = 0.0f;   // see reduce_rows_wave
        }
        out[row0 + r] = r_first_nan<OP>(v, first ? first + (row0 + r) * first_axis : nullptr);
    }
}

// blockIdx.y = chunk of the row (chunks > 1: few rows, long rows — out[row][chunk], a later pass
// folds the chunks; the MEAN division then happens there).
template <int OP, typename I>
__global__ __launch_bounds__(256) void reduce_rows_block(const float *__restrict__ in,
                                                         float *__restrict__ out, I rows, I row_len,
                                                         float mean_div, I chunk_len, int prod_quirk,
                                                         const float *__restrict__ first = nullptr, I first_axis = 0) {
    __shared__ float lds4[4];
    const I row = blockIdx.x, chunk = blockIdx.y;
    const I c0 = chunk * chunk_len;
    const I len = (row_len - c0 < chunk_len) ? row_len - c0 : chunk_len;
    const float *p = in + (size_t)row * row_len + c0;
    const float id = r_identity<OP>();
    float r = id;
    I head = (I)(((16 - ((uintptr_t)p & 15u)) & 15u) / 4);
    if (head > len) head = len;
    if ((I)threadIdx.x < head) r = p[threadIdx.x];
    const I nvec = (len - head) / 4;
    v4f acc0{id, id, id, id}, acc1 = acc0;
    I v = threadIdx.x;
    for (; v + 256 < nvec; v += 512) {
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(p + head + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f *)(p + head + (size_t)(v + 256) * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc0[k] = r_combine<OP>(acc0[k], x0[k]);
            acc1[k] = r_combine<OP>(acc1[k], x1[k]);
        }
    }
    for (; v < nvec; v += 256) {
        const v4f x0 = *(const v4f *)(p + head + (size_t)v * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc0[k] = r_combine<OP>(acc0[k], x0[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r = r_combine<OP>(r, r_combine<OP>(acc0[k], acc1[k]));
    const I t = head + nvec * 4 + threadIdx.x;
    if (t < len) r = r_combine<OP>(r, p[t]);
    r = block_reduce<OP>(r, lds4);
    if (threadIdx.x == 0) {
        if constexpr (OP == NP_MEAN) r = __fdiv_rn(r, mean_div);
        if constexpr (OP == NP_PROD) {
            if (prod_quirk && r == 0.0f) r = 0.0f;   // see reduce_rows_wave
        }
        out[(size_t)row * gridDim.y + chunk] = r_first_nan<OP>(r, first ? first + (size_t)row * first_axis : nullptr);   // (chunked launches pass none)
    }
}

// how many chunks to cut the axis into so that the column reduce has >= ~8 workgroups per CU
size_t choose_splits(size_t outer, size_t axis_len, size_t inner4) {
    const size_t col_tiles = (inner4 + 63) / 64;
    const size_t base = col_tiles * outer;
    // 12 workgroups per CU (tuning: np::stream_cap() x 3/2), and an ODD number of rows per chunk: chunks that start a
    // power-of-two number of rows apart (65536 x 4096 in 128 chunks: 512 rows = 8 MiB) put every workgroup's
    // current row on the same HBM channels — 6.19 TB/s against 6.45-6.50 (profiles/r02/reduce_cap_ab_2.log)
    const size_t target = np::stream_cap() * 3 / 2;
    if (base >= target) return 1;
    size_t s = (target + base - 1) / base;
    // keep at least 64 rows per chunk so the per-workgroup epilogue stays negligible
    const size_t max_s = axis_len / 64 > 0 ? axis_len / 64 : 1;
    if (s > max_s) s = max_s;
    if (s > 65535) s = 65535;
    if (s < 1) s = 1;
    // the kernels derive rows per chunk as ceil(axis_len / splits): step to the nearest split count that makes it odd
    for (size_t t = s; t > 1 && t + 16 > s; --t)
        if (((axis_len + t - 1) / t) % 2 == 1) return t;
    return s;
}

// mean_div_override != 0: this call folds the partials of an earlier pass — MEAN divides by the
// original axis length, not by the number of partials, and the NaN rule of MIN / MAX looks at position 0 of the ORIGINAL
// array's slices (first0, an array of outer x first_axis0 x inner), which the kernel that writes `out` is handed.
template <int OP, typename I>
int launch_reduce_axis(const float *in, size_t outer, size_t axis_len, size_t inner, float *out,
                       unsigned flags, float mean_div_override = 0.0f, const float *first0 = nullptr, size_t first_axis0 = 0) {
    hipStream_t s = np::stream();
    const float *first = first0 ? first0 : in;
    const size_t first_axis = first0 ? first_axis0 : axis_len;
    const float mean_div = mean_div_override != 0.0f ? mean_div_override
                                                      : (float)(long)axis_len;   // CreateFromLongScalar, numpower.c:2666
    const int quirk = (OP == NP_PROD && (flags & NP_QUIRK_AVX_BODY) && axis_len > 1) ? 1 : 0;
    const size_t body_end = np_avx_body_end(inner);
    constexpr int P1 = (OP == NP_MEAN) ? NP_SUM : OP;   // what a non-final pass computes
    const size_t target_wg = (size_t)np::num_cus() * 8;

    if (inner == 1) {
        // contiguous rows
        if (axis_len >= 4096) {
            if (outer > 0x7fffffffu)
                return np::fail(NP_ERR_INVALID, "np_reduce_axis: too many rows for row reduce");
            // few long rows (a (3, 30M) array, a column vector): cut each row into chunks so that
            // the grid still fills the chip, then fold the chunks
            size_t chunks = 1;
            if (outer < target_wg) {
                chunks = (target_wg + outer - 1) / outer;
                const size_t max_chunks = axis_len / 2048;
                if (chunks > max_chunks) chunks = max_chunks;
                if (chunks > 65535) chunks = 65535;
                if (chunks < 1) chunks = 1;
            }
            if (chunks == 1) {
                reduce_rows_block<OP, I><<<(unsigned)outer, 256, 0, s>>>(in, out, (I)outer, (I)axis_len,
                                                                      mean_div, (I)axis_len, quirk, first, (I)first_axis);
                NP_LAUNCH_CHECK("reduce_rows_block");
                g_last_path |= NP_REDUCE_PATH_ROWS_BLOCK;
                return NP_OK;
            }
            const size_t chunk_len = ((axis_len + chunks - 1) / chunks + 3) / 4 * 4;
            chunks = (axis_len + chunk_len - 1) / chunk_len;
            np::Scratch partials;
            if (int rc = partials.alloc(outer * chunks * sizeof(float))) return rc;
            reduce_rows_block<P1, I><<<dim3((unsigned)outer, (unsigned)chunks), 256, 0, s>>>(
                in, (float *)partials.ptr, (I)outer, (I)axis_len, 1.0f, (I)chunk_len, 0);
            NP_LAUNCH_CHECK("reduce_rows_block(chunks)");
            g_last_path |= NP_REDUCE_PATH_ROWS_BLOCK_CHUNKED;
            return launch_reduce_axis<OP, I>((const float *)partials.ptr, outer, chunks, 1, out, flags, mean_div, first, first_axis);
        }
        if (axis_len > 4 && axis_len <= 48 && outer * axis_len >= (size_t(8) << 20) && ((uintptr_t)in & 15u) == 0) {
            // slabs of R rows (a multiple of 256) staged through ~32 KB of LDS: 10^7 x 10 4.5 -> 5.95 TB/s, 5 * 10^6 x 16
            // 2.4 -> 6.4, 2 * 10^7 x 5 3.8 -> 5.35 (tools/short_rows_reduce_ab.py); rows of 63 floats lose (two slabs per CU)
            // and so do small arrays (300001 x 7: 3.5 -> 4.2 us), which stay with the lane-group kernel below
            const unsigned pitch = (unsigned)axis_len | 1u;
            unsigned R = (8192u / pitch) / 256u * 256u;
            if (R < 256) R = 256;
            const size_t blocks = (outer + R - 1) / R;
            const size_t lds = (size_t)R * pitch * sizeof(float);
            if (blocks <= 0x7fffffffu && lds <= 64 * 1024) {
                const unsigned magic = (unsigned)((0x100000000ull + axis_len - 1) / axis_len);
                reduce_rows_staged<OP><<<(unsigned)blocks, 256, lds, s>>>(in, out, outer, (unsigned)axis_len, R, magic,
                                                                       mean_div, quirk, first, first_axis);
                NP_LAUNCH_CHECK("reduce_rows_staged");
                g_last_path |= NP_REDUCE_PATH_ROWS_STAGED;
                return NP_OK;
            }
        }
        if (axis_len > 4 && axis_len <= 256) {
            // L lanes per row with at most ~8 elements per lane
            size_t L = 2;
            while (L * 8 < axis_len) L *= 2;
            const size_t rows_per_block = 256 / L;
            const size_t blocks = (outer + rows_per_block - 1) / rows_per_block;
            if (blocks > 0x7fffffffu)
                return np::fail(NP_ERR_INVALID, "np_reduce_axis: too many rows for row reduce");
#define NP_RG(L_) reduce_rows_group<OP, L_, I><<<(unsigned)blocks, 256, 0, s>>>(in, out, (I)outer, (I)axis_len, mean_div, quirk, first, (I)first_axis)
            switch (L) {
                case 2: NP_RG(2); break;
                case 4: NP_RG(4); break;
                case 8: NP_RG(8); break;
                case 16: NP_RG(16); break;
                default: NP_RG(32); break;
            }
#undef NP_RG
            NP_LAUNCH_CHECK("reduce_rows_group");
            g_last_path |= NP_REDUCE_PATH_ROWS_GROUP;
            return NP_OK;
        }
        if (axis_len >= 32) {
            const size_t blocks = (outer + 3) / 4;
            if (blocks > 0x7fffffffu)
                return np::fail(NP_ERR_INVALID, "np_reduce_axis: too many rows for row reduce");
            reduce_rows_wave<OP, I><<<(unsigned)blocks, 256, 0, s>>>(in, out, (I)outer, (I)axis_len,
                                                                  mean_div, quirk, first, (I)first_axis);
            NP_LAUNCH_CHECK("reduce_rows_wave");
            g_last_path |= NP_REDUCE_PATH_ROWS_WAVE;
            return NP_OK;
        }
    } else if ((inner % 4 == 0 || inner >= 4000) && outer <= 65535 &&
               !(inner <= 128 && axis_len >= 512 && outer * inner < target_wg * 64)) {
        // (a handful of float4 columns would use a fraction of the 64-column tile: those go to the
        // flat small-inner kernel below; any pointer alignment.  Ragged rows (inner % 4 != 0: every row starts
        // on a different 4-byte boundary) come here from 4000 columns up — 10007 x 10007 axis-0 sum 4.4 -> 5.4
        // TB/s, 5000 x 20001 4.55 -> 5.58, 25000 x 4001 4.8 -> 5.15; at 2502 columns it is a tie with the
        // generic kernel and at 1001 it loses 12 %: tools/ragged_reduce_ab.py)
        const size_t inner4 = (inner + 3) / 4;
        const size_t splits = choose_splits(outer, axis_len, inner4);
        const dim3 grid((unsigned)((inner4 + 63) / 64), (unsigned)splits, (unsigned)outer);
        // tiles that straddle 128-byte lines: neighbours on one XCD (np_reduce_set_variant(4200001): the launch order, A/B)
        const unsigned xcd_runs = ((inner * sizeof(float)) % 128 != 0 || ((uintptr_t)in & 127u) != 0) && grid.x > 1 &&
                                  (size_t)grid.x * grid.y * grid.z < (size_t(1) << 31) && !np::g_xcd_runs_off ? 1u : 0u;
        if (xcd_runs) g_last_path |= NP_REDUCE_PATH_COLS_XCD_RUNS;
        if (splits == 1) {
            reduce_axis_cols<OP, true, I><<<grid, 256, 0, s>>>(in, out, (I)axis_len, (I)inner, (I)1,
                                                            mean_div, quirk, (I)body_end, xcd_runs, first, (I)first_axis);
            NP_LAUNCH_CHECK("reduce_axis_cols");
            g_last_path |= NP_REDUCE_PATH_COLS_ONE_PASS;
            return NP_OK;
        }
        np::Scratch partials;
        if (int rc = partials.alloc(outer * splits * inner * sizeof(float))) return rc;
        reduce_axis_cols<OP, false, I><<<grid, 256, 0, s>>>(in, (float *)partials.ptr, (I)axis_len,
                                                         (I)inner, (I)splits, mean_div, 0, (I)0, xcd_runs);
        NP_LAUNCH_CHECK("reduce_axis_cols(pass 1)");
        // Many chunks over few column tiles (a tall, skinny array: 500000 x 200 is ONE tile in 3072 chunks): the pass below would
        // fold them with one workgroup per tile, four rows in flight per wave — 192 dependent iterations, as long as the first
        // pass itself (134 us where the read takes 67).  The partials are again a tall skinny array: reduce THEM in chunks first
        // (one more 4 us launch).  From 256 chunks up; BASELINE config 4 (192 chunks over 16 tiles, a 5 us fold) is not touched.
        if (splits >= 256) {
            g_last_path |= NP_REDUCE_PATH_COLS_SPLITS_RECURSE;
            return launch_reduce_axis<OP, I>((const float *)partials.ptr, outer, splits, inner, out, flags, mean_div, first, first_axis);
        }
        g_last_path |= NP_REDUCE_PATH_COLS_TWO_PASSES;
        // pass 2: the partials are an outer x splits x inner array; MEAN must divide by the real
        // axis length, not by `splits`.
        const dim3 grid2((unsigned)((inner4 + 63) / 64), 1, (unsigned)outer);
        reduce_axis_cols<OP, true, I><<<grid2, 256, 0, s>>>((const float *)partials.ptr, out,
                                                         (I)splits, (I)inner, (I)1, mean_div,
                                                         quirk, (I)body_end, 0u, first, (I)first_axis);
        NP_LAUNCH_CHECK("reduce_axis_cols(pass 2)");
        return NP_OK;
    } else if (inner <= 128 && axis_len >= 512 && outer <= 65535 && outer * inner < target_wg * 64) {
        // a handful of columns, many rows: flat coalesced slabs, then fold the per-slab partials
        size_t blocks = target_wg / outer;
        const size_t max_blocks = axis_len / 256;
        if (blocks > max_blocks) blocks = max_blocks;
        if (blocks < 1) blocks = 1;
        size_t rows_per_block = (axis_len + blocks - 1) / blocks;
        // slabs that start on 16-byte boundaries: the float4 walk (np_reduce_set_variant(4300001): the dword walk, A/B)
        const bool v4 = !g_small_inner_dword && ((uintptr_t)in & 15u) == 0 && (outer == 1 || (axis_len * inner) % 4 == 0);
        if (v4) rows_per_block = (rows_per_block + 3) / 4 * 4;
        blocks = (axis_len + rows_per_block - 1) / rows_per_block;
        np::Scratch partials;
        if (int rc = partials.alloc(outer * blocks * inner * sizeof(float))) return rc;
        if (v4)
            reduce_small_inner_v4<P1, I><<<dim3((unsigned)blocks, (unsigned)outer), 256, 0, s>>>(
                in, (float *)partials.ptr, (I)axis_len, (I)inner, (I)rows_per_block);
        else
            reduce_small_inner<P1, I><<<dim3((unsigned)blocks, (unsigned)outer), 256, 0, s>>>(
                in, (float *)partials.ptr, (I)axis_len, (I)inner, (I)rows_per_block);
        NP_LAUNCH_CHECK("reduce_small_inner");
        g_last_path |= v4 ? NP_REDUCE_PATH_SMALL_INNER_V4 : NP_REDUCE_PATH_SMALL_INNER;
        return launch_reduce_axis<OP, I>((const float *)partials.ptr, outer, blocks, inner, out, flags, mean_div, first, first_axis);
    }
    // generic fallback (ragged inner, misaligned views, tiny problems): one thread per output and
    // axis chunk; chunk the axis when the outputs alone cannot fill the machine
    const size_t outputs = outer * inner;
    const size_t target_threads = (size_t)np::num_cus() * 2048;
    size_t chunks = 1;
    if (outputs < target_threads && axis_len >= 128) {
        chunks = (target_threads + outputs - 1) / outputs;
        const size_t max_chunks = axis_len / 32;
        if (chunks > max_chunks) chunks = max_chunks;
        if (chunks < 1) chunks = 1;
    }
    const size_t chunk_len = (axis_len + chunks - 1) / chunks;
    chunks = chunk_len ? (axis_len + chunk_len - 1) / chunk_len : 1;
    if (chunks < 1) chunks = 1;
    const size_t total = outputs * chunks;
    size_t blocks = (total + 255) / 256;
    const size_t cap = (size_t)np::num_cus() * 16;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (chunks == 1) {
        reduce_axis_generic<OP, I><<<(unsigned)blocks, 256, 0, s>>>(in, out, (I)outer, (I)axis_len,
                                                                 (I)inner, mean_div, quirk,
                                                                 (I)body_end, (I)1, (I)axis_len, first, (I)first_axis);
        NP_LAUNCH_CHECK("reduce_axis_generic");
        g_last_path |= NP_REDUCE_PATH_GENERIC;
        return NP_OK;
    }
    np::Scratch partials;
    if (int rc = partials.alloc(total * sizeof(float))) return rc;
    reduce_axis_generic<P1, I><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)partials.ptr, (I)outer,
                                                             (I)axis_len, (I)inner, 1.0f, 0, (I)0,
                                                             (I)chunks, (I)chunk_len);
    NP_LAUNCH_CHECK("reduce_axis_generic(chunks)");
    g_last_path |= NP_REDUCE_PATH_GENERIC_CHUNKED;
    return launch_reduce_axis<OP, I>((const float *)partials.ptr, outer, chunks, inner, out, flags, mean_div, first, first_axis);
}

template <int OP>
int dispatch_reduce_axis(const float *in, size_t outer, size_t axis_len, size_t inner, float *out,
                         unsigned flags) {
    const size_t n = outer * axis_len * inner;
    if (n < (size_t(1) << 31))
        return launch_reduce_axis<OP, uint32_t>(in, outer, axis_len, inner, out, flags);
    return launch_reduce_axis<OP, uint64_t>(in, outer, axis_len, inner, out, flags);
}

}  // namespace

extern "C" {

int np_reduce_all_dev(int op, const float *in, size_t n, float *dev_out) {
    if (op < 0 || op >= NP_REDUCE_OP_COUNT)
        return np::fail(NP_ERR_INVALID, "np_reduce_all: unknown op %d", op);
    if (!dev_out) return np::fail(NP_ERR_INVALID, "np_reduce_all: null output");
    if (n > 0 && !in) return np::fail(NP_ERR_INVALID, "np_reduce_all: null input");
    if (int rc = np::ensure_init()) return rc;
    g_last_path = 0;
    switch (op) {
        case NP_SUM: return dispatch_reduce_all<NP_SUM>(in, n, dev_out);
        case NP_PROD: return dispatch_reduce_all<NP_PROD>(in, n, dev_out);
        case NP_MIN: return dispatch_reduce_all<NP_MIN>(in, n, dev_out);
        case NP_MAX: return dispatch_reduce_all<NP_MAX>(in, n, dev_out);
        default: return dispatch_reduce_all<NP_MEAN>(in, n, dev_out);
    }
}

int np_reduce_all(int op, const float *in, size_t n, float *host_out) {
    if (!host_out) return np::fail(NP_ERR_INVALID, "np_reduce_all: null output");
    if (int rc = np::ensure_init()) return rc;
    np::ResultCall call;
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    if (int rc = np_reduce_all_dev(op, in, n, slot)) return rc;
    if (int rc = call.wait()) return rc;
    *host_out = slot[0];
    return NP_OK;
}

size_t np_reduce_axis_workspace(size_t outer, size_t axis_len, size_t inner) {
    if (inner <= 1 || inner % 4 != 0 || outer > 65535) return 0;
    if (np::ensure_init()) return 0;
    const size_t splits = choose_splits(outer, axis_len, inner / 4);
    return splits > 1 ? outer * splits * inner * sizeof(float) : 0;
}

int np_reduce_axis(int op, const float *in, size_t outer, size_t axis_len, size_t inner,
                   float *out, unsigned flags) {
    if (op < 0 || op >= NP_REDUCE_OP_COUNT)
        return np::fail(NP_ERR_INVALID, "np_reduce_axis: unknown op %d", op);
    if (outer == 0 || inner == 0) return NP_OK;
    if (axis_len == 0) return np::fail(NP_ERR_INVALID, "np_reduce_axis: empty axis");
    if (!in || !out) return np::fail(NP_ERR_INVALID, "np_reduce_axis: null pointer");
    if (int rc = np::ensure_init()) return rc;
    g_last_path = 0;
    switch (op) {
        case NP_SUM: return dispatch_reduce_axis<NP_SUM>(in, outer, axis_len, inner, out, flags);
        case NP_PROD: return dispatch_reduce_axis<NP_PROD>(in, outer, axis_len, inner, out, flags);
        case NP_MIN: return dispatch_reduce_axis<NP_MIN>(in, outer, axis_len, inner, out, flags);
        case NP_MAX: return dispatch_reduce_axis<NP_MAX>(in, outer, axis_len, inner, out, flags);
        default: return dispatch_reduce_axis<NP_MEAN>(in, outer, axis_len, inner, out, flags);
    }
}

int np_reduce_set_variant(int variant) {
    if (variant >= 2000000 && variant < 2100000) {   // the largest first-pass grid that folds its partials in-kernel
        np::g_fold_in_kernel_max = (size_t)(variant - 2000000);
        return NP_OK;
    }
    if (variant == 4300000 || variant == 4300001) {   // column sums over a few columns: float4 walk (0) or dword walk (1)
        g_small_inner_dword = variant - 4300000;
        return NP_OK;
    }
    if (variant == 4200000 || variant == 4200001) {   // column sums and argmax / argmin over wide unaligned rows: tiles dealt to the XCDs in runs (0) or in launch order (1)
        np::g_xcd_runs_off = variant - 4200000;
        return NP_OK;
    }
    if (variant >= 4100000 && variant < 4100100) {   // argmax / argmin over a few columns (flat walks): workgroups per CU
        np::g_arg_flat_wg_per_cu = variant - 4100000;   // 0 = the default rule
        return NP_OK;
    }
    if (variant >= 4000000 && variant < 4000100) {   // argmax / argmin over wide inner: workgroups per CU
        np::g_arg_cols_wg_per_cu = variant - 4000000;   // 0 = the default rule
        return NP_OK;
    }
    if (variant >= 3000000 && variant < 3100000) {   // np_reduce_all of <= 4 M elements on at most N workgroups (0 = off)
        np::g_small_reduce_blocks = (size_t)(variant - 3000000);
        return NP_OK;
    }
    if (variant < 0 || variant > 1000000) return np::fail(NP_ERR_INVALID, "np_reduce_set_variant: workgroups per CU out of range");
    np::g_wg_per_cu = variant;
    return NP_OK;
}

int np_debug_reduce_last_path(unsigned *host_mask) {
    if (!host_mask) return np::fail(NP_ERR_INVALID, "np_debug_reduce_last_path: null pointer");
    *host_mask = g_last_path;
    return NP_OK;
}

}  // extern "C"
