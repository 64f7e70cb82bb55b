// argmax / argmin of libnp_hip.so (np_argreduce): index-carrying reductions along one axis of a contiguous array viewed as
// outer x axis_len x inner.  Helpers, the streaming kernels, the kernels that fold their (value, index) partials,
// launch_arg_fold and the entry point with its planner, in that order.  Value reductions: np_reduce.hip.
#include <float.h>
#include <math.h>
#include <string.h>

#include "np_internal.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// argmax / argmin (src/ndmath/calculation.c:9-72): index-carrying reductions
// ------------------------------------------------------------------------------------------
//
// float_argmax: first index of the maximum; a NaN in element 0 wins outright, later NaNs are never
// selected (`*ip > mp` is false for NaN).  float_argmin: `!(mp <= *ip)` — the first NaN anywhere
// wins (and stops the scan), otherwise the first index of the minimum.  `better(a, b)` below says
// whether candidate a must replace b when a comes from a LATER index range (ties keep the earlier).
struct ArgPair {
    float v;
    unsigned i;   // index along the reduced axis
};

template <bool IS_MAX>
__device__ __forceinline__ float arg_key(float x, unsigned index) {
    if constexpr (IS_MAX) {
        // NaN at position 0 is maximal; NaN elsewhere can never win
        if (x != x) return (index == 0) ? INFINITY : -INFINITY;
        return x;
    }
    return x;
}

// true if (vb, ib) should replace (va, ia); both are valid candidates
template <bool IS_MAX>
__device__ __forceinline__ bool arg_replace(float va, unsigned ia, float vb, unsigned ib) {
    if constexpr (IS_MAX) {
        if (vb > va) return true;
        return (vb == va) && (ib < ia);
    } else {
        const bool na = va != va, nb = vb != vb;
        if (na || nb) {
            if (na && nb) return ib < ia;
            return nb;               // a NaN beats every number (first NaN wins)
        }
        if (vb < va) return true;
        return (vb == va) && (ib < ia);
    }
}

template <bool IS_MAX>
__device__ __forceinline__ ArgPair arg_combine(ArgPair a, ArgPair b) {
    return arg_replace<IS_MAX>(a.v, a.i, b.v, b.i) ? b : a;
}

// ---- the streaming forms (round 5) ----------------------------------------------------------------------------------
// An ACCUMULATOR (one float4 component of one of the loads a lane keeps in flight) meets its elements in increasing index
// order, so "the first occurrence wins" is a strict compare and an update is three VALU ops — compare, select the value,
// select the trip counter (shared by the four components of a load: no per-element index arithmetic).  The general
// (value, index) combine with its tie and NaN rules runs once per accumulator at the end.  NaN rules inside the loop:
// argmax — a NaN never wins (`x > best` is false), which is its key -inf of arg_key(); a NaN in position 0 of the axis is
// maximal and is patched in by whoever owns position 0.  argmin — the first NaN wins and then stays.
constexpr unsigned kArgNone = 0xffffffffu;

template <bool IS_MAX>
__device__ __forceinline__ void arg_take(float &bv, unsigned &bt, float x, unsigned t) {
    bool r;
    if constexpr (IS_MAX) r = x > bv;
    else r = !(bv <= x) && (bv == bv);
    bv = r ? x : bv;
    bt = r ? t : bt;
}

// what a single element is worth to the general combine when its position is not 0 (position 0: the caller)
template <bool IS_MAX>
__device__ __forceinline__ float arg_key_later(float x) {
    if constexpr (IS_MAX) return (x != x) ? -INFINITY : x;
    return x;
}

typedef v4f arg_v4f_u __attribute__((aligned(4)));   // a dwordx4 load from any dword-aligned address
#define ARG_LOAD4(ptr) __builtin_nontemporal_load((const arg_v4f_u *)(ptr))

// `count` contiguous elements at q, element e has index base + e along the reduced axis; the STRIDE threads of the caller
// (a wave, or every thread of the workgroups that share a row: grid-stride, as reduce_all_pass1 walks; tid < STRIDE) share them.  Returns this thread's best (value, index), {identity, kArgNone} if it
// met nothing.  Aligned float4 loads behind a scalar head, four loads in flight per lane.
template <bool IS_MAX>
__device__ __forceinline__ ArgPair arg_scan_contig(const float *__restrict__ q, unsigned count, unsigned base, unsigned tid,
                                                   const unsigned STRIDE) {
    const float id = IS_MAX ? -INFINITY : INFINITY;
    unsigned head = (unsigned)(((16u - ((uintptr_t)q & 15u)) & 15u) >> 2);
    if (head > count) head = count;
    const float *qa = q + head;
    const unsigned nvec = (count - head) >> 2;
    float bv[4][4];
    unsigned bt[4][4];
    const bool main_runs = tid + 3 * STRIDE < nvec;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bv[s2][k] = id;
            bt[s2][k] = s2 == 0 ? (tid < nvec ? tid : kArgNone) : (main_runs ? tid + s2 * STRIDE : kArgNone);
        }
    unsigned v = tid;
    for (; v + 3 * STRIDE < nvec; v += 4 * STRIDE) {
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)(v + STRIDE) * 4));
        const v4f x2 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)(v + 2 * STRIDE) * 4));
        const v4f x3 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)(v + 3 * STRIDE) * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            arg_take<IS_MAX>(bv[0][k], bt[0][k], x0[k], v);
            arg_take<IS_MAX>(bv[1][k], bt[1][k], x1[k], v + STRIDE);
            arg_take<IS_MAX>(bv[2][k], bt[2][k], x2[k], v + 2 * STRIDE);
            arg_take<IS_MAX>(bv[3][k], bt[3][k], x3[k], v + 3 * STRIDE);
        }
    }
    if (v < nvec) {   // at most three vectors are left per lane: issued together, into the accumulators whose turn it would have been
        const unsigned v1 = v + STRIDE, v2 = v + 2 * STRIDE;
        const bool h1 = v1 < nvec, h2 = v2 < nvec;
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)v * 4));
        v4f x1{id, id, id, id}, x2 = x1;
        if (h1) x1 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)v1 * 4));
        if (h2) x2 = __builtin_nontemporal_load((const v4f *)(qa + (size_t)v2 * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!main_runs) {   // accumulators 1 and 2 meet their first element here: it is a candidate even if it equals the identity
                if (h1) bt[1][k] = v1;
                if (h2) bt[2][k] = v2;
            }
            arg_take<IS_MAX>(bv[0][k], bt[0][k], x0[k], v);
            if (h1) arg_take<IS_MAX>(bv[1][k], bt[1][k], x1[k], v1);
            if (h2) arg_take<IS_MAX>(bv[2][k], bt[2][k], x2[k], v2);
        }
    }
    ArgPair best{id, kArgNone};
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const ArgPair c{bv[s2][k], bt[s2][k] == kArgNone ? kArgNone : base + head + 4u * bt[s2][k] + (unsigned)k};
            best = arg_combine<IS_MAX>(best, c);
        }
    if (tid < head) best = arg_combine<IS_MAX>(best, ArgPair{arg_key_later<IS_MAX>(q[tid]), base + tid});
    const unsigned t = head + 4u * nvec + tid;
    if (t < count) best = arg_combine<IS_MAX>(best, ArgPair{arg_key_later<IS_MAX>(q[t]), base + t});
    return best;
}

template <bool IS_MAX>
__device__ __forceinline__ ArgPair arg_wave_reduce(ArgPair best) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ArgPair o;
        o.v = __shfl_down(best.v, off, 64);
        o.i = __shfl_down(best.i, off, 64);
        best = arg_combine<IS_MAX>(best, o);   // a lane without a candidate holds {identity, kArgNone}: it loses every tie
    }
    return best;
}

// `chunks` workgroups per contiguous row (inner == 1) walk it together, grid-stride; partial index = row*chunks+chunk.
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_rows_kernel(const float *__restrict__ in, float *__restrict__ pv,
                                                             unsigned *__restrict__ pi, unsigned len,
                                                             unsigned chunks) {
    __shared__ float sv[4];
    __shared__ unsigned si[4];
    const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const float *p = in + (size_t)row * len;
    ArgPair best = arg_scan_contig<IS_MAX>(p, len, 0u, chunk * 256u + threadIdx.x, chunks * 256u);
    best = arg_wave_reduce<IS_MAX>(best);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sv[wave] = best.v;
        si[wave] = best.i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ArgPair r{sv[0], si[0]};
        for (int w = 1; w < 4; ++w) r = arg_combine<IS_MAX>(r, ArgPair{sv[w], si[w]});
        if (IS_MAX && chunk == 0 && p[0] != p[0]) r = ArgPair{INFINITY, 0u};   // a NaN in position 0 is maximal
        pv[blockIdx.x] = r.v;
        pi[blockIdx.x] = r.i;
    }
}

// One WAVE per contiguous row (rows of a few hundred to a few thousand elements, many of them): every load of the row in
// flight at once, folded with shuffles, no LDS, no partials, no second launch.
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_rows_wave(const float *__restrict__ in, float *__restrict__ out,
                                                           size_t rows, unsigned len) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const unsigned lane = threadIdx.x & 63;
    const float *p = in + row * len;
    ArgPair best = arg_scan_contig<IS_MAX>(p, len, 0u, lane, 64u);
    best = arg_wave_reduce<IS_MAX>(best);
    if (lane == 0) {
        if (IS_MAX && p[0] != p[0]) best = ArgPair{INFINITY, 0u};
        out[row] = (float)best.i;
    }
}

// generic with the axis cut into chunks: one thread per (output, chunk), coalesced across the inner
// index; writes (value, index) partials [outer][chunks][inner] for argreduce_fold_kernel
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_chunks_kernel(const float *__restrict__ in, float *__restrict__ pv,
                                                               unsigned *__restrict__ pi, size_t outer,
                                                               unsigned axis_len, size_t inner, unsigned chunks,
                                                               unsigned chunk_len) {
    const size_t total = outer * chunks * inner;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const size_t oc = idx / inner, j = idx - oc * inner;
        const size_t o = oc / chunks;
        const unsigned c = (unsigned)(oc - o * chunks);
        const unsigned a0 = c * chunk_len;
        const unsigned a1 = axis_len - a0 < chunk_len ? axis_len : a0 + chunk_len;   // (a0 + chunk_len may wrap on an axis near 2^32)
        const float *p = in + o * axis_len * inner + j;
        ArgPair best{arg_key<IS_MAX>(p[(size_t)a0 * inner], a0), a0};
        // four loads in flight; ties are broken by index, so the combining order does not matter
        unsigned a = a0 + 1;
        for (; a + 3 < a1; a += 4) {
            const float x0 = p[(size_t)a * inner], x1 = p[(size_t)(a + 1) * inner];
            const float x2 = p[(size_t)(a + 2) * inner], x3 = p[(size_t)(a + 3) * inner];
            const ArgPair q0{arg_key<IS_MAX>(x0, a), a}, q1{arg_key<IS_MAX>(x1, a + 1), a + 1};
            const ArgPair q2{arg_key<IS_MAX>(x2, a + 2), a + 2}, q3{arg_key<IS_MAX>(x3, a + 3), a + 3};
            best = arg_combine<IS_MAX>(best, arg_combine<IS_MAX>(arg_combine<IS_MAX>(q0, q1), arg_combine<IS_MAX>(q2, q3)));
        }
        for (; a < a1; ++a) {
            const ArgPair q{arg_key<IS_MAX>(p[(size_t)a * inner], a), a};
            best = arg_combine<IS_MAX>(best, q);
        }
        pv[idx] = best.v;
        pi[idx] = best.i;
    }
}

// generic: one thread per output element, sequential over the axis exactly like the reference loop
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_generic_kernel(const float *__restrict__ in,
                                                                float *__restrict__ out, size_t outer,
                                                                unsigned axis_len, size_t inner) {
    const size_t total = outer * inner;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const size_t o = idx / inner, j = idx % inner;
        const float *p = in + o * axis_len * inner + j;
        ArgPair best{arg_key<IS_MAX>(p[0], 0), 0};
        unsigned a = 1;
        for (; a + 3 < axis_len; a += 4) {   // four loads in flight (index tie-break: order-independent)
            const float x0 = p[(size_t)a * inner], x1 = p[(size_t)(a + 1) * inner];
            const float x2 = p[(size_t)(a + 2) * inner], x3 = p[(size_t)(a + 3) * inner];
            const ArgPair q0{arg_key<IS_MAX>(x0, a), a}, q1{arg_key<IS_MAX>(x1, a + 1), a + 1};
            const ArgPair q2{arg_key<IS_MAX>(x2, a + 2), a + 2}, q3{arg_key<IS_MAX>(x3, a + 3), a + 3};
            best = arg_combine<IS_MAX>(best, arg_combine<IS_MAX>(arg_combine<IS_MAX>(q0, q1), arg_combine<IS_MAX>(q2, q3)));
        }
        for (; a < axis_len; ++a) {
            const ArgPair c{arg_key<IS_MAX>(p[(size_t)a * inner], a), a};
            best = arg_combine<IS_MAX>(best, c);
        }
        out[idx] = (float)best.i;
    }
}

// argmax / argmin with a handful of columns and many rows (inner <= 64): slabs of rows read as FLAT memory with float4
// loads.  T = the largest multiple of `inner` threads that fits: a thread's vector v = t + j T starts at flat element
// 4 t + 4 j T, and 4 j T is a whole number of rows — so component k of thread t stays in column (4 t + k) % inner for the whole
// walk and its row advances by 4 T / inner per trip: four accumulators per load, each with a fixed column, the trip counter j
// as their index.  Four loads in flight.  Partials [outer][blocks][inner].
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_small_inner(const float *__restrict__ in, float *__restrict__ pv,
                                                             unsigned *__restrict__ pi, unsigned axis_len,
                                                             unsigned inner, unsigned rows_per_block) {
    __shared__ float sv[1024];
    __shared__ unsigned si[1024];
    const float id = IS_MAX ? -INFINITY : INFINITY;
    const unsigned T = (256u / inner) * inner;
    const unsigned o = blockIdx.y, b = blockIdx.x;
    const unsigned r0 = b * rows_per_block;
    const unsigned r1 = axis_len - r0 < rows_per_block ? axis_len : r0 + rows_per_block;   // (r0 + rows_per_block may wrap on an axis near 2^32)
    const unsigned cnt = (r1 - r0) * inner;          // the host keeps rows_per_block * inner below 2^31
    const unsigned nvec = cnt >> 2;
    const float *p = in + ((size_t)o * axis_len + r0) * inner;
    const unsigned t = threadIdx.x;
    if (t < T) {
        float bv[4][4];
        unsigned bj[4][4];
        const bool main_runs = t + 3 * T < nvec;
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bv[s2][k] = id;
                bj[s2][k] = s2 == 0 ? (t < nvec ? 0u : kArgNone) : (main_runs ? (unsigned)s2 : kArgNone);
            }
        unsigned v = t, j = 0;
        for (; v + 3 * T < nvec; v += 4 * T, j += 4) {
            const v4f x0 = ARG_LOAD4(p + (size_t)v * 4), x1 = ARG_LOAD4(p + (size_t)(v + T) * 4);
            const v4f x2 = ARG_LOAD4(p + (size_t)(v + 2 * T) * 4), x3 = ARG_LOAD4(p + (size_t)(v + 3 * T) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                arg_take<IS_MAX>(bv[0][k], bj[0][k], x0[k], j);
                arg_take<IS_MAX>(bv[1][k], bj[1][k], x1[k], j + 1);
                arg_take<IS_MAX>(bv[2][k], bj[2][k], x2[k], j + 2);
                arg_take<IS_MAX>(bv[3][k], bj[3][k], x3[k], j + 3);
            }
        }
        if (v < nvec) {   // at most three vectors are left per lane: issued together (arg_scan_contig does the same)
            const bool h1 = v + T < nvec, h2 = v + 2 * T < nvec;
            const v4f x0 = ARG_LOAD4(p + (size_t)v * 4);
            v4f x1{id, id, id, id}, x2 = x1;
            if (h1) x1 = ARG_LOAD4(p + (size_t)(v + T) * 4);
            if (h2) x2 = ARG_LOAD4(p + (size_t)(v + 2 * T) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!main_runs) {
                    if (h1) bj[1][k] = j + 1;
                    if (h2) bj[2][k] = j + 2;
                }
                arg_take<IS_MAX>(bv[0][k], bj[0][k], x0[k], j);
                if (h1) arg_take<IS_MAX>(bv[1][k], bj[1][k], x1[k], j + 1);
                if (h2) arg_take<IS_MAX>(bv[2][k], bj[2][k], x2[k], j + 2);
            }
        }
        const unsigned rows_per_trip = 4 * T / inner;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned row0 = r0 + (4 * t + k) / inner;
            ArgPair best{id, kArgNone};
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
                best = arg_combine<IS_MAX>(best, ArgPair{bv[s2][k], bj[s2][k] == kArgNone ? kArgNone : row0 + bj[s2][k] * rows_per_trip});
            sv[4 * t + k] = best.v;
            si[4 * t + k] = best.i;
        }
    }
    __syncthreads();
    // entry e' = m * inner + c (m < 4 T / inner) belongs to column c: halve the m range until one entry per column is left
    // (a thread per column walking its 4 T / inner entries was 340 dependent steps for inner = 3: 16 % of the kernel)
    for (unsigned mcur = 4 * T / inner; mcur > 1;) {
        const unsigned half = (mcur + 1) / 2;
        for (unsigned idx = t; idx < (mcur - half) * inner; idx += 256) {
            const unsigned hi = idx + half * inner;
            const ArgPair r = arg_combine<IS_MAX>(ArgPair{sv[idx], si[idx]}, ArgPair{sv[hi], si[hi]});
            sv[idx] = r.v;
            si[idx] = r.i;
        }
        __syncthreads();
        mcur = half;
    }
    if (t < inner) {
        ArgPair r{sv[t], si[t]};
        for (unsigned e = 4 * nvec; e < cnt; ++e)                                                       // the <= 3 leftover elements
            if (e % inner == t) r = arg_combine<IS_MAX>(r, ArgPair{arg_key_later<IS_MAX>(p[e]), r0 + e / inner});
        if (IS_MAX && r0 == 0 && p[t] != p[t]) r = ArgPair{INFINITY, 0u};   // a NaN in position 0 is maximal
        const size_t at = ((size_t)o * gridDim.x + b) * inner + t;
        pv[at] = r.v;
        pi[at] = r.i;
    }
}

// The same walk with a float4 COLUMN GROUP as the element, for inner % 4 == 0 and inner <= 256 (inner4 = inner / 4 groups per
// row): T4 = the largest multiple of inner4 threads; thread t keeps group t % inner4, its row advances by T4 / inner4 per trip.
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_small_inner4(const float *__restrict__ in, float *__restrict__ pv,
                                                              unsigned *__restrict__ pi, unsigned axis_len,
                                                              unsigned inner4, unsigned rows_per_block) {
    __shared__ float sv[1024];
    __shared__ unsigned si[1024];
    const float id = IS_MAX ? -INFINITY : INFINITY;
    const unsigned T = (256u / inner4) * inner4;
    const unsigned o = blockIdx.y, b = blockIdx.x;
    const unsigned r0 = b * rows_per_block;
    const unsigned r1 = axis_len - r0 < rows_per_block ? axis_len : r0 + rows_per_block;   // (r0 + rows_per_block may wrap on an axis near 2^32)
    const unsigned nvec = (r1 - r0) * inner4;
    const float *p = in + ((size_t)o * axis_len + r0) * inner4 * 4;
    const unsigned t = threadIdx.x;
    if (t < T) {
        float bv[4][4];
        unsigned bj[4][4];
        const bool main_runs = t + 3 * T < nvec;
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bv[s2][k] = id;
                bj[s2][k] = s2 == 0 ? (t < nvec ? 0u : kArgNone) : (main_runs ? (unsigned)s2 : kArgNone);
            }
        unsigned v = t, j = 0;
        for (; v + 3 * T < nvec; v += 4 * T, j += 4) {
            const v4f x0 = ARG_LOAD4(p + (size_t)v * 4), x1 = ARG_LOAD4(p + (size_t)(v + T) * 4);
            const v4f x2 = ARG_LOAD4(p + (size_t)(v + 2 * T) * 4), x3 = ARG_LOAD4(p + (size_t)(v + 3 * T) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                arg_take<IS_MAX>(bv[0][k], bj[0][k], x0[k], j);
                arg_take<IS_MAX>(bv[1][k], bj[1][k], x1[k], j + 1);
                arg_take<IS_MAX>(bv[2][k], bj[2][k], x2[k], j + 2);
                arg_take<IS_MAX>(bv[3][k], bj[3][k], x3[k], j + 3);
            }
        }
        if (v < nvec) {   // at most three vectors are left per lane: issued together (arg_scan_contig does the same)
            const bool h1 = v + T < nvec, h2 = v + 2 * T < nvec;
            const v4f x0 = ARG_LOAD4(p + (size_t)v * 4);
            v4f x1{id, id, id, id}, x2 = x1;
            if (h1) x1 = ARG_LOAD4(p + (size_t)(v + T) * 4);
            if (h2) x2 = ARG_LOAD4(p + (size_t)(v + 2 * T) * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!main_runs) {
                    if (h1) bj[1][k] = j + 1;
                    if (h2) bj[2][k] = j + 2;
                }
                arg_take<IS_MAX>(bv[0][k], bj[0][k], x0[k], j);
                if (h1) arg_take<IS_MAX>(bv[1][k], bj[1][k], x1[k], j + 1);
                if (h2) arg_take<IS_MAX>(bv[2][k], bj[2][k], x2[k], j + 2);
            }
        }
        const unsigned rows_per_trip = T / inner4, row0 = r0 + t / inner4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ArgPair best{id, kArgNone};
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
                best = arg_combine<IS_MAX>(best, ArgPair{bv[s2][k], bj[s2][k] == kArgNone ? kArgNone : row0 + bj[s2][k] * rows_per_trip});
            sv[4 * t + k] = best.v;
            si[4 * t + k] = best.i;
        }
    }
    __syncthreads();
    if (t < 4 * inner4) {                              // one thread per column: group t / 4, component t % 4
        ArgPair r{id, kArgNone};
        for (unsigned e = t; e < 4 * T; e += 4 * inner4) r = arg_combine<IS_MAX>(r, ArgPair{sv[e], si[e]});
        if (IS_MAX && r0 == 0 && p[t] != p[t]) r = ArgPair{INFINITY, 0u};
        const size_t at = ((size_t)o * gridDim.x + b) * (4 * inner4) + t;
        pv[at] = r.v;
        pi[at] = r.i;
    }
}

// Wide inner (>= 192 columns or so): a workgroup owns 64 float4 column groups and one chunk of the axis; its four waves walk
// interleaved rows (a wave-level load is one contiguous 1 KiB piece of a row), four rows in flight per lane, and meet in LDS.
// Rows need not be 16-byte aligned (dwordx4 loads from dword-aligned addresses); the last group of a row with inner % 4 != 0
// reads its 1-3 columns one by one.  FINAL: chunks == 1, the index goes straight to out[]; else partials [outer][chunks][inner].
template <bool IS_MAX, bool FINAL>
__global__ __launch_bounds__(256) void argreduce_cols_tile(const float *__restrict__ in, float *__restrict__ pv,
                                                           unsigned *__restrict__ pi, float *__restrict__ out,
                                                           unsigned axis_len, unsigned inner, unsigned chunk_len, unsigned xcd_runs) {
    __shared__ float sv[3][64][4];
    __shared__ unsigned si[3][64][4];
    const float id = IS_MAX ? -INFINITY : INFINITY;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned o = blockIdx.z, c = blockIdx.y, tile = blockIdx.x;
    const unsigned chunks = gridDim.y;
    if (xcd_runs) {
        // Rows that are not 16-byte multiples: a tile's 1 KiB piece of a row shares its first and its last 128-byte line with
        // the neighbouring tiles.  Workgroup L runs on XCD L % 8, so with the plain order neighbours sit on different XCDs and
        // each fetches the shared line for its own L2: 9 lines for 8, +12.4 % of traffic (FETCH_SIZE, 9973^2:
        // profiles/r06/arg_unaligned_probe.log).  Dealing the (tile, chunk, outer) units to the XCDs in eight contiguous runs
        // (np_sgemm.hip's tile_coords bijection) makes neighbouring tiles of a chunk share ONE L2.
        const unsigned T = gridDim.x, W = T * chunks * gridDim.z;
        const unsigned L = blockIdx.x + T * (blockIdx.y + chunks * blockIdx.z);
        const unsigned q = W / 8, r = W % 8, xcd = L % 8, idx = L / 8;
        const unsigned unit = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        tile = unit % T;
        c = (unit / T) % chunks;
        o = unit / (T * chunks);
    }
    const unsigned col = (tile * 64 + lane) * 4;
    const unsigned ncol = col >= inner ? 0u : (inner - col >= 4 ? 4u : inner - col);   // columns this lane owns
    const unsigned a0 = c * chunk_len;
    const unsigned a1 = axis_len - a0 < chunk_len ? axis_len : a0 + chunk_len;   // (a0 + chunk_len may wrap on an axis near 2^32)
    const float *p = in + (size_t)o * axis_len * inner + col;
    float bv[4] = {id, id, id, id};
    unsigned ba[4];
    const unsigned first = a0 + wave;
#pragma unroll
    for (int k = 0; k < 4; ++k) ba[k] = (first < a1 && (unsigned)k < ncol) ? first : kArgNone;
    if (ncol == 4) {
        unsigned a = first;
        for (; a + 28 < a1; a += 32) {   // eight rows in flight per lane
            v4f x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = ARG_LOAD4(p + (size_t)(a + 4 * u) * inner);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) arg_take<IS_MAX>(bv[k], ba[k], x[u][k], a + 4 * u);
        }
        for (; a + 12 < a1; a += 16) {
            const v4f x0 = ARG_LOAD4(p + (size_t)a * inner), x1 = ARG_LOAD4(p + (size_t)(a + 4) * inner);
            const v4f x2 = ARG_LOAD4(p + (size_t)(a + 8) * inner), x3 = ARG_LOAD4(p + (size_t)(a + 12) * inner);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                arg_take<IS_MAX>(bv[k], ba[k], x0[k], a);
                arg_take<IS_MAX>(bv[k], ba[k], x1[k], a + 4);
                arg_take<IS_MAX>(bv[k], ba[k], x2[k], a + 8);
                arg_take<IS_MAX>(bv[k], ba[k], x3[k], a + 12);
            }
        }
        for (; a < a1; a += 4) {
            const v4f x0 = ARG_LOAD4(p + (size_t)a * inner);
#pragma unroll
            for (int k = 0; k < 4; ++k) arg_take<IS_MAX>(bv[k], ba[k], x0[k], a);
        }
    } else if (ncol > 0) {
        // The last 1-3 columns of a row with inner % 4 != 0: ONE lane per chunk.  Until round 6 it walked its rows one scalar load
        // at a time — load, compare, next load: ~48 dependent memory round trips per column behind which the whole workgroup (and,
        // with every chunk's last tile doing the same, the launch) waited: 10007^2 ran 3.5 TB/s where 10008^2 runs 5.4
        // (profiles/r06/arg_unaligned_probe.log).  Eight rows in flight like the full lanes; a column this lane does not own is
        // read again as its last one (in bounds) and never taken.
        const unsigned k1 = ncol > 1 ? 1u : 0u, k2 = ncol > 2 ? 2u : k1;
        unsigned a = first;
        for (; a + 28 < a1; a += 32) {
            float x0[8], x1[8], x2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float *q = p + (size_t)(a + 4 * u) * inner;
                x0[u] = __builtin_nontemporal_load(q);
                x1[u] = __builtin_nontemporal_load(q + k1);
                x2[u] = __builtin_nontemporal_load(q + k2);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                arg_take<IS_MAX>(bv[0], ba[0], x0[u], a + 4 * u);
                if (ncol > 1) arg_take<IS_MAX>(bv[1], ba[1], x1[u], a + 4 * u);
                if (ncol > 2) arg_take<IS_MAX>(bv[2], ba[2], x2[u], a + 4 * u);
            }
        }
        for (; a < a1; a += 4) {
            const float *q = p + (size_t)a * inner;
            const float y0 = q[0], y1 = q[k1], y2 = q[k2];
            arg_take<IS_MAX>(bv[0], ba[0], y0, a);
            if (ncol > 1) arg_take<IS_MAX>(bv[1], ba[1], y1, a);
            if (ncol > 2) arg_take<IS_MAX>(bv[2], ba[2], y2, a);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sv[wave - 1][lane][k] = bv[k];
            si[wave - 1][lane][k] = ba[k];
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((unsigned)k >= ncol) continue;
            ArgPair r{bv[k], ba[k]};
            for (int w = 0; w < 3; ++w) r = arg_combine<IS_MAX>(r, ArgPair{sv[w][lane][k], si[w][lane][k]});
            if (IS_MAX && c == 0) {
                const float x0 = p[k];
                if (x0 != x0) r = ArgPair{INFINITY, 0u};                   // a NaN in position 0 is maximal
            }
            if (FINAL) {
                out[(size_t)o * inner + col + k] = (float)r.i;
            } else {
                const size_t at = ((size_t)o * chunks + c) * inner + col + k;
                pv[at] = r.v;
                pi[at] = r.i;
            }
        }
    }
}

// argmax / argmin over SHORT contiguous rows (the class scores of a sample: an N x 10 array, axis 1):
// L lanes per row (L = 1 .. 32), folded with xor-shuffles; a workgroup per row left 255 of 256 threads
// idle (10^7 x 10: 9 ms).
template <bool IS_MAX, int L>
__global__ __launch_bounds__(256) void argreduce_rows_group(const float *__restrict__ in, float *__restrict__ out,
                                                            size_t rows, unsigned len) {
    const size_t row = ((size_t)blockIdx.x * 256 + threadIdx.x) / L;
    const unsigned l = threadIdx.x % L;
    ArgPair best{IS_MAX ? -INFINITY : INFINITY, 0xffffffffu};
    if (row < rows) {
        const float *p = in + row * len;
        for (unsigned j = l; j < len; j += L) {
            const ArgPair c{arg_key<IS_MAX>(p[j], j), j};
            best = (best.i == 0xffffffffu) ? c : arg_combine<IS_MAX>(best, c);
        }
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) {
        ArgPair q;
        q.v = __shfl_xor(best.v, off, 64);
        q.i = __shfl_xor(best.i, off, 64);
        if (q.i != 0xffffffffu) best = (best.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(best, q);
    }
    if (l == 0 && row < rows) out[row] = (float)best.i;
}

// fold the per-chunk partials of each row (chunks are in index order) and write the float index
template <bool IS_MAX>
// partials are laid out [outer][chunks][inner]; output element = (o, j)
__global__ __launch_bounds__(256) void argreduce_fold_kernel(const float *__restrict__ pv,
                                                             const unsigned *__restrict__ pi,
                                                             float *__restrict__ out, size_t outputs,
                                                             unsigned chunks, size_t inner) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= outputs) return;
    const size_t o = idx / inner, j = idx - o * inner;
    const size_t base = o * chunks * inner + j;
    ArgPair r{pv[base], pi[base]};
    for (unsigned c = 1; c < chunks; ++c) {
        const ArgPair q{pv[base + (size_t)c * inner], pi[base + (size_t)c * inner]};
        if (q.i != 0xffffffffu) r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);
    }
    out[idx] = (float)r.i;
}

// the same fold with one WORKGROUP per output: with few outputs the chunk lists are long (3 outputs x
// 170 000 chunks for an N x 3 array) and a single thread walking one would take milliseconds
template <bool IS_MAX>
__global__ __launch_bounds__(256) void argreduce_fold_block_kernel(const float *__restrict__ pv,
                                                                   const unsigned *__restrict__ pi,
                                                                   float *__restrict__ out, unsigned chunks,
                                                                   size_t inner) {
    __shared__ float sv[4];
    __shared__ unsigned si[4];
    const size_t idx = blockIdx.x;
    const size_t o = idx / inner, j = idx - o * inner;
    const size_t base = o * chunks * inner + j;
    ArgPair best{IS_MAX ? -INFINITY : INFINITY, 0xffffffffu};
    for (unsigned cb = 0; cb < chunks; cb += 8 * blockDim.x) {   // eight (value, index) loads in flight per lane
        ArgPair q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned c = cb + u * blockDim.x + threadIdx.x;
            q[u] = c < chunks ? ArgPair{pv[base + (size_t)c * inner], pi[base + (size_t)c * inner]} : ArgPair{best.v, 0xffffffffu};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (q[u].i != 0xffffffffu) best = (best.i == 0xffffffffu) ? q[u] : arg_combine<IS_MAX>(best, q[u]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ArgPair q;
        q.v = __shfl_down(best.v, off, 64);
        q.i = __shfl_down(best.i, off, 64);
        if (q.i != 0xffffffffu) best = (best.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(best, q);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sv[wave] = best.v;
        si[wave] = best.i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ArgPair r{sv[0], si[0]};
        for (int w = 1; w < 4; ++w) {
            const ArgPair q{sv[w], si[w]};
            if (q.i != 0xffffffffu) r = (r.i == 0xffffffffu) ? q : arg_combine<IS_MAX>(r, q);
        }
        out[idx] = (float)r.i;
    }
}

// the same fold for WIDE inner (partials [outer][chunks][inner], inner >= 192: what argreduce_cols_tile leaves): a workgroup
// per COLS columns, lanes along the columns first (rows of partials are read in contiguous pieces), its 256 / COLS phases over
// interleaved chunks with four loads in flight, meeting in LDS.  (argreduce_fold_block_kernel reads one column's partials
// `inner` floats apart: a cache line per element — with 768 chunks of 1024 columns that fold cost more than the pass it followed.)
// COLS = 64, 16 or 4: the host takes the widest that still gives the fold 64 workgroups.
template <bool IS_MAX, int COLS>
__global__ __launch_bounds__(256) void argreduce_fold_cols_kernel(const float *__restrict__ pv, const unsigned *__restrict__ pi,
                                                                  float *__restrict__ out, unsigned chunks, size_t inner) {
    constexpr unsigned P = 256 / COLS;
    __shared__ float sv[256];
    __shared__ unsigned si[256];
    const unsigned col = threadIdx.x % COLS, ph = threadIdx.x / COLS;
    const size_t j = (size_t)blockIdx.x * COLS + col;
    const size_t o = blockIdx.y;
    ArgPair best{IS_MAX ? -INFINITY : INFINITY, kArgNone};
    if (j < inner) {
        const size_t base = o * chunks * inner + j;
        unsigned c = ph;
        for (; c + 3 * P < chunks; c += 4 * P) {
            const ArgPair q0{pv[base + (size_t)c * inner], pi[base + (size_t)c * inner]};
            const ArgPair q1{pv[base + (size_t)(c + P) * inner], pi[base + (size_t)(c + P) * inner]};
            const ArgPair q2{pv[base + (size_t)(c + 2 * P) * inner], pi[base + (size_t)(c + 2 * P) * inner]};
            const ArgPair q3{pv[base + (size_t)(c + 3 * P) * inner], pi[base + (size_t)(c + 3 * P) * inner]};
            best = arg_combine<IS_MAX>(best, arg_combine<IS_MAX>(arg_combine<IS_MAX>(q0, q1), arg_combine<IS_MAX>(q2, q3)));
        }
        for (; c < chunks; c += P) best = arg_combine<IS_MAX>(best, ArgPair{pv[base + (size_t)c * inner], pi[base + (size_t)c * inner]});
    }
    sv[threadIdx.x] = best.v;
    si[threadIdx.x] = best.i;
    __syncthreads();
    if (ph == 0 && j < inner) {
        for (unsigned q = 1; q < P; ++q) best = arg_combine<IS_MAX>(best, ArgPair{sv[q * COLS + col], si[q * COLS + col]});
        out[o * inner + j] = (float)best.i;
    }
}

// K_<IS_MAX[, further template arguments]> for this call's is_max: a launch site selects its kernel once and launches once
#define ARG_KERNEL(K_, ...) (is_max ? K_<true, ##__VA_ARGS__> : K_<false, ##__VA_ARGS__>)

// np_debug_argreduce_last_record: the NP_ARG_* record (np_hip_debug.h) of what the last np_argreduce call launched; cleared at the
// top of the entry point, one host store per launch site.
unsigned g_arg_record[NP_ARG_RECORD_WORDS];
unsigned g_arg_count = 0;
void arg_clear() {
    memset(g_arg_record, 0, sizeof g_arg_record);
    g_arg_count = 0;
}
void arg_note(unsigned kernel, unsigned targ, dim3 grid, size_t chunks, size_t chunk_len, unsigned xcd_runs) {
    memset(g_arg_record, 0, sizeof g_arg_record);
    g_arg_record[NP_ARG_KERNEL] = kernel;
    g_arg_record[NP_ARG_TEMPLATE] = targ;
    g_arg_record[NP_ARG_GRID_X] = grid.x;
    g_arg_record[NP_ARG_GRID_Y] = grid.y;
    g_arg_record[NP_ARG_GRID_Z] = grid.z;
    g_arg_record[NP_ARG_CHUNKS] = (unsigned)chunks;
    g_arg_record[NP_ARG_CHUNK_LEN] = (unsigned)chunk_len;
    g_arg_record[NP_ARG_XCD_RUNS] = xcd_runs;
    g_arg_count = 1;
}
void arg_note_fold(unsigned fold, unsigned cols, dim3 grid) {
    g_arg_record[NP_ARG_FOLD] = fold;
    g_arg_record[NP_ARG_FOLD_COLS] = cols;
    g_arg_record[NP_ARG_FOLD_GRID_X] = grid.x;
    g_arg_record[NP_ARG_FOLD_GRID_Y] = grid.y;
    g_arg_record[NP_ARG_FOLD_GRID_Z] = grid.z;
}

// fold [outer][chunks][inner] partials: thread per output for short chunk lists, workgroup per output
// for long ones
int launch_arg_fold(int is_max, const float *pv, const unsigned *pi, float *out, size_t outputs, size_t chunks, size_t inner) {
    hipStream_t s = np::stream();
    if (inner >= 192 && chunks > 8 && outputs / inner <= 65535) {
        const size_t outer = outputs / inner;
        const int cols = ((inner + 63) / 64) * outer >= 64 ? 64 : (((inner + 15) / 16) * outer >= 64 ? 16 : 4);
        const dim3 grid((unsigned)((inner + cols - 1) / cols), (unsigned)outer);
        const auto k = cols == 64   ? ARG_KERNEL(argreduce_fold_cols_kernel, 64)
                       : cols == 16 ? ARG_KERNEL(argreduce_fold_cols_kernel, 16)
                                    : ARG_KERNEL(argreduce_fold_cols_kernel, 4);
        arg_note_fold(NP_ARG_FOLD_COLS_KERNEL, (unsigned)cols, grid);
        k<<<grid, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);
        NP_LAUNCH_CHECK("argreduce_fold_cols_kernel");
        return NP_OK;
    }
    if (chunks > 64 && outputs <= 0x7fffffffu) {
        arg_note_fold(NP_ARG_FOLD_BLOCK, 0, dim3((unsigned)outputs));
        ARG_KERNEL(argreduce_fold_block_kernel)<<<(unsigned)outputs, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);
        NP_LAUNCH_CHECK("argreduce_fold_block_kernel");
        return NP_OK;
    }
    const unsigned fgrid = (unsigned)((outputs + 255) / 256);
    arg_note_fold(NP_ARG_FOLD_THREAD, 0, dim3(fgrid));
    ARG_KERNEL(argreduce_fold_kernel)<<<fgrid, 256, 0, s>>>(pv, pi, out, outputs, (unsigned)chunks, inner);
    NP_LAUNCH_CHECK("argreduce_fold_kernel");
    return NP_OK;
}

}  // namespace

extern "C" {

int np_debug_argreduce_last_record(unsigned *host_record, unsigned capacity, unsigned *host_count) {
    if (!host_count || (capacity && !host_record)) return np::fail(NP_ERR_INVALID, "np_debug_argreduce_last_record: null pointer");
    *host_count = g_arg_count;
    if (g_arg_count && capacity)
        for (unsigned w = 0; w < NP_ARG_RECORD_WORDS; ++w) host_record[w] = g_arg_record[w];
    return NP_OK;
}

int np_argreduce(int is_max, const float *in, size_t outer, size_t axis_len, size_t inner, float *out) {
    arg_clear();
    if (outer == 0 || inner == 0) return NP_OK;
    if (axis_len == 0) return np::fail(NP_ERR_INVALID, "attempt to get %s of an empty sequence", is_max ? "argmax" : "argmin");
    if (!in || !out) return np::fail(NP_ERR_INVALID, "np_argreduce: null pointer");
    // the kernels count along the axis in 32 bits and look up to 28 rows ahead of their position (`a + 28 < a1`): 256 below 2^32
    if (axis_len > 0xffffff00ull) return np::fail(NP_ERR_INVALID, "np_argreduce: axis too long");
    if (int rc = np::ensure_init()) return rc;
    hipStream_t s = np::stream();
    if (inner == 1 && axis_len <= 256 && outer >= 1024) {
        size_t L = 1;
        while (L * 8 < axis_len) L *= 2;
        const size_t blocks = (outer * L + 255) / 256;
        if (blocks <= 0x7fffffffu) {
            auto k = ARG_KERNEL(argreduce_rows_group, 32);
            switch (L) {
                case 1: k = ARG_KERNEL(argreduce_rows_group, 1); break;
                case 2: k = ARG_KERNEL(argreduce_rows_group, 2); break;
                case 4: k = ARG_KERNEL(argreduce_rows_group, 4); break;
                case 8: k = ARG_KERNEL(argreduce_rows_group, 8); break;
                case 16: k = ARG_KERNEL(argreduce_rows_group, 16); break;
                default: break;   // 32 lanes per row
            }
            arg_note(NP_ARG_KERNEL_ROWS_GROUP, (unsigned)L, dim3((unsigned)blocks), 1, axis_len, 0);
            k<<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len);
            NP_LAUNCH_CHECK("argreduce_rows_group");
            return NP_OK;
        }
    }
    if (inner == 1 && axis_len <= 32768 && outer >= (size_t)np::num_cus() * 16 && (outer + 3) / 4 <= 0x7fffffffu) {
        // many rows of a few hundred to a few thousand elements: one wave per row, one launch, no partials
        const unsigned grid = (unsigned)((outer + 3) / 4);
        arg_note(NP_ARG_KERNEL_ROWS_WAVE, 0, dim3(grid), 1, axis_len, 0);
        ARG_KERNEL(argreduce_rows_wave)<<<grid, 256, 0, s>>>(in, out, outer, (unsigned)axis_len);
        NP_LAUNCH_CHECK("argreduce_rows_wave");
        return NP_OK;
    }
    if (inner == 1) {
        // contiguous rows: (row, chunk) workgroups + a fold over the chunks of each row
        const size_t target = np::capped_grid((size_t)np::num_cus() * 8 + 1, (size_t)np::num_cus() * 8);   // odd: np_internal.h
        size_t chunks = 1;
        if (outer < target) {
            chunks = (target + outer - 1) / outer;
            const size_t max_chunks = (axis_len + 4095) / 4096;   // >= 4096 elements per chunk (four float4 per lane)
            if (chunks > max_chunks) chunks = max_chunks;
        }
        if (outer * chunks > 0x7fffffffull) return np::fail(NP_ERR_INVALID, "np_argreduce: too many rows");
        np::Scratch pv, pi;
        if (int rc = pv.alloc(outer * chunks * sizeof(float))) return rc;
        if (int rc = pi.alloc(outer * chunks * sizeof(unsigned))) return rc;
        const unsigned grid = (unsigned)(outer * chunks);
        arg_note(NP_ARG_KERNEL_ROWS, 0, dim3(grid), chunks, (axis_len + chunks - 1) / chunks, 0);
        ARG_KERNEL(argreduce_rows_kernel)<<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)chunks);
        NP_LAUNCH_CHECK("argreduce_rows_kernel");
        return launch_arg_fold(is_max, (const float *)pv.ptr, (const unsigned *)pi.ptr, out, outer, chunks, 1);
    }
    const size_t total = outer * inner;
    // a few columns (inner <= 64, or whole float4 groups up to 256 columns), many rows: slabs of rows as flat memory
    const bool groups4 = inner % 4 == 0 && inner <= 256;
    if ((groups4 || inner <= 64) && axis_len * inner >= 4096 && outer <= 65535) {
        // one long axis (outer == 1: argmax over the rows of an N x C array): TWO workgroups per CU — four float4 loads in flight per
        // lane fill the machine, and a quarter of the blocks is a quarter of the partials the fold has to read (profiles/r05/arg_flat_ab.log,
        // 2 against 8 per CU: N x 3 6.21 / 5.91 TB/s, N x 64 5.52 / 5.19, N x 256 5.61 / 5.15); with several outer slices eight, as before
        // (16 x 100000 x 60: 4.81 / 5.73)
        const size_t target_wg = (size_t)np::num_cus() * (size_t)(np::g_arg_flat_wg_per_cu > 0 ? np::g_arg_flat_wg_per_cu : (outer == 1 ? 2 : 8));
        size_t blocks = (target_wg + outer - 1) / outer;
        const size_t min_rows = (4096 + inner - 1) / inner;              // a block walks >= 16 KiB
        const size_t max_blocks = axis_len / min_rows > 0 ? axis_len / min_rows : 1;
        if (blocks > max_blocks) blocks = max_blocks;
        if (blocks < 1) blocks = 1;
        size_t rows_per_block = ((axis_len + blocks - 1) / blocks + 3) / 4 * 4;   // slabs start on a float4 boundary of the flat view
        if (rows_per_block * inner < (size_t(1) << 31)) {
            blocks = (axis_len + rows_per_block - 1) / rows_per_block;
            np::Scratch pv, pi;
            if (int rc = pv.alloc(total * blocks * sizeof(float))) return rc;
            if (int rc = pi.alloc(total * blocks * sizeof(unsigned))) return rc;
            const dim3 grid((unsigned)blocks, (unsigned)outer);
            // (float4 column groups or single columns: the same signature, the row width counted in the kernel's own unit)
            const auto k = groups4 ? ARG_KERNEL(argreduce_small_inner4) : ARG_KERNEL(argreduce_small_inner);
            arg_note(groups4 ? NP_ARG_KERNEL_SMALL_INNER4 : NP_ARG_KERNEL_SMALL_INNER, 0, grid, blocks, rows_per_block, 0);
            k<<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)(groups4 ? inner / 4 : inner), (unsigned)rows_per_block);
            NP_LAUNCH_CHECK("argreduce_small_inner");
            return launch_arg_fold(is_max, (const float *)pv.ptr, (const unsigned *)pi.ptr, out, total, blocks, inner);
        }
    }
    // wide inner: 64 float4 column groups per workgroup, the axis cut into chunks like the column sum (choose_splits)
    if (inner >= 192 && outer <= 65535 && axis_len >= 16) {
        const size_t inner4 = (inner + 3) / 4;
        const size_t tiles = (inner4 + 63) / 64;
        // TWO workgroups per CU when the rows are float4-aligned, EIGHT when they are not (the column SUM takes twelve, choose_splits:
        // its partials are 4 bytes per column and chunk; these are 8 and are read back by a fold with far fewer workgroups).  Same box,
        // 2 / 4 / 8 per CU (profiles/r05/arg_cols_ab.log): 65536 x 1024 5.92 / 5.54 / 5.17 TB/s, 25000 x 4000 6.26 / 6.17 / 5.87,
        // 64 x 1500 x 1000 5.71 / 5.61 / 5.33 — eight rows in flight per lane fill the machine from few workgroups, and fewer chunks
        // are fewer partials; 9973^2 (every wave-level load unaligned, latency-bound) 3.44 / 4.36 / 4.78.  Chunks of >= 64 rows, an
        // odd number of rows per chunk (np_internal.h: no power-of-two distances between the rows in flight)
        size_t chunks = 1;
        const bool rows_aligned = inner % 4 == 0 && ((uintptr_t)in & 15u) == 0;
        const size_t wg_per_cu = np::g_arg_cols_wg_per_cu > 0 ? (size_t)np::g_arg_cols_wg_per_cu : (rows_aligned ? 2 : 8);
        const size_t base_wg = tiles * outer, target_wg = (size_t)np::num_cus() * wg_per_cu;
        if (base_wg < target_wg) {
            // ROUNDED DOWN (round 6): with two fat workgroups per CU the launch must not exceed the machine — 39 tiles in
            // ceil(512 / 39) = 14 chunks are 546 workgroups, and the 34 beyond the 512 that start together run alone at the end:
            // 9984^2 5.56 -> 6.0 TB/s, 16384 x 6144 5.3 -> 6.2, 30000 x 3000 5.0 -> 5.6 with the count that fits; every shape whose
            // tile count divides 512 (1024, 2048, 4096, 8192 ... columns) was exact already (profiles/r06/arg_cols_ab.log)
            chunks = target_wg / base_wg;
            const size_t max_chunks = axis_len / 64 > 0 ? axis_len / 64 : 1;
            if (chunks > max_chunks) chunks = max_chunks;
            if (chunks < 1) chunks = 1;
        }
        size_t chunk_len = (axis_len + chunks - 1) / chunks;
        if (chunks > 1 && chunk_len % 2 == 0) ++chunk_len;
        chunks = (axis_len + chunk_len - 1) / chunk_len;
        if (tiles <= 0x7fffffffu && chunks <= 65535) {
            const dim3 grid((unsigned)tiles, (unsigned)chunks, (unsigned)outer);
            // neighbouring tiles on one XCD when rows straddle lines (argreduce_cols_tile; np_reduce_set_variant(4200001): off, A/B)
            const bool rows_are_lines = (inner * sizeof(float)) % 128 == 0 && ((uintptr_t)in & 127u) == 0;
            const unsigned xcd_runs = (!rows_are_lines && tiles > 1 && tiles * chunks * outer < (size_t(1) << 31) && !np::g_xcd_runs_off) ? 1u : 0u;
            if (chunks == 1) {
                arg_note(NP_ARG_KERNEL_COLS_TILE, 1, grid, chunks, chunk_len, xcd_runs);
                ARG_KERNEL(argreduce_cols_tile, true)<<<grid, 256, 0, s>>>(in, nullptr, nullptr, out, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
                NP_LAUNCH_CHECK("argreduce_cols_tile");
                return NP_OK;
            }
            np::Scratch pv, pi;
            if (int rc = pv.alloc(total * chunks * sizeof(float))) return rc;
            if (int rc = pi.alloc(total * chunks * sizeof(unsigned))) return rc;
            arg_note(NP_ARG_KERNEL_COLS_TILE, 0, grid, chunks, chunk_len, xcd_runs);
            ARG_KERNEL(argreduce_cols_tile, false)<<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, nullptr, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
            NP_LAUNCH_CHECK("argreduce_cols_tile");
            return launch_arg_fold(is_max, (const float *)pv.ptr, (const unsigned *)pi.ptr, out, total, chunks, inner);
        }
    }
    // few outputs, long axis (argmax over the rows of an N x 3 array): one thread per output would
    // leave the chip idle — cut the axis into chunks, then fold the (value, index) partials
    const size_t target_threads = (size_t)np::num_cus() * 2048;
    if (total < target_threads && axis_len >= 128) {
        size_t chunks = (target_threads + total - 1) / total;
        const size_t max_chunks = axis_len / 32;
        if (chunks > max_chunks) chunks = max_chunks;
        const size_t chunk_len = (axis_len + chunks - 1) / chunks;
        chunks = (axis_len + chunk_len - 1) / chunk_len;
        if (chunks > 1) {
            np::Scratch pv, pi;
            if (int rc = pv.alloc(total * chunks * sizeof(float))) return rc;
            if (int rc = pi.alloc(total * chunks * sizeof(unsigned))) return rc;
            size_t blocks = (total * chunks + 255) / 256;
            const size_t cap = (size_t)np::num_cus() * 16;
            if (blocks > cap) blocks = cap;
            arg_note(NP_ARG_KERNEL_CHUNKS, 0, dim3((unsigned)blocks), chunks, chunk_len, 0);
            ARG_KERNEL(argreduce_chunks_kernel)<<<(unsigned)blocks, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, outer, (unsigned)axis_len, inner, (unsigned)chunks, (unsigned)chunk_len);
            NP_LAUNCH_CHECK("argreduce_chunks_kernel");
            return launch_arg_fold(is_max, (const float *)pv.ptr, (const unsigned *)pi.ptr, out, total, chunks, inner);
        }
    }
    size_t blocks = (total + 255) / 256;
    const size_t cap = (size_t)np::num_cus() * 16;
    if (blocks > cap) blocks = cap;
    arg_note(NP_ARG_KERNEL_GENERIC, 0, dim3((unsigned)blocks), 1, axis_len, 0);
    ARG_KERNEL(argreduce_generic_kernel)<<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len, inner);
    NP_LAUNCH_CHECK("argreduce_generic_kernel");
    return NP_OK;
}

}  // extern "C"
