// Reductions of libnp_hip.so: full reductions (sum / prod / min / max / mean) and single-axis
// reductions over a contiguous array viewed as outer x axis_len x inner.
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

// Workgroups per CU of the streaming reductions' first pass (np_reduce_set_variant; tools/reduce_cap_ab.py).
// One partial per workgroup, so more workgroups = more partials for the one-block second pass to fold.
int g_wg_per_cu = 0;   // 0 = the default below
int g_arg_flat_wg_per_cu = 0;   // the flat walks for a few columns: workgroups per CU, 0 = by shape (np_reduce_set_variant(4100000 + N): A/B)
int g_small_inner_dword = 0;    // reduce_small_inner: 1 = the dword walk of rounds 1-5 (np_reduce_set_variant(4300001): A/B)
int g_arg_xcd_runs_off = 0;     // argreduce_cols_tile on unaligned rows: 1 = the plain workgroup order (np_reduce_set_variant(4200001): A/B)
int g_arg_cols_wg_per_cu = 0;   // argreduce_cols_tile: workgroups per CU the axis is cut for; 0 = by alignment (np_reduce_set_variant(4000000 + N): A/B)
constexpr int kStreamWgPerCu = 8;
// np_debug_reduce_last_path: the NP_REDUCE_PATH_* bits of what the last np_reduce_axis / np_reduce_all(_dev) call launched, its
// recursion on partials included.  A plain process global, cleared at the top of those entry points.
unsigned g_last_path = 0;
inline size_t stream_cap() {
    if (g_wg_per_cu >= 1000) return (size_t)g_wg_per_cu;   // tuning: an exact workgroup count
    return (size_t)np::num_cus() * (size_t)(g_wg_per_cu > 0 ? g_wg_per_cu : kStreamWgPerCu);
}

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

// two sums behind one first pass (weighted_sums_pass1): workgroup b folds partials[b * np ...] into out[b], reduce_all_pass2's order
__global__ __launch_bounds__(256) void reduce_all_pass2_pair(const float *__restrict__ partials, int np, float *__restrict__ out) {
    __shared__ float lds4[4];
    const float *p = partials + (size_t)blockIdx.x * np;
    float r = 0.0f;
    for (int base = 0; base < np; base += 8 * (int)blockDim.x) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * (int)blockDim.x + (int)threadIdx.x;
            v[u] = i < np ? p[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) r += v[u];
    }
    r = block_reduce<NP_SUM>(r, lds4);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// Fused sum-reductions over a transformed input (src/ndmath/statistics.c):
//   XFORM 1: (x - p0)^2      second pass of variance / std (p0 = mean)
//   XFORM 2: x * y           weighted sum of NDArray_Average
//   XFORM 3: x != y ? 1 : 0                  mismatch count of NDArray_ArrayEqual (logic.c:686-690)
//   XFORM 4: |x-y| > p1 + p0*|y| ? 1 : 0     violation count of float_allclose (logic.c:730-733)
// Same streaming structure as reduce_all_pass1 (float4 nt loads, wave shuffle + LDS, one partial
// per workgroup); requires 16-byte aligned inputs (callers fall back to XFORM via scalar head/tail).
template <int XFORM>
__device__ __forceinline__ float xform_term(float x, float y, float p0, float p1) {
    if constexpr (XFORM == 1) {
        const float d = x - p0;
        return d * d;
    } else if constexpr (XFORM == 2) {
        return x * y;
    } else if constexpr (XFORM == 3) {
        return (x != y) ? 1.0f : 0.0f;   // NaN != NaN, as the reference's C loop
    } else {
        // the reference's expression; `atol + rtol * fabsf(b)` is one fused multiply-add in a
        // gcc -march=native build.  NaN compares false -> "close".
        const float diff = fabsf(x - y);
        const float tolerance = __fmaf_rn(p0, fabsf(y), p1);
        return (diff > tolerance) ? 1.0f : 0.0f;
    }
}

template <int XFORM, typename I>
__global__ __launch_bounds__(256) void reduce_xform_pass1(const float *__restrict__ in,
                                                          const float *__restrict__ in2,
                                                          float *__restrict__ partials, I n, I nvec,
                                                          float p0, float p1, unsigned *__restrict__ ticket,
                                                          float *__restrict__ out) {
    __shared__ float lds4[4];
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    v4f acc0{0, 0, 0, 0}, acc1 = acc0;
    auto xf = [&](float x, float y) -> float { return xform_term<XFORM>(x, y, p0, p1); };
    I v = tid;
    for (; v + stride < nvec; v += 2 * stride) {
        const v4f x0 = __builtin_nontemporal_load((const v4f_u *)(in + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f_u *)(in + (size_t)(v + stride) * 4));
        v4f y0{0, 0, 0, 0}, y1 = y0;
        if constexpr (XFORM >= 2) {
            y0 = __builtin_nontemporal_load((const v4f_u *)(in2 + (size_t)v * 4));
            y1 = __builtin_nontemporal_load((const v4f_u *)(in2 + (size_t)(v + stride) * 4));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc0[k] += xf(x0[k], y0[k]);
            acc1[k] += xf(x1[k], y1[k]);
        }
    }
    for (; v < nvec; v += stride) {
        const v4f x0 = *(const v4f_u *)(in + (size_t)v * 4);
        v4f y0{0, 0, 0, 0};
        if constexpr (XFORM >= 2) y0 = *(const v4f_u *)(in2 + (size_t)v * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc0[k] += xf(x0[k], y0[k]);
    }
    float r = (acc0[0] + acc1[0]) + (acc0[1] + acc1[1]) + ((acc0[2] + acc1[2]) + (acc0[3] + acc1[3]));
    if (blockIdx.x == 0) {
        const I t = nvec * 4 + threadIdx.x;   // ragged tail (n % 4 elements)
        if (t < n) r += xf(in[t], XFORM >= 2 ? in2[t] : 0.0f);
    }
    r = block_reduce<NP_SUM>(r, lds4);
    fold_in_last_workgroup<NP_SUM>(r, partials, ticket, out, 1.0f, lds4);
}

// generic (misaligned views): one thread per element stride, scalar loads
template <int XFORM, typename I>
__global__ __launch_bounds__(256) void reduce_xform_scalar(const float *__restrict__ in,
                                                           const float *__restrict__ in2,
                                                           float *__restrict__ partials, I n, float p0,
                                                           float p1, unsigned *__restrict__ ticket,
                                                           float *__restrict__ out) {
    __shared__ float lds4[4];
    const I stride = (I)gridDim.x * blockDim.x;
    float r = 0.0f;
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        r += xform_term<XFORM>(in[i], XFORM >= 2 ? in2[i] : 0.0f, p0, p1);
    r = block_reduce<NP_SUM>(r, lds4);
    fold_in_last_workgroup<NP_SUM>(r, partials, ticket, out, 1.0f, lds4);
}

// ------------------------------------------------------------------------------------------
// mean and sum of squared deviations in ONE read (variance / std, src/ndmath/statistics.c:88-130)
// ------------------------------------------------------------------------------------------
//
// The reference forms the mean with one pass (NDArray_Sum_Float / numElements, statistics.c:95,119) and walks the
// array again for sum (x - mean)^2 (:98-100; variance: Subtract, Abs, Pow, Sum — four more passes and three
// temporaries, :119-129).  Here every element is read once: a running (count, mean, M2) per lane, merged pairwise
// (Chan, Golub & LeVeque) through the wave shuffles, LDS and the per-workgroup partials of the other reductions.
//
// What keeps that at the accuracy of the two-pass form in fp32: a mean is carried as ANCHOR + OFFSET — `k`, a float near
// the mean (a data value for a fresh batch, the rounded mean after a merge), and `mu` = mean - k, far below the data's
// magnitude.  A merge needs the difference of two means, (kb - ka) + (mub - mua): floats that are close subtract exactly,
// and every rounding that is left is relative to that difference — a mean stored as ONE float is off by up to half an ulp
// of ITS OWN magnitude, an error that enters a merge to first order (2 delta eps n_a n_b / n) and is 6e-5 of the variance
// of a few hundred values near 1e4.  Within a lane a trip's 16 values are taken relative to the first of them: s = sum d, q = sum d^2,
// M2 = q - s^2 / 16; that subtraction cancels at most four bits (the anchor is one of the 16: s^2 <= 15 q).
// Order of the merges is fixed by the launch geometry: bit-identical from run to run.  NaN / inf anywhere: NaN, as the
// reference's inf - inf.
struct Mom {
    float n, k, mu, m2;   // count; anchor; mean - anchor; sum of squared deviations from the mean
};

// a comes first; 1 / (a.n + b.n) to an ulp is enough (the error is relative to delta)
__device__ __forceinline__ Mom mom_merge(const Mom a, const Mom b) {
    const float n = a.n + b.n;
    const float delta = (b.k - a.k) + (b.mu - a.mu);
    const float w = b.n * __builtin_amdgcn_rcpf(n);
    Mom r;
    r.n = n;
    // the merged mean a.k + (a.mu + delta w), renormalised (TwoSum): the anchor moves to the mean rounded to a float and the
    // offset becomes what that rounding lost — an offset kept relative to a FAR anchor (an outlier that happened to come
    // first) would carry the rounding error of its own size, eps |mean - k|, into the mean
    const float mu = __fmaf_rn(delta, w, a.mu);
    const float k = a.k + mu;
    const float bb = k - a.k;
    r.k = k;
    r.mu = (a.k - (k - bb)) + (mu - bb);
    r.m2 = (a.m2 + b.m2) + delta * delta * (a.n * w);
    const bool a_empty = a.n == 0.0f, b_empty = b.n == 0.0f;
    if (b_empty) r = a;
    if (a_empty) r = b;
    return r;
}

// four values as one batch, anchored on the first
__device__ __forceinline__ Mom mom_of4(const v4f x) {
    const float k = x[0];
    const float d1 = x[1] - k, d2 = x[2] - k, d3 = x[3] - k;
    const float s = (d1 + d2) + d3;
    const float q = __fmaf_rn(d3, d3, __fmaf_rn(d2, d2, d1 * d1));
    const float mu = 0.25f * s;
    return Mom{4.0f, k, mu, __fmaf_rn(-s, mu, q) + (k - k)};   // k - k: 0, or NaN for an infinite anchor (inf is not "equal to the mean")
}

// sixteen values (a lane's four loads of one trip) as one batch, anchored on the first
__device__ __forceinline__ Mom mom_of16(const v4f x0, const v4f x1, const v4f x2, const v4f x3) {
    const float k = x0[0];
    v4f s4{0, 0, 0, 0}, q4 = s4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float d0 = x0[c] - k, d1 = x1[c] - k, d2 = x2[c] - k, d3 = x3[c] - k;
        s4[c] = (d0 + d1) + (d2 + d3);
        q4[c] = __fmaf_rn(d3, d3, __fmaf_rn(d2, d2, __fmaf_rn(d1, d1, d0 * d0)));
    }
    const float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    const float q = (q4[0] + q4[1]) + (q4[2] + q4[3]);
    const float mu = 0.0625f * s;
    return Mom{16.0f, k, mu, __fmaf_rn(-s, mu, q)};   // d0 of component 0 is k - k: NaN for an infinite anchor
}

__device__ __forceinline__ Mom mom_shfl_down(const Mom a, int off) {
    return Mom{__shfl_down(a.n, off, 64), __shfl_down(a.k, off, 64), __shfl_down(a.mu, off, 64), __shfl_down(a.m2, off, 64)};
}

// the 256 threads' states -> one, valid in thread 0: lanes pairwise (offsets 32 ... 1), then the four waves in order
__device__ __forceinline__ Mom mom_block_reduce(Mom a, Mom *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = mom_merge(a, mom_shfl_down(a, off));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
        for (int w = 1; w < 4; ++w) a = mom_merge(a, lds[w]);
    }
    return a;
}

// thread t merges partials t, t + 256, ... in that order, the workgroup joins them; partials are [4][np] (n, k, mu, m2)
template <bool COHERENT>
__device__ __forceinline__ Mom mom_fold_partials(const float *partials, unsigned np, Mom *lds) {
    Mom f{0.0f, 0.0f, 0.0f, 0.0f};
    // nine partials per thread in flight: the 2049 of a 10^8-element pass are ONE trip (three dependent trips of four cost the
    // one-workgroup fold ~3 us of memory round trips, of a 72 us call)
    constexpr int UNR = 9;
    for (unsigned base = 0; base < np; base += UNR * 256u) {
        Mom v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const unsigned i = base + u * 256u + threadIdx.x;
            v[u] = Mom{0.0f, 0.0f, 0.0f, 0.0f};
            if (i < np) {
                if constexpr (COHERENT)
                    v[u] = Mom{coherent_load(&partials[i]), coherent_load(&partials[np + i]), coherent_load(&partials[2 * np + i]),
                               coherent_load(&partials[3 * np + i])};
                else
                    v[u] = Mom{partials[i], partials[np + i], partials[2 * np + i], partials[3 * np + i]};
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) f = mom_merge(f, v[u]);
    }
    return mom_block_reduce(f, lds);
}

// out[0] = mean, out[1] = sum (x - mean)^2
__device__ __forceinline__ void mom_write(const Mom r, float *out) {
    out[0] = r.k + r.mu;
    out[1] = r.m2;
}

// pass 1: the walk of reduce_all_pass1 (aligned non-temporal float4 loads from in + head, four in flight per lane, the <= 3
// vectors left at the end of a lane's walk issued together; block 0 takes the ragged head and tail)
template <typename I>
__global__ __launch_bounds__(256) void moments_pass1(const float *__restrict__ in, float *__restrict__ partials, I n, I head,
                                                     I nvec, unsigned *__restrict__ ticket, float *__restrict__ out) {
    __shared__ Mom lds[4];
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    const float *base = in + head;
    Mom acc{0.0f, 0.0f, 0.0f, 0.0f};
    I v = tid;
    for (; v + 3 * stride < nvec; v += 4 * stride) {
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + stride) * 4));
        const v4f x2 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + 2 * stride) * 4));
        const v4f x3 = __builtin_nontemporal_load((const v4f *)(base + (size_t)(v + 3 * stride) * 4));
        acc = mom_merge(acc, mom_of16(x0, x1, x2, x3));
    }
    if (v < nvec) {
        const I v1 = v + stride, v2 = v + 2 * stride;
        const bool h1 = v1 < nvec, h2 = v2 < nvec;
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v * 4));
        v4f x1{0, 0, 0, 0}, x2 = x1;
        if (h1) x1 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v1 * 4));
        if (h2) x2 = __builtin_nontemporal_load((const v4f *)(base + (size_t)v2 * 4));
        acc = mom_merge(acc, mom_of4(x0));
        if (h1) acc = mom_merge(acc, mom_of4(x1));
        if (h2) acc = mom_merge(acc, mom_of4(x2));
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) {
            const float x = in[threadIdx.x];
            acc = mom_merge(acc, Mom{1.0f, x, 0.0f, x - x});
        }
        const I t = head + nvec * 4 + threadIdx.x;
        if (t < n) {
            const float x = in[t];
            acc = mom_merge(acc, Mom{1.0f, x, 0.0f, x - x});
        }
    }
    acc = mom_block_reduce(acc, lds);
    const unsigned np = gridDim.x;
    if (np == 1) {
        if (threadIdx.x == 0) mom_write(acc, out);
        return;
    }
    if (!ticket) {   // a one-workgroup second kernel folds
        if (threadIdx.x == 0) {
            partials[blockIdx.x] = acc.n;
            partials[np + blockIdx.x] = acc.k;
            partials[2 * np + blockIdx.x] = acc.mu;
            partials[3 * np + blockIdx.x] = acc.m2;
        }
        return;
    }
    if (threadIdx.x == 0) {
        coherent_store(&partials[blockIdx.x], acc.n);
        coherent_store(&partials[np + blockIdx.x], acc.k);
        coherent_store(&partials[2 * np + blockIdx.x], acc.mu);
        coherent_store(&partials[3 * np + blockIdx.x], acc.m2);
    }
    if (!last_workgroup_done(ticket, np)) return;
    const Mom r = mom_fold_partials<true>(partials, np, lds);
    if (threadIdx.x == 0) {
        mom_write(r, out);
        coherent_store(ticket, 0u);
    }
}

__global__ __launch_bounds__(256) void moments_pass2(const float *__restrict__ partials, unsigned np, float *__restrict__ out) {
    __shared__ Mom lds[4];
    const Mom r = mom_fold_partials<false>(partials, np, lds);
    if (threadIdx.x == 0) mom_write(r, out);
}

// sum a w and sum w of NDArray_Average (statistics.c:147-150) in one read of both arrays: the walk of
// reduce_xform_pass1 (dword-aligned float4 loads: the two operands need not agree in alignment) with two sums per lane.
// Partials [2][blocks]; out[0] = sum a w, out[1] = sum w.
template <typename I>
__global__ __launch_bounds__(256) void weighted_sums_pass1(const float *__restrict__ a, const float *__restrict__ w,
                                                           float *__restrict__ partials, I n, I nvec,
                                                           unsigned *__restrict__ ticket, float *__restrict__ out) {
    __shared__ float lds4[4];
    __shared__ float lds4b[4];
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    v4f p0{0, 0, 0, 0}, p1 = p0, s0 = p0, s1 = p0;
    I v = tid;
    for (; v + stride < nvec; v += 2 * stride) {
        const v4f x0 = __builtin_nontemporal_load((const v4f_u *)(a + (size_t)v * 4));
        const v4f x1 = __builtin_nontemporal_load((const v4f_u *)(a + (size_t)(v + stride) * 4));
        const v4f y0 = __builtin_nontemporal_load((const v4f_u *)(w + (size_t)v * 4));
        const v4f y1 = __builtin_nontemporal_load((const v4f_u *)(w + (size_t)(v + stride) * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p0[k] += x0[k] * y0[k];   // a product rounded, then added: NDArray_Multiply_Float then NDArray_Sum_Float (no FMA)
            p1[k] += x1[k] * y1[k];
            s0[k] += y0[k];
            s1[k] += y1[k];
        }
    }
    if (v < nvec) {
        const v4f x0 = *(const v4f_u *)(a + (size_t)v * 4);
        const v4f y0 = *(const v4f_u *)(w + (size_t)v * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p0[k] += x0[k] * y0[k];
            s0[k] += y0[k];
        }
    }
    float rp = (p0[0] + p1[0]) + (p0[1] + p1[1]) + ((p0[2] + p1[2]) + (p0[3] + p1[3]));
    float rs = (s0[0] + s1[0]) + (s0[1] + s1[1]) + ((s0[2] + s1[2]) + (s0[3] + s1[3]));
    if (blockIdx.x == 0) {
        const I t = nvec * 4 + threadIdx.x;   // ragged tail (n % 4 elements)
        if (t < n) {
            rp += a[t] * w[t];
            rs += w[t];
        }
    }
    rp = block_reduce<NP_SUM>(rp, lds4);
    rs = block_reduce<NP_SUM>(rs, lds4b);
    const unsigned np = gridDim.x;
    if (np == 1) {
        if (threadIdx.x == 0) {
            out[0] = rp;
            out[1] = rs;
        }
        return;
    }
    if (!ticket) {
        if (threadIdx.x == 0) {
            partials[blockIdx.x] = rp;
            partials[np + blockIdx.x] = rs;
        }
        return;
    }
    if (threadIdx.x == 0) {
        coherent_store(&partials[blockIdx.x], rp);
        coherent_store(&partials[np + blockIdx.x], rs);
    }
    if (!last_workgroup_done(ticket, np)) return;
    // np <= 256 (np::fold_ticket): one partial of each sum per thread, the fold order of reduce_all_pass2
    float fp = 0.0f, fs = 0.0f;
    for (unsigned i = threadIdx.x; i < np; i += blockDim.x) {
        fp += coherent_load(&partials[i]);
        fs += coherent_load(&partials[np + i]);
    }
    __syncthreads();   // lds4 / lds4b are read by thread 0 of block_reduce above
    fp = block_reduce<NP_SUM>(fp, lds4);
    fs = block_reduce<NP_SUM>(fs, lds4b);
    if (threadIdx.x == 0) {
        out[0] = fp;
        out[1] = fs;
        coherent_store(ticket, 0u);
    }
}

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

// NDArray_All (logic.c:25-58) as a min-reduction over a per-element verdict (1 = passes).
// QUIRK: index < body_end follows the reference's AVX2 body, which tests `movemask != 0x0F` on an
// 8-lane mask: lanes 0-3 of every 8-block must be non-zero and non-NaN (_CMP_NEQ_OQ true) and
// lanes 4-7 must NOT be (zero or NaN); the rest follows the scalar tail (x == 0.0 fails).
template <bool QUIRK, typename I>
__device__ __forceinline__ float all_verdict(float x, I index, I body_end) {
    if (QUIRK && index < body_end) {
        const bool neq_oq = (x < 0.0f) || (x > 0.0f);
        return (((index & 7) < 4) == neq_oq) ? 1.0f : 0.0f;
    }
    return (x == 0.0f) ? 0.0f : 1.0f;
}

template <bool QUIRK, typename I>
__global__ __launch_bounds__(256) void all_pass1(const float *__restrict__ in,
                                                 float *__restrict__ partials, I n, I head, I nvec,
                                                 I body_end, unsigned *__restrict__ ticket,
                                                 float *__restrict__ out) {
    __shared__ float lds4[4];
    const I stride = (I)gridDim.x * blockDim.x;
    float r = 1.0f;
    const float *base = in + head;
    for (I v = (I)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
        const v4f x = __builtin_nontemporal_load((const v4f *)(base + (size_t)v * 4));
#pragma unroll
        for (int k = 0; k < 4; ++k) r = fminf(r, all_verdict<QUIRK, I>(x[k], head + v * 4 + k, body_end));
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) r = fminf(r, all_verdict<QUIRK, I>(in[threadIdx.x], (I)threadIdx.x, body_end));
        const I t = head + nvec * 4 + threadIdx.x;
        if (t < n) r = fminf(r, all_verdict<QUIRK, I>(in[t], t, body_end));
    }
    r = block_reduce<NP_MIN>(r, lds4);
    fold_in_last_workgroup<NP_MIN>(r, partials, ticket, out, 1.0f, lds4);
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

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------


template <int OP, typename I>
int launch_reduce_all(const float *in, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    size_t head = ((16 - ((uintptr_t)in & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    // enough workgroups to fill the chip (8 per CU), but never more than one per 4 KiB of input
    size_t blocks = np::capped_grid((nvec + 255) / 256, stream_cap());
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

// how many chunks to cut the axis into so that the column reduce has >= ~8 workgroups per CU
size_t choose_splits(size_t outer, size_t axis_len, size_t inner4) {
    const size_t col_tiles = (inner4 + 63) / 64;
    const size_t base = col_tiles * outer;
    // 12 workgroups per CU (tuning: stream_cap() x 3/2), and an ODD number of rows per chunk: chunks that start a
    // power-of-two number of rows apart (65536 x 4096 in 128 chunks: 512 rows = 8 MiB) put every workgroup's
    // current row on the same HBM channels — 6.19 TB/s against 6.45-6.50 (profiles/r02/reduce_cap_ab_2.log)
    const size_t target = stream_cap() * 3 / 2;
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
                                  (size_t)grid.x * grid.y * grid.z < (size_t(1) << 31) && !g_arg_xcd_runs_off ? 1u : 0u;
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

}  // extern "C" (the template below cannot have C linkage)

// mean and sum of squared deviations -> dev_out[0], dev_out[1]: one streaming pass (+ a one-workgroup fold above 256 workgroups)
template <typename I>
static int launch_moments(const float *in, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    size_t head = ((16 - ((uintptr_t)in & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    size_t blocks = np::capped_grid((nvec + 255) / 256, stream_cap());
    if (np::g_small_reduce_blocks && n <= (size_t(1) << 20) && blocks > np::g_small_reduce_blocks) blocks = np::g_small_reduce_blocks;
    np::Scratch partials;
    if (int rc = partials.alloc(4 * blocks * sizeof(float))) return rc;
    unsigned *ticket = np::fold_ticket(blocks);
    moments_pass1<I><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)partials.ptr, (I)n, (I)head, (I)nvec, ticket, dev_out);
    NP_LAUNCH_CHECK("moments_pass1");
    if (ticket || blocks == 1) return NP_OK;
    moments_pass2<<<1, 256, 0, s>>>((const float *)partials.ptr, (unsigned)blocks, dev_out);
    NP_LAUNCH_CHECK("moments_pass2");
    return NP_OK;
}

// sum a w -> dev_out[0], sum w -> dev_out[1]
template <typename I>
static int launch_weighted_sums(const float *a, const float *w, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    const size_t nvec = n / 4;
    const size_t blocks = np::capped_grid((nvec + 255) / 256, stream_cap());
    np::Scratch partials;
    if (int rc = partials.alloc(2 * blocks * sizeof(float))) return rc;
    unsigned *ticket = np::fold_ticket(blocks);
    weighted_sums_pass1<I><<<(unsigned)blocks, 256, 0, s>>>(a, w, (float *)partials.ptr, (I)n, (I)nvec, ticket, dev_out);
    NP_LAUNCH_CHECK("weighted_sums_pass1");
    if (ticket || blocks == 1) return NP_OK;
    reduce_all_pass2_pair<<<2, 256, 0, s>>>((const float *)partials.ptr, (int)blocks, dev_out);
    NP_LAUNCH_CHECK("reduce_all_pass2_pair");
    return NP_OK;
}

// sum over XFORM(in[, in2]) -> one device float (32-bit indices below 2^31 elements, 64-bit beyond: array_equal / allclose of
// arrays the reference's `int` counts cannot address but 288 GB of HBM can hold)
template <int XFORM, typename I>
static int xform_sum_as(const float *in, const float *in2, size_t n, float p0, float p1, float *dev_out) {
    hipStream_t s = np::stream();
    const size_t nvec = n / 4;   // dword-aligned float4 loads: views may start anywhere
    const size_t blocks = np::capped_grid((nvec + 255) / 256, stream_cap());
    np::Scratch partials;
    if (int rc = partials.alloc(blocks * sizeof(float))) return rc;
    unsigned *ticket = np::fold_ticket(blocks);
    reduce_xform_pass1<XFORM, I><<<(unsigned)blocks, 256, 0, s>>>(in, in2, (float *)partials.ptr, (I)n, (I)nvec, p0, p1, ticket, dev_out);
    NP_LAUNCH_CHECK("reduce_xform");
    if (ticket) return NP_OK;
    reduce_all_pass2<NP_SUM><<<1, 256, 0, s>>>((const float *)partials.ptr, (int)blocks, dev_out, 1.0f);
    NP_LAUNCH_CHECK("reduce_all_pass2");
    return NP_OK;
}

template <int XFORM>
static int xform_sum(const float *in, const float *in2, size_t n, float p0, float p1, float *dev_out) {
    if (n < (size_t(1) << 31)) return xform_sum_as<XFORM, uint32_t>(in, in2, n, p0, p1, dev_out);
    return xform_sum_as<XFORM, uint64_t>(in, in2, n, p0, p1, dev_out);
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

// fold [outer][chunks][inner] partials: thread per output for short chunk lists, workgroup per output
// for long ones
static int launch_arg_fold(int is_max, const float *pv, const unsigned *pi, float *out, size_t outputs,
                           size_t chunks, size_t inner) {
    hipStream_t s = np::stream();
    if (inner >= 192 && chunks > 8 && outputs / inner <= 65535) {
        const size_t outer = outputs / inner;
        const int cols = ((inner + 63) / 64) * outer >= 64 ? 64 : (((inner + 15) / 16) * outer >= 64 ? 16 : 4);
        const dim3 grid((unsigned)((inner + cols - 1) / cols), (unsigned)outer);
#define NP_FOLDC(C_)                                                                                          \
    do {                                                                                                      \
        if (is_max) argreduce_fold_cols_kernel<true, C_><<<grid, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);  \
        else argreduce_fold_cols_kernel<false, C_><<<grid, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);        \
    } while (0)
        if (cols == 64) NP_FOLDC(64);
        else if (cols == 16) NP_FOLDC(16);
        else NP_FOLDC(4);
#undef NP_FOLDC
        NP_LAUNCH_CHECK("argreduce_fold_cols_kernel");
        return NP_OK;
    }
    if (chunks > 64 && outputs <= 0x7fffffffu) {
        if (is_max)
            argreduce_fold_block_kernel<true><<<(unsigned)outputs, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);
        else
            argreduce_fold_block_kernel<false><<<(unsigned)outputs, 256, 0, s>>>(pv, pi, out, (unsigned)chunks, inner);
        NP_LAUNCH_CHECK("argreduce_fold_block_kernel");
        return NP_OK;
    }
    const unsigned fgrid = (unsigned)((outputs + 255) / 256);
    if (is_max)
        argreduce_fold_kernel<true><<<fgrid, 256, 0, s>>>(pv, pi, out, outputs, (unsigned)chunks, inner);
    else
        argreduce_fold_kernel<false><<<fgrid, 256, 0, s>>>(pv, pi, out, outputs, (unsigned)chunks, inner);
    NP_LAUNCH_CHECK("argreduce_fold_kernel");
    return NP_OK;
}

extern "C" {

int np_argreduce(int is_max, const float *in, size_t outer, size_t axis_len, size_t inner, float *out) {
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
#define NP_AG(L_)                                                                                         \
    do {                                                                                                  \
        if (is_max)                                                                                       \
            argreduce_rows_group<true, L_><<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len);  \
        else                                                                                              \
            argreduce_rows_group<false, L_><<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len); \
    } while (0)
            switch (L) {
                case 1: NP_AG(1); break;
                case 2: NP_AG(2); break;
                case 4: NP_AG(4); break;
                case 8: NP_AG(8); break;
                case 16: NP_AG(16); break;
                default: NP_AG(32); break;
            }
#undef NP_AG
            NP_LAUNCH_CHECK("argreduce_rows_group");
            return NP_OK;
        }
    }
    if (inner == 1 && axis_len <= 32768 && outer >= (size_t)np::num_cus() * 16 && (outer + 3) / 4 <= 0x7fffffffu) {
        // many rows of a few hundred to a few thousand elements: one wave per row, one launch, no partials
        const unsigned grid = (unsigned)((outer + 3) / 4);
        if (is_max)
            argreduce_rows_wave<true><<<grid, 256, 0, s>>>(in, out, outer, (unsigned)axis_len);
        else
            argreduce_rows_wave<false><<<grid, 256, 0, s>>>(in, out, outer, (unsigned)axis_len);
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
        if (is_max)
            argreduce_rows_kernel<true><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)chunks);
        else
            argreduce_rows_kernel<false><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)chunks);
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
        const size_t target_wg = (size_t)np::num_cus() * (size_t)(g_arg_flat_wg_per_cu > 0 ? g_arg_flat_wg_per_cu : (outer == 1 ? 2 : 8));
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
            if (groups4) {
                if (is_max)
                    argreduce_small_inner4<true><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)(inner / 4), (unsigned)rows_per_block);
                else
                    argreduce_small_inner4<false><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)(inner / 4), (unsigned)rows_per_block);
            } else if (is_max) {
                argreduce_small_inner<true><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)inner, (unsigned)rows_per_block);
            } else {
                argreduce_small_inner<false><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, (unsigned)axis_len, (unsigned)inner, (unsigned)rows_per_block);
            }
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
        const size_t wg_per_cu = g_arg_cols_wg_per_cu > 0 ? (size_t)g_arg_cols_wg_per_cu : (rows_aligned ? 2 : 8);
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
            const unsigned xcd_runs = (!rows_are_lines && tiles > 1 && tiles * chunks * outer < (size_t(1) << 31) && !g_arg_xcd_runs_off) ? 1u : 0u;
            if (chunks == 1) {
                if (is_max)
                    argreduce_cols_tile<true, true><<<grid, 256, 0, s>>>(in, nullptr, nullptr, out, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
                else
                    argreduce_cols_tile<false, true><<<grid, 256, 0, s>>>(in, nullptr, nullptr, out, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
                NP_LAUNCH_CHECK("argreduce_cols_tile");
                return NP_OK;
            }
            np::Scratch pv, pi;
            if (int rc = pv.alloc(total * chunks * sizeof(float))) return rc;
            if (int rc = pi.alloc(total * chunks * sizeof(unsigned))) return rc;
            if (is_max)
                argreduce_cols_tile<true, false><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, nullptr, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
            else
                argreduce_cols_tile<false, false><<<grid, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, nullptr, (unsigned)axis_len, (unsigned)inner, (unsigned)chunk_len, xcd_runs);
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
            if (is_max)
                argreduce_chunks_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, outer, (unsigned)axis_len, inner, (unsigned)chunks, (unsigned)chunk_len);
            else
                argreduce_chunks_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)pv.ptr, (unsigned *)pi.ptr, outer, (unsigned)axis_len, inner, (unsigned)chunks, (unsigned)chunk_len);
            NP_LAUNCH_CHECK("argreduce_chunks_kernel");
            return launch_arg_fold(is_max, (const float *)pv.ptr, (const unsigned *)pi.ptr, out, total, chunks, inner);
        }
    }
    size_t blocks = (total + 255) / 256;
    const size_t cap = (size_t)np::num_cus() * 16;
    if (blocks > cap) blocks = cap;
    if (is_max)
        argreduce_generic_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len, inner);
    else
        argreduce_generic_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(in, out, outer, (unsigned)axis_len, inner);
    NP_LAUNCH_CHECK("argreduce_generic_kernel");
    return NP_OK;
}

int np_moments_dev(const float *in, size_t n, float *dev_out) {
    if (!dev_out) return np::fail(NP_ERR_INVALID, "np_moments: null output");
    if (n == 0 || !in) return np::fail(NP_ERR_INVALID, "np_moments: empty input");
    if (int rc = np::ensure_init()) return rc;
    if (n < (size_t(1) << 31)) return launch_moments<uint32_t>(in, n, dev_out);
    return launch_moments<uint64_t>(in, n, dev_out);
}

int np_moments(const float *in, size_t n, float *host_mean, float *host_m2) {
    if (!host_mean || !host_m2) return np::fail(NP_ERR_INVALID, "np_moments: null output");
    if (n == 0 || !in) return np::fail(NP_ERR_INVALID, "np_moments: empty input");
    if (int rc = np::ensure_init()) return rc;
    // ONE read of the array, one host wait (until round 6: np_reduce_all for the mean, the host's division, a second pass)
    np::ResultCall call(2);
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    if (int rc = np_moments_dev(in, n, slot)) return rc;
    if (int rc = call.wait()) return rc;
    *host_mean = slot[0];
    *host_m2 = slot[1];
    return NP_OK;
}

int np_weighted_sums(const float *a, const float *w, size_t n, float *host_sum_aw, float *host_sum_w) {
    if (!host_sum_aw || !host_sum_w) return np::fail(NP_ERR_INVALID, "np_weighted_sums: null output");
    if (n == 0 || !a || !w) return np::fail(NP_ERR_INVALID, "np_weighted_sums: empty input");
    if (int rc = np::ensure_init()) return rc;
    np::ResultCall call(2);
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    // one kernel carrying both sums: a and w are read once each (8 B/elem; until round 6 w was read a second time)
    if (n < (size_t(1) << 31)) {
        if (int rc = launch_weighted_sums<uint32_t>(a, w, n, slot)) return rc;
    } else {
        if (int rc = launch_weighted_sums<uint64_t>(a, w, n, slot)) return rc;
    }
    if (int rc = call.wait()) return rc;
    *host_sum_aw = slot[0];
    *host_sum_w = slot[1];
    return NP_OK;
}

int np_count_mismatch(int mode, const float *a, const float *b, size_t n, float rtol, float atol,
                      int *host_any) {
    if (!host_any) return np::fail(NP_ERR_INVALID, "np_count_mismatch: null output");
    *host_any = 0;
    if (mode != NP_MISMATCH_EXACT && mode != NP_MISMATCH_ALLCLOSE)
        return np::fail(NP_ERR_INVALID, "np_count_mismatch: unknown mode %d", mode);
    if (n == 0) return NP_OK;
    if (!a || !b) return np::fail(NP_ERR_INVALID, "np_count_mismatch: null input");
    if (int rc = np::ensure_init()) return rc;
    np::ResultCall call;
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    // a sum of 0/1 terms: inexact above 2^24 but zero exactly when every term is zero
    if (mode == NP_MISMATCH_EXACT) {
        if (int rc = xform_sum<3>(a, b, n, 0.0f, 0.0f, slot)) return rc;
    } else {
        if (int rc = xform_sum<4>(a, b, n, rtol, atol, slot)) return rc;
    }
    if (int rc = call.wait()) return rc;
    *host_any = (slot[0] != 0.0f) ? 1 : 0;
    return NP_OK;
}

int np_all(const float *in, size_t n, unsigned flags, int *host_out) {
    if (!host_out) return np::fail(NP_ERR_INVALID, "np_all: null output");
    *host_out = 1;
    if (n == 0) return NP_OK;
    if (!in) return np::fail(NP_ERR_INVALID, "np_all: null input");
    if (int rc = np::ensure_init()) return rc;
    hipStream_t s = np::stream();
    size_t head = ((16 - ((uintptr_t)in & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    const size_t blocks = np::capped_grid((nvec + 255) / 256, stream_cap());
    np::Scratch partials;
    if (int rc = partials.alloc(blocks * sizeof(float))) return rc;
    np::ResultCall call;
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    const size_t body_end = (flags & NP_QUIRK_AVX_BODY) ? np_avx_body_end(n) : 0;
    unsigned *ticket = np::fold_ticket(blocks);
    const bool wide = n >= (size_t(1) << 31);   // 64-bit indices past 2^31 elements
#define NP_ALL_PASS1(Q, I) all_pass1<Q, I><<<(unsigned)blocks, 256, 0, s>>>(in, (float *)partials.ptr, (I)n, (I)head, (I)nvec, (I)body_end, ticket, slot)
    if (flags & NP_QUIRK_AVX_BODY) {
        if (wide) NP_ALL_PASS1(true, uint64_t); else NP_ALL_PASS1(true, uint32_t);
    } else {
        if (wide) NP_ALL_PASS1(false, uint64_t); else NP_ALL_PASS1(false, uint32_t);
    }
#undef NP_ALL_PASS1
    NP_LAUNCH_CHECK("all_pass1");
    if (!ticket) {
        reduce_all_pass2<NP_MIN><<<1, 256, 0, s>>>((const float *)partials.ptr, (int)blocks, slot, 1.0f);
        NP_LAUNCH_CHECK("reduce_all_pass2");
    }
    if (int rc = call.wait()) return rc;
    *host_out = (slot[0] != 0.0f) ? 1 : 0;
    return NP_OK;
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
    if (variant == 4200000 || variant == 4200001) {   // argmax / argmin over wide unaligned rows: tiles dealt to the XCDs in runs (0) or in launch order (1)
        g_arg_xcd_runs_off = variant - 4200000;
        return NP_OK;
    }
    if (variant >= 4100000 && variant < 4100100) {   // argmax / argmin over a few columns (flat walks): workgroups per CU
        g_arg_flat_wg_per_cu = variant - 4100000;   // 0 = the default rule
        return NP_OK;
    }
    if (variant >= 4000000 && variant < 4000100) {   // argmax / argmin over wide inner: workgroups per CU
        g_arg_cols_wg_per_cu = variant - 4000000;   // 0 = the default rule
        return NP_OK;
    }
    if (variant >= 3000000 && variant < 3100000) {   // np_reduce_all of <= 4 M elements on at most N workgroups (0 = off)
        np::g_small_reduce_blocks = (size_t)(variant - 3000000);
        return NP_OK;
    }
    if (variant < 0 || variant > 1000000) return np::fail(NP_ERR_INVALID, "np_reduce_set_variant: workgroups per CU out of range");
    g_wg_per_cu = variant;
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

int np_debug_reduce_last_path(unsigned *host_mask) {
    if (!host_mask) return np::fail(NP_ERR_INVALID, "np_debug_reduce_last_path: null pointer");
    *host_mask = g_last_path;
    return NP_OK;
}

}  // extern "C"
