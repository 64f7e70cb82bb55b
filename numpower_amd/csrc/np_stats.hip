// Scalar statistics and predicates of libnp_hip.so: mean and sum of squared deviations in one read (np_moments), the two sums
// of a weighted average (np_weighted_sums), the mismatch counts behind array_equal / allclose (np_count_mismatch) and all()
// (np_all).  Each is one streaming first pass in the shape of reduce_all_pass1 (np_reduce.hip) with one partial per
// workgroup, folded by the last workgroup to finish or by a one-block second launch (np::fold_partials where a partial is one float).
#include <float.h>
#include <math.h>

#include "np_internal.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_u __attribute__((aligned(4)));   // float4 access that only assumes dword alignment

using namespace np::dev;   // block_reduce / fold_in_last_workgroup / coherent_load ... (np_internal.h)

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
// host side
// ------------------------------------------------------------------------------------------

// mean and sum of squared deviations -> dev_out[0], dev_out[1]: one streaming pass (+ a one-workgroup fold above 256 workgroups)
template <typename I>
int launch_moments(const float *in, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    size_t head = ((16 - ((uintptr_t)in & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 4;
    size_t blocks = np::capped_grid((nvec + 255) / 256, np::stream_cap());
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
int launch_weighted_sums(const float *a, const float *w, size_t n, float *dev_out) {
    hipStream_t s = np::stream();
    const size_t nvec = n / 4;
    const size_t blocks = np::capped_grid((nvec + 255) / 256, np::stream_cap());
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
int xform_sum_as(const float *in, const float *in2, size_t n, float p0, float p1, float *dev_out) {
    hipStream_t s = np::stream();
    const size_t nvec = n / 4;   // dword-aligned float4 loads: views may start anywhere
    const size_t blocks = np::capped_grid((nvec + 255) / 256, np::stream_cap());
    np::Scratch partials;
    if (int rc = partials.alloc(blocks * sizeof(float))) return rc;
    unsigned *ticket = np::fold_ticket(blocks);
    reduce_xform_pass1<XFORM, I><<<(unsigned)blocks, 256, 0, s>>>(in, in2, (float *)partials.ptr, (I)n, (I)nvec, p0, p1, ticket, dev_out);
    NP_LAUNCH_CHECK("reduce_xform");
    if (ticket) return NP_OK;
    return np::fold_partials(NP_SUM, (const float *)partials.ptr, blocks, dev_out);
}

template <int XFORM>
int xform_sum(const float *in, const float *in2, size_t n, float p0, float p1, float *dev_out) {
    if (n < (size_t(1) << 31)) return xform_sum_as<XFORM, uint32_t>(in, in2, n, p0, p1, dev_out);
    return xform_sum_as<XFORM, uint64_t>(in, in2, n, p0, p1, dev_out);
}

}  // namespace

extern "C" {

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
    const size_t blocks = np::capped_grid((nvec + 255) / 256, np::stream_cap());
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
        if (int rc = np::fold_partials(NP_MIN, (const float *)partials.ptr, blocks, slot)) return rc;
    }
    if (int rc = call.wait()) return rc;
    *host_out = (slot[0] != 0.0f) ? 1 : 0;
    return NP_OK;
}

}  // extern "C"
