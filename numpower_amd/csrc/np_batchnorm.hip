// Batch normalization for GPU arrays: np_batchnorm_forward (training and inference) and np_batchnorm_backward.
// The rules are in np_hip.h; this comment says how the kernels keep them.
//
// The operand is (N, C, inner), contiguous fp32; the statistics of channel c run over its n = N.inner values.  Every kernel is
// built from the same pieces, so that a value has the same bits wherever it is computed:
//   channel sums     forward: K = x[0, c, 0], a = sum of (x - K), b = sum of (x - K)^2; backward: a = sum of dy, b = sum of
//                    dy . xh.  All in fp64: the difference and the product of two floats are exact in double, so the only
//                    roundings are those of the additions, far below what the ONE rounding to fp32 can see (the tests carry
//                    the guard that proves it for their data).  The order of the additions is fixed by (N, C, inner) and the
//                    form: per lane in ascending order, lanes by a xor butterfly, waves and slices in ascending order.
//   finish_sums      the per-channel scalars from (a, b): mean, invstd and the running statistics, or dbeta, dgamma, mb, mg.
//   element values   fwd_value / bwd_value below, separately rounded fp32 steps (contraction is off in this unit).
// Special values need no branch: a NaN or an Inf in a channel makes a or b NaN or Inf, then invstd (or mean) NaN, then every
// element of that channel; no sum ever mixes two channels.
//
// Three forms for the passes that need statistics, chosen from (N, C, inner) alone (pick_form), reported by
// np_debug_batchnorm_last_path, and a fourth name for inference:
//   1 ONE     inner > 1, n <= kOneMaxN.  One launch, a workgroup per channel: 256 lanes up to kOneSmallN values, 1024 lanes
//             above, lane t holding the values t, t + L, ... in registers (16 at 256 lanes; 8 at 1024 lanes,
//             where a lane has 128 VGPRs).  The channel is read once, the
//             lanes' sums are joined through LDS in wave order, the outputs are written from the held values: 8 bytes per
//             element forward, 12 backward.
//   2 SPLIT   inner > 1, larger channels.  The n values of a channel are cut into S slices of whole groups of four (plan_of:
//             S from the extents alone).  bn_stats_kernel, a workgroup per (channel, slice), writes a pair of fp64 partials;
//             bn_fold_kernel, a wave per channel, adds them in slice order and finishes the channel; bn_apply_kernel walks the
//             same slices again.  A group of four is one 16-byte access where inner % 4 == 0 (such a group never leaves its
//             plane; the access assumes 4-byte alignment only), four scalar accesses otherwise.  The position inside the plane
//             is carried along and reduced by a multiply-high (FastDiv): no integer division per element.
//   3 ROWS    inner == 1, the (N, C) case.  min(64, C rounded up to a power of two) lanes lie along C, the rest of the 256 along
//             N, so a wave's access is a contiguous run for any C, and a narrow C with a long N still fills the workgroup.  N
//             is cut into S slices the same way; the same fold kernel; bn_rows_apply_kernel.
//   4 APPLY   inference: the apply kernel of form 2 or 3 alone, one launch, invstd = f32(1 / sqrt((double) running_var + eps))
//             formed per channel inside it.
// Three launches at most (np_debug_batchnorm_last_path counts them).  Partials and the backward pass's (mb, mg) pairs live in
// pool scratch that is released on every path.  dx may alias dy: form 1 has read the whole channel before it writes, forms 2 and
// 3 write an element from the lane that read it, after the statistics kernel has ended.
//
// Indexing: C < 2^31 (refused otherwise); every element offset is formed in size_t, so N.C.inner may pass 2^31.  Every kernel
// walks its work items with a grid-stride loop, the grid capped at kMaxGrid workgroups.
#include "np_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_u __attribute__((aligned(4)));   // float4 access that only assumes dword alignment

constexpr unsigned kOneSmallN = 4096;      // form boundaries (np_debug_batchnorm_bounds reports them; tests/batchnorm_family.py restates the dispatcher)
constexpr unsigned kOneMaxN = 8192;
constexpr unsigned kTargetGroups = 2048;   // SPLIT / ROWS: the workgroups the slices aim for
constexpr unsigned kMaxSlices = 1024;
constexpr unsigned kSliceMinSteps = 4;     // a slice holds at least this many steps of a workgroup
constexpr unsigned kOneVals = 16;          // ONE: values a lane holds on 256 lanes; kOneMaxN / 1024 on 1024 lanes
constexpr unsigned kMaxGrid = 1u << 20;
constexpr int kNumBounds = 5;
constexpr size_t kChanLim = (size_t)1 << 31;
constexpr size_t kFastDivMax = (size_t)1 << 30;

enum { FORM_ONE = 1, FORM_SPLIT = 2, FORM_ROWS = 3, FORM_APPLY = 4 };
enum { OP_FWD = 0, OP_INF = 1, OP_BWD = 2 };

int g_bn_last_form = 0;       // np_debug_batchnorm_last_path
int g_bn_last_launches = 0;
size_t g_bn_last_slices = 0;
int g_bn_force_form = -1;     // np_debug_batchnorm_force_form

// n / d for n < 2^31 by a multiply-high (as np_pool.hip)
struct FastDiv {
    unsigned d, mul, shift;
};

FastDiv fast_div(unsigned d) {
    if (d == 1) return {1u, 0u, 0u};
    unsigned log2_up = 0;
    while (((uint64_t)1 << log2_up) < d) ++log2_up;
    const unsigned p = 31 + log2_up;
    return {d, (unsigned)((((uint64_t)1 << p) + d - 1) / d), p - 32};
}

__device__ __forceinline__ unsigned quotient(unsigned n, const FastDiv &f) { return f.d == 1 ? n : __umulhi(n, f.mul) >> f.shift; }

struct BnArgs {
    const float *x, *dy, *gamma, *beta;
    float *out;                        // y | dx
    float *save_mean, *save_invstd;    // written by the training forward pass, read by the backward pass
    float *run_mean, *run_var;         // updated by the training forward pass (may be nullptr), read by inference
    float *dgamma, *dbeta;             // may be nullptr
    double *part;                      // SPLIT / ROWS: [C][S][2]
    float *mbmg;                       // SPLIT / ROWS backward: [C][2]
    size_t N, inner, n;                // n = N.inner
    unsigned C;
    double eps, momentum;
    unsigned S;                        // slices
    size_t per;                        // groups of four (SPLIT) or rows (ROWS) per slice
    unsigned CW;                       // ROWS: lanes along C, a power of two up to 64
    FastDiv by_inner;
    int inner_small;                   // inner <= 2^30: by_inner is valid
    int vec;                           // inner % 4 == 0: a group of four is contiguous
};

// the per-channel scalars an element needs
struct Chan {
    float mean, invstd, g, b, mb, mg;
};

// ---- element values: every form writes through these ----
__device__ __forceinline__ float fwd_value(float x, const Chan &ch, bool has_g, bool has_b) {
    const float d = x - ch.mean;
    float h = d * ch.invstd;
    if (has_g) h = h * ch.g;
    if (has_b) h = h + ch.b;
    return h;
}
__device__ __forceinline__ float xhat(float x, const Chan &ch) {
    const float d = x - ch.mean;
    return d * ch.invstd;
}
// k = gamma . invstd, or invstd without a gamma
__device__ __forceinline__ float bwd_value(float x, float dy, const Chan &ch, float k) {
    const float xh = xhat(x, ch);
    return k * ((dy - ch.mb) - xh * ch.mg);
}
__device__ __forceinline__ float bwd_scale(const Chan &ch, bool has_g) { return has_g ? ch.g * ch.invstd : ch.invstd; }

// one element's terms of the channel sums; K: the shift (forward)
template <int OP>
__device__ __forceinline__ void add_terms(float x, float dy, double K, const Chan &ch, double &a, double &b) {
    if (OP == OP_FWD) {
        const double d = (double)x - K;
        a += d;
        b += d * d;
    } else {
        a += (double)dy;
        b += (double)dy * (double)xhat(x, ch);
    }
}

// the channel's scalars from its sums.  Every lane may call it; `write` is true in the one lane that stores.
// forward: o1 = save_mean, o2 = save_invstd; backward: o1 = mb, o2 = mg
template <int OP>
__device__ __forceinline__ void finish_sums(const BnArgs &g, unsigned c, double K, double a, double b, bool write, float &o1, float &o2) {
    const double n = (double)g.n;
    if (OP == OP_FWD) {
        const double m1 = a / n;
        const double mean64 = K + m1;
        const double var64 = b / n - m1 * m1;
        o1 = (float)mean64;
        o2 = (float)(1.0 / sqrt(var64 + g.eps));
        if (write) {
            g.save_mean[c] = o1;
            g.save_invstd[c] = o2;
            if (g.run_mean) g.run_mean[c] = (float)((1.0 - g.momentum) * (double)g.run_mean[c] + g.momentum * mean64);
            if (g.run_var) g.run_var[c] = (float)((1.0 - g.momentum) * (double)g.run_var[c] + g.momentum * (var64 * n / (n - 1.0)));
        }
    } else {
        o1 = (float)(a / n);
        o2 = (float)(b / n);
        if (write) {
            if (g.dbeta) g.dbeta[c] = (float)a;
            if (g.dgamma) g.dgamma[c] = (float)b;
        }
    }
}

template <int OP>
__device__ __forceinline__ Chan chan_of(const BnArgs &g, unsigned c) {
    Chan ch;
    if (OP == OP_INF) {
        ch.mean = g.run_mean[c];
        ch.invstd = (float)(1.0 / sqrt((double)g.run_var[c] + g.eps));
    } else {
        ch.mean = g.save_mean[c];
        ch.invstd = g.save_invstd[c];
    }
    ch.g = g.gamma ? g.gamma[c] : 1.0f;
    ch.b = g.beta ? g.beta[c] : 0.0f;
    ch.mb = OP == OP_BWD ? g.mbmg[2 * (size_t)c] : 0.0f;
    ch.mg = OP == OP_BWD ? g.mbmg[2 * (size_t)c + 1] : 0.0f;
    return ch;
}

// ---- joins: all lanes of the workgroup (WAVES waves) get the same bits; part: 2 . WAVES doubles of LDS ----
__device__ __forceinline__ void wave_sum2(double &a, double &b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
}
template <int WAVES>
__device__ __forceinline__ void group_sum2(double &a, double &b, double *part) {
    wave_sum2(a, b);
    __syncthreads();   // the previous join's readers are done with part
    if ((threadIdx.x & 63) == 0) part[2 * (threadIdx.x >> 6)] = a, part[2 * (threadIdx.x >> 6) + 1] = b;
    __syncthreads();
    a = part[0], b = part[1];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) a += part[2 * w], b += part[2 * w + 1];
}

// ---- ONE: a workgroup per channel, the channel in registers ----
template <int OP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void bn_one_kernel(const BnArgs g) {
    __shared__ double part[2 * WAVES];
    constexpr unsigned L = WAVES * 64, NV = WAVES == 4 ? kOneVals : kOneMaxN / 1024;
    static_assert(NV * L == (WAVES == 4 ? kOneSmallN : kOneMaxN), "the lanes hold the largest channel of their form");
    const unsigned n = (unsigned)g.n, inner = (unsigned)g.inner;
    const bool has_g = g.gamma != nullptr, has_b = g.beta != nullptr;
    for (unsigned c = blockIdx.x; c < g.C; c += gridDim.x) {
        Chan ch = {0.0f, 0.0f, has_g ? g.gamma[c] : 1.0f, has_b ? g.beta[c] : 0.0f, 0.0f, 0.0f};
        double K = 0.0;
        if (OP == OP_FWD) K = (double)g.x[(size_t)c * inner];
        else ch.mean = g.save_mean[c], ch.invstd = g.save_invstd[c];
        float xv[NV], dv[NV];
#pragma unroll
        for (unsigned k = 0; k < NV; ++k) {
            const unsigned j = k * L + threadIdx.x;
            xv[k] = 0.0f, dv[k] = 0.0f;
            if (j < n) {
                const unsigned ni = quotient(j, g.by_inner);
                const size_t off = ((size_t)ni * g.C + c) * inner + (j - ni * inner);
                xv[k] = g.x[off];
                if (OP == OP_BWD) dv[k] = g.dy[off];
            }
        }
        double a = 0.0, b = 0.0;
#pragma unroll
        for (unsigned k = 0; k < NV; ++k)
            if (k * L + threadIdx.x < n) add_terms<OP>(xv[k], dv[k], K, ch, a, b);
        group_sum2<WAVES>(a, b, part);
        float o1, o2;
        finish_sums<OP>(g, c, K, a, b, threadIdx.x == 0, o1, o2);
        if (OP == OP_FWD) ch.mean = o1, ch.invstd = o2;
        else ch.mb = o1, ch.mg = o2;
        const float k_dx = bwd_scale(ch, has_g);
#pragma unroll
        for (unsigned k = 0; k < NV; ++k) {
            const unsigned j = k * L + threadIdx.x;
            if (j < n) {
                const unsigned ni = quotient(j, g.by_inner);
                const size_t off = ((size_t)ni * g.C + c) * inner + (j - ni * inner);
                g.out[off] = OP == OP_FWD ? fwd_value(xv[k], ch, has_g, has_b) : bwd_value(xv[k], dv[k], ch, k_dx);
            }
        }
    }
}

// ---- SPLIT: slices of whole groups of four along a channel's n values ----
__device__ __forceinline__ void advance(const BnArgs &g, size_t &ni, size_t &i, unsigned step) {
    i += step;
    if (g.inner_small) {
        const unsigned q = quotient((unsigned)i, g.by_inner);   // i < inner + step < 2^31
        ni += q;
        i -= (size_t)q * g.inner;
    } else {
        while (i >= g.inner) i -= g.inner, ++ni;
    }
}

// slice s of channel c: f(off, 4) for four contiguous elements at off, f(off, 1) for one
template <class F>
__device__ __forceinline__ void walk_slice(const BnArgs &g, unsigned c, unsigned s, F f) {
    const size_t groups = (g.n + 3) / 4, q0 = (size_t)s * g.per, q1 = q0 + g.per < groups ? q0 + g.per : groups;
    size_t ni = (q0 * 4) / g.inner, i = q0 * 4 - ni * g.inner;   // the slice's first element: once per workgroup
    advance(g, ni, i, threadIdx.x * 4);
    for (size_t q = q0 + threadIdx.x; q < q1; q += 256) {
        if (g.vec) {
            f((ni * g.C + c) * g.inner + i, 4);
        } else {
            size_t nn = ni, ii = i;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (q * 4 + e < g.n) f((nn * g.C + c) * g.inner + ii, 1);
                if (++ii == g.inner) ii = 0, ++nn;
            }
        }
        advance(g, ni, i, 1024);
    }
}

template <int OP>
__global__ __launch_bounds__(256) void bn_stats_kernel(const BnArgs g) {
    __shared__ double part[8];
    const size_t items = (size_t)g.C * g.S;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned c = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)c * g.S);
        Chan ch = {};
        double K = 0.0;
        if (OP == OP_FWD) K = (double)g.x[(size_t)c * g.inner];
        else ch.mean = g.save_mean[c], ch.invstd = g.save_invstd[c];
        double a = 0.0, b = 0.0;
        walk_slice(g, c, s, [&](size_t off, int cnt) {
            if (cnt == 4) {
                const v4f xv = *(const v4f_u *)(g.x + off);
                v4f dv = {0.0f, 0.0f, 0.0f, 0.0f};
                if (OP == OP_BWD) dv = *(const v4f_u *)(g.dy + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) add_terms<OP>(xv[e], dv[e], K, ch, a, b);
            } else {
                add_terms<OP>(g.x[off], OP == OP_BWD ? g.dy[off] : 0.0f, K, ch, a, b);
            }
        });
        group_sum2<4>(a, b, part);
        if (threadIdx.x == 0) g.part[2 * w] = a, g.part[2 * w + 1] = b;
    }
}

// a wave per channel: the partials in slice order (lane l takes l, l + 64, ...; then the butterfly), then the channel's scalars
template <int OP>
__global__ __launch_bounds__(64) void bn_fold_kernel(const BnArgs g) {
    for (unsigned c = blockIdx.x; c < g.C; c += gridDim.x) {
        double a = 0.0, b = 0.0;
        for (unsigned s = threadIdx.x; s < g.S; s += 64) {
            const size_t w = (size_t)c * g.S + s;
            a += g.part[2 * w], b += g.part[2 * w + 1];
        }
        wave_sum2(a, b);
        const double K = OP == OP_FWD ? (double)g.x[(size_t)c * g.inner] : 0.0;
        float o1, o2;
        finish_sums<OP>(g, c, K, a, b, threadIdx.x == 0, o1, o2);
        if (OP == OP_BWD && threadIdx.x == 0) g.mbmg[2 * (size_t)c] = o1, g.mbmg[2 * (size_t)c + 1] = o2;
    }
}

template <int OP>
__global__ __launch_bounds__(256) void bn_apply_kernel(const BnArgs g) {
    const size_t items = (size_t)g.C * g.S;
    const bool has_g = g.gamma != nullptr, has_b = g.beta != nullptr;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned c = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)c * g.S);
        const Chan ch = chan_of<OP>(g, c);
        const float k_dx = bwd_scale(ch, has_g);
        walk_slice(g, c, s, [&](size_t off, int cnt) {
            if (cnt == 4) {
                const v4f xv = *(const v4f_u *)(g.x + off);
                v4f r;
                if (OP == OP_BWD) {
                    const v4f dv = *(const v4f_u *)(g.dy + off);
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = bwd_value(xv[e], dv[e], ch, k_dx);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = fwd_value(xv[e], ch, has_g, has_b);
                }
                *(v4f_u *)(g.out + off) = r;
            } else {
                g.out[off] = OP == OP_BWD ? bwd_value(g.x[off], g.dy[off], ch, k_dx) : fwd_value(g.x[off], ch, has_g, has_b);
            }
        });
    }
}

// ---- ROWS: inner == 1.  Lane t: channel lane t % CW, row lane t / CW; a work item is (channel block, slice of rows) ----
template <int OP>
__global__ __launch_bounds__(256) void bn_rows_stats_kernel(const BnArgs g) {
    __shared__ double sh[512];
    const unsigned CW = g.CW, RL = 256 / CW, cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW;
    const size_t items = (size_t)((g.C + CW - 1) / CW) * g.S;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned cb = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)cb * g.S), c = cb * CW + cl;
        const size_t r0 = (size_t)s * g.per, r1 = r0 + g.per < g.N ? r0 + g.per : g.N;
        double a = 0.0, b = 0.0;
        if (c < g.C) {
            Chan ch = {};
            double K = 0.0;
            if (OP == OP_FWD) K = (double)g.x[c];
            else ch.mean = g.save_mean[c], ch.invstd = g.save_invstd[c];
#pragma unroll 4
            for (size_t r = r0 + rl; r < r1; r += RL) {
                const size_t off = r * g.C + c;
                add_terms<OP>(g.x[off], OP == OP_BWD ? g.dy[off] : 0.0f, K, ch, a, b);
            }
        }
        __syncthreads();   // the previous item's readers are done with sh
        sh[2 * threadIdx.x] = a, sh[2 * threadIdx.x + 1] = b;
        for (unsigned half = RL / 2; half > 0; half /= 2) {      // the row lanes, a tree: lane rl takes rl + half
            __syncthreads();
            if (rl < half) {
                a += sh[2 * (threadIdx.x + half * CW)], b += sh[2 * (threadIdx.x + half * CW) + 1];
                sh[2 * threadIdx.x] = a, sh[2 * threadIdx.x + 1] = b;
            }
        }
        if (rl == 0 && c < g.C) {
            const size_t at = (size_t)c * g.S + s;
            g.part[2 * at] = a, g.part[2 * at + 1] = b;
        }
    }
}

template <int OP>
__global__ __launch_bounds__(256) void bn_rows_apply_kernel(const BnArgs g) {
    const unsigned CW = g.CW, RL = 256 / CW, cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW;
    const size_t items = (size_t)((g.C + CW - 1) / CW) * g.S;
    const bool has_g = g.gamma != nullptr, has_b = g.beta != nullptr;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned cb = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)cb * g.S), c = cb * CW + cl;
        if (c >= g.C) continue;   // no barrier in this kernel
        const size_t r0 = (size_t)s * g.per, r1 = r0 + g.per < g.N ? r0 + g.per : g.N;
        const Chan ch = chan_of<OP>(g, c);
        const float k_dx = bwd_scale(ch, has_g);
#pragma unroll 4
        for (size_t r = r0 + rl; r < r1; r += RL) {
            const size_t off = r * g.C + c;
            g.out[off] = OP == OP_BWD ? bwd_value(g.x[off], g.dy[off], ch, k_dx) : fwd_value(g.x[off], ch, has_g, has_b);
        }
    }
}

// ---- host ----
bool serves(int form, size_t n, size_t inner) {
    switch (form) {
    case FORM_ONE: return n <= kOneMaxN;
    case FORM_SPLIT: return true;
    case FORM_ROWS: return inner == 1;
    default: return false;
    }
}

// the form comes from (N, inner) alone, and from the A-B switch
int pick_form(const char *who, size_t N, size_t inner, int &form) {
    const size_t n = N * inner;
    form = inner == 1 ? FORM_ROWS : n <= kOneMaxN ? FORM_ONE : FORM_SPLIT;
    if (g_bn_force_form < 0) return NP_OK;
    if (!serves(g_bn_force_form, n, inner))
        return np::fail(NP_ERR_INVALID, "%s: the forced form %d cannot serve N = %zu, inner = %zu", who, g_bn_force_form, N, inner);
    form = g_bn_force_form;
    return NP_OK;
}

size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// the slices of SPLIT and ROWS, from the extents alone: units of work (groups of four, or rows) cut so that a slice holds at
// least kSliceMinSteps steps of a workgroup, the grid aims at kTargetGroups workgroups, and S <= kMaxSlices
void plan_of(int form, BnArgs &g) {
    g.CW = 1;
    size_t units, per_step, blocks;
    if (form == FORM_ROWS) {
        while (g.CW < 64 && g.CW < g.C) g.CW *= 2;
        units = g.N, per_step = 256 / g.CW, blocks = ceil_div(g.C, g.CW);
    } else {
        units = ceil_div(g.n, 4), per_step = 256, blocks = g.C;
    }
    const size_t steps = ceil_div(units, per_step);
    size_t S = steps / kSliceMinSteps;
    if (S > kTargetGroups / blocks) S = kTargetGroups / blocks;
    if (S > kMaxSlices) S = kMaxSlices;
    if (S < 1) S = 1;
    g.per = ceil_div(units, S);
    g.S = (unsigned)ceil_div(units, g.per);
}

unsigned grid_of(size_t blocks) { return (unsigned)(blocks < kMaxGrid ? (blocks < 1 ? 1 : blocks) : kMaxGrid); }

// OP_FWD and OP_BWD in the form given; OP_INF: the apply kernel of `form`'s geometry alone
template <int OP>
int launch(int form, BnArgs &g) {
    g.inner_small = g.inner <= kFastDivMax;
    g.by_inner = fast_div(g.inner_small ? (unsigned)g.inner : 1u);
    g.vec = g.inner % 4 == 0;
    g.S = 0;
    int launches = 0;
    if (OP != OP_INF && form == FORM_ONE) {
        if (g.n <= kOneSmallN) bn_one_kernel<OP, 4><<<grid_of(g.C), 256, 0, np::stream()>>>(g);
        else bn_one_kernel<OP, 16><<<grid_of(g.C), 1024, 0, np::stream()>>>(g);
        NP_LAUNCH_CHECK("bn_one_kernel");
        launches = 1;
    } else {
        const bool rows = form == FORM_ROWS;
        plan_of(form, g);
        const size_t items = (rows ? ceil_div(g.C, g.CW) : (size_t)g.C) * g.S;
        np::Scratch part, mbmg;   // released on every path below
        if (OP != OP_INF) {
            if (int rc = part.alloc(2 * (size_t)g.C * g.S * sizeof(double))) return rc;
            g.part = (double *)part.ptr;
            if (OP == OP_BWD) {
                if (int rc = mbmg.alloc(2 * (size_t)g.C * sizeof(float))) return rc;
                g.mbmg = (float *)mbmg.ptr;
            }
            constexpr int SOP = OP == OP_INF ? OP_FWD : OP;
            if (rows) bn_rows_stats_kernel<SOP><<<grid_of(items), 256, 0, np::stream()>>>(g);
            else bn_stats_kernel<SOP><<<grid_of(items), 256, 0, np::stream()>>>(g);
            NP_LAUNCH_CHECK("bn_stats_kernel");
            bn_fold_kernel<SOP><<<grid_of(g.C), 64, 0, np::stream()>>>(g);
            NP_LAUNCH_CHECK("bn_fold_kernel");
            launches = 2;
        }
        if (rows) bn_rows_apply_kernel<OP><<<grid_of(items), 256, 0, np::stream()>>>(g);
        else bn_apply_kernel<OP><<<grid_of(items), 256, 0, np::stream()>>>(g);
        NP_LAUNCH_CHECK("bn_apply_kernel");
        ++launches;
    }
    g_bn_last_form = OP == OP_INF ? FORM_APPLY : form;
    g_bn_last_launches = launches;
    g_bn_last_slices = g.S;
    return NP_OK;
}

// the extents of a call; numel is written when they are accepted.  No device is touched.
int check_extents(const char *who, size_t N, size_t C, size_t inner, size_t &numel) {
    if (N < 1 || C < 1 || inner < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (C >= kChanLim) return np::fail(NP_ERR_INVALID, "%s: C = %zu is 2^31 or more", who, C);
    const size_t lim = SIZE_MAX / sizeof(float);
    if (N > lim / C || N * C > lim / inner) return np::fail(NP_ERR_INVALID, "%s: N.C.inner does not fit a size_t", who);
    numel = N * C * inner;
    return NP_OK;
}

struct Range {
    const void *p;
    size_t count;   // floats; p == nullptr: absent
};

bool overlap(const Range &a, const Range &b) {
    if (!a.p || !b.p) return false;
    const uintptr_t p = (uintptr_t)a.p, q = (uintptr_t)b.p;
    return p < q + b.count * sizeof(float) && q < p + a.count * sizeof(float);
}

// true when an output overlaps an input or another output
bool any_overlap(const Range *out, int n_out, const Range *in, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (overlap(out[i], in[j])) return true;
        for (int j = i + 1; j < n_out; ++j)
            if (overlap(out[i], out[j])) return true;
    }
    return false;
}

}  // namespace

extern "C" {

// The order is the pointers, the extents, the parameters, the aliasing, the form, ensure_init, then work: a refused call has touched no device.
int np_batchnorm_forward(const float *x, const float *gamma, const float *beta, size_t N, size_t C, size_t inner, int training, double momentum,
                         double eps, float *running_mean, float *running_var, float *y, float *save_mean, float *save_invstd) {
    const char *who = "np_batchnorm_forward";
    if (!x || !y) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    if (training && (!save_mean || !save_invstd)) return np::fail(NP_ERR_INVALID, "%s: null pointer (training saves the mean and invstd)", who);
    if (!training && (!running_mean || !running_var)) return np::fail(NP_ERR_INVALID, "%s: null pointer (inference needs both running statistics)", who);
    size_t numel = 0;
    if (int rc = check_extents(who, N, C, inner, numel)) return rc;
    if (!(eps >= 0.0)) return np::fail(NP_ERR_INVALID, "%s: eps must not be negative", who);
    if (training && !(momentum >= 0.0 && momentum <= 1.0)) return np::fail(NP_ERR_INVALID, "%s: momentum must lie in [0, 1]", who);
    if (training && N * inner == 1) return np::fail(NP_ERR_INVALID, "%s: training needs more than one value per channel", who);
    const Range in[] = {{x, numel}, {gamma, C}, {beta, C}, {training ? nullptr : running_mean, C}, {training ? nullptr : running_var, C}};
    const Range out[] = {{y, numel}, {training ? save_mean : nullptr, C}, {training ? save_invstd : nullptr, C}, {training ? running_mean : nullptr, C},
                         {training ? running_var : nullptr, C}};
    if (any_overlap(out, 5, in, 5)) return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output", who);
    int form = 0;
    if (int rc = pick_form(who, N, inner, form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    BnArgs g = {};
    g.x = x, g.gamma = gamma, g.beta = beta, g.out = y, g.save_mean = save_mean, g.save_invstd = save_invstd;
    g.run_mean = running_mean, g.run_var = running_var;
    g.N = N, g.inner = inner, g.n = N * inner, g.C = (unsigned)C, g.eps = eps, g.momentum = momentum;
    if (training) return launch<OP_FWD>(form, g);
    return launch<OP_INF>(form == FORM_ONE ? FORM_SPLIT : form, g);
}

int np_batchnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd, size_t N, size_t C,
                          size_t inner, float *dx, float *dgamma, float *dbeta) {
    const char *who = "np_batchnorm_backward";
    if (!x || !dy || !save_mean || !save_invstd || !dx) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    size_t numel = 0;
    if (int rc = check_extents(who, N, C, inner, numel)) return rc;
    const Range in[] = {{x, numel}, {dx == dy ? nullptr : dy, numel}, {gamma, C}, {save_mean, C}, {save_invstd, C}};
    const Range out[] = {{dx, numel}, {dgamma, C}, {dbeta, C}};
    if (any_overlap(out, 3, in, 5) || overlap({dy, numel}, {dgamma, C}) || overlap({dy, numel}, {dbeta, C}))
        return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output (dx == dy is allowed)", who);
    int form = 0;
    if (int rc = pick_form(who, N, inner, form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    BnArgs g = {};
    g.x = x, g.dy = dy, g.gamma = gamma, g.out = dx, g.save_mean = (float *)save_mean, g.save_invstd = (float *)save_invstd;
    g.dgamma = dgamma, g.dbeta = dbeta;
    g.N = N, g.inner = inner, g.n = N * inner, g.C = (unsigned)C;
    return launch<OP_BWD>(form, g);
}

int np_debug_batchnorm_last_path(int *form, int *launches, size_t *slices) {
    if (!form || !launches || !slices) return np::fail(NP_ERR_INVALID, "np_debug_batchnorm_last_path: null pointer");
    *form = g_bn_last_form, *launches = g_bn_last_launches, *slices = g_bn_last_slices;
    return NP_OK;
}

int np_debug_batchnorm_force_form(int form) {
    if (form != -1 && (form < FORM_ONE || form > FORM_ROWS))
        return np::fail(NP_ERR_INVALID, "np_debug_batchnorm_force_form: form must be -1 (by the extents) or 1 .. 3");
    g_bn_force_form = form;
    return NP_OK;
}

int np_debug_batchnorm_bounds(size_t bounds[], int n) {
    if (!bounds) return np::fail(NP_ERR_INVALID, "np_debug_batchnorm_bounds: null pointer");
    if (n < kNumBounds) return np::fail(NP_ERR_INVALID, "np_debug_batchnorm_bounds: room for %d values is needed", kNumBounds);
    bounds[0] = kOneSmallN, bounds[1] = kOneMaxN, bounds[2] = kTargetGroups, bounds[3] = kMaxSlices, bounds[4] = kSliceMinSteps;
    return NP_OK;
}

}  // extern "C"
