// Layer and group normalization for GPU arrays: np_groupnorm_forward and np_groupnorm_backward.
// The rules are in np_hip.h; this comment says how the kernels keep them.
//
// The operand is (N, G, D, inner), contiguous fp32: M = N.G rows of L = D.inner contiguous floats, P = G.D affine parameters,
// element j of row r using parameter (r mod G).D + j / inner.  Every kernel is built from the same pieces, so that a value has the
// same bits wherever it is computed:
//   row sums         forward: K = x[r, 0], a = sum of (x - K), b = sum of (x - K)^2; backward: g = f32(dy . gamma[p]), a = sum of g,
//                    b = sum of g . xh.  All in fp64 from +0.0 (differences and products of two floats are exact in double).  The
//                    order of the additions is fixed by (N, G, D, inner) and the form: per lane in ascending order, lanes by a
//                    xor butterfly (confined to the row's lanes), waves and slices in ascending order.
//   finish_row       the per-row scalars from (a, b): mean and invstd, or mb and mg.
//   element values   fwd_value / bwd_value below, separately rounded fp32 steps (contraction is off in this unit).
// Special values need no branch: a NaN or an Inf in a row makes a or b NaN or Inf, then invstd (or mean) NaN, then every element
// of that row; no row sum ever mixes two rows.
//
// Four forms for the row passes (forward, dx), chosen from L alone (pick_row_form), reported by np_debug_groupnorm_last_path:
//   1 SHORT   L <= kShortMaxL.  A row takes W = L rounded up to a power of two lanes, a lane holds one value, a wave holds 64 / W
//             rows; the butterfly runs over the offsets below W only.  One launch.
//   2 WAVE    L <= kWaveMaxL.  A wave per row, four waves to a workgroup.  Lane t holds the groups of four t, t + 64, ... (1, 2 or
//             4 groups by L) in registers: one read, one write.  A group of four is one 16-byte access where L % 4 == 0 (every
//             row then starts a multiple of four floats from the base; the access assumes 4-byte alignment only) and four scalar
//             accesses of the same elements otherwise, so the bits do not depend on it.  One launch.
//   3 GROUP   L <= kGroupMaxL.  A workgroup per row: 256 lanes with 2 or 4 groups of four up to kGroupSmallL, 1024 lanes with 2
//             groups above.  The waves' sums are joined through LDS in wave order.  One launch.
//   4 SPLIT   longer rows (and any row when forced).  The groups of four of a row are cut into S slices (plan_rows: S from the
//             extents alone).  gn_stats_kernel, a workgroup per (row, slice), writes a pair of fp64 partials; gn_fold_kernel, a
//             wave per row, adds them in slice order and finishes the row; gn_apply_kernel walks the same slices again.  Three
//             launches.
// The parameter index is needed only with a gamma or a beta.  It is formed once per group of four by a multiply-high (FastDiv) or
// carried along the walk (SPLIT), and stepped inside the group: no integer division per element.
//
// The parameter gradients are a reduction over (N, P, inner) whose xh takes the saved statistics of row n.G + p / D: two forms,
// chosen from inner alone, two launches (none when dgamma and dbeta are both NULL), run BEFORE the row pass so that dx may alias dy:
//   1 COLUMNS inner == 1.  min(64, P rounded up to a power of two) lanes lie along P, the rest of the 256 along N; N is cut into
//             slices.
//   2 PLANES  inner > 1 (and inner == 1 when forced).  A workgroup per (parameter, slice) over the n = N.inner values of the
//             parameter in groups of four.
// Both write fp64 partials; gn_param_fold_kernel, a wave per parameter, adds them in slice order.
// Partials and the backward pass's (mb, mg) pairs live in pool scratch that is released on every path.
//
// Indexing: M < 2^31 and P < 2^31 (refused otherwise); every element offset is formed in size_t.  Every kernel walks its work
// items with a grid-stride loop, the grid capped at kMaxGrid workgroups.
#include "np_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_u __attribute__((aligned(4)));   // float4 access that only assumes dword alignment

constexpr unsigned kShortMaxL = 32;        // form boundaries (np_debug_groupnorm_bounds reports them; tests/groupnorm_family.py restates the dispatcher)
constexpr unsigned kWaveMaxL = 1024;
constexpr unsigned kGroupSmallL = 4096;
constexpr unsigned kGroupMaxL = 8192;
constexpr unsigned kTargetGroups = 2048;   // SPLIT / the parameter forms: the workgroups the slices aim for
constexpr unsigned kMaxSlices = 1024;
constexpr unsigned kSliceMinSteps = 4;     // a slice holds at least this many steps of a workgroup
constexpr unsigned kMaxGrid = 1u << 20;
constexpr int kNumBounds = 7;
constexpr size_t kIndexLim = (size_t)1 << 31;
constexpr size_t kFastDivMax = (size_t)1 << 30;

enum { ROW_SHORT = 1, ROW_WAVE = 2, ROW_GROUP = 3, ROW_SPLIT = 4 };
enum { PARAM_COLUMNS = 1, PARAM_PLANES = 2 };
enum { OP_FWD = 0, OP_BWD = 1 };

int g_gn_last_row_form = 0;   // np_debug_groupnorm_last_path
int g_gn_last_param_form = 0;
int g_gn_last_launches = 0;
size_t g_gn_last_row_slices = 0;
size_t g_gn_last_param_slices = 0;
int g_gn_force_row = -1;      // np_debug_groupnorm_force_form
int g_gn_force_param = -1;

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

struct GnArgs {
    const float *x, *dy, *gamma, *beta;
    float *out;                        // y | dx
    float *save_mean, *save_invstd;    // [M]: written by the forward pass, read by the backward pass
    float *dgamma, *dbeta;             // [P], may be nullptr
    double *part;                      // SPLIT: [M][S][2]
    float *mbmg;                       // SPLIT backward: [M][2]
    double *ppart;                     // the parameter reduction: [P][PS][2]
    size_t N, inner, L, n;             // L = D.inner; n = N.inner, the values of one parameter
    unsigned M, G, D, P;
    double eps;
    unsigned W, Wlog;                  // SHORT: lanes per row, a power of two up to 32, and its log2
    unsigned S;                        // SPLIT: slices per row
    size_t per;                        // SPLIT: groups of four per slice
    unsigned PS;                       // the parameter reduction: slices
    size_t pper;                       // groups of four (PLANES) or rows (COLUMNS) per slice
    unsigned CW;                       // COLUMNS: lanes along P, a power of two up to 64
    FastDiv by_inner, by_G, by_D;
    int inner_small;                   // inner <= 2^30: by_inner is valid
    int vec;                           // L % 4 == 0: a group of four of a row is one access
    int pvec;                          // inner % 4 == 0: a group of four of a parameter's values is contiguous
};

// the per-row scalars an element needs
struct Row {
    float mean, invstd, mb, mg;
};

// ---- element values: every form writes through these ----
__device__ __forceinline__ float xhat(float x, const Row &rw) {
    const float d = x - rw.mean;
    return d * rw.invstd;
}
__device__ __forceinline__ float fwd_value(float x, const Row &rw, const GnArgs &g, unsigned p) {
    float h = xhat(x, rw);
    if (g.gamma) h = h * g.gamma[p];
    if (g.beta) h = h + g.beta[p];
    return h;
}
// gd = f32(dy . gamma[p]), or dy without a gamma
__device__ __forceinline__ float bwd_value(float x, float gd, const Row &rw) {
    const float xh = xhat(x, rw);
    return rw.invstd * ((gd - rw.mb) - xh * rw.mg);
}

// one element's terms of the row sums; K: the shift (forward); v: dy . gamma (backward)
template <int OP>
__device__ __forceinline__ void add_terms(float x, float v, double K, const Row &rw, double &a, double &b) {
    if (OP == OP_FWD) {
        const double d = (double)x - K;
        a += d;
        b += d * d;
    } else {
        a += (double)v;
        b += (double)v * (double)xhat(x, rw);
    }
}

// the row's scalars from its sums: forward (mean, invstd), backward (mb, mg)
template <int OP>
__device__ __forceinline__ void finish_row(const GnArgs &g, double K, double a, double b, float &o1, float &o2) {
    const double n = (double)g.L;
    if (OP == OP_FWD) {
        const double m1 = a / n;
        const double mean64 = K + m1;
        const double var64 = b / n - m1 * m1;
        o1 = (float)mean64;
        o2 = (float)(1.0 / sqrt(var64 + g.eps));
    } else {
        o1 = (float)(a / n);
        o2 = (float)(b / n);
    }
}

// does the pass need the parameter index?
template <int OP>
__device__ __forceinline__ bool needs_param(const GnArgs &g) {
    return OP == OP_FWD ? (g.gamma != nullptr || g.beta != nullptr) : g.gamma != nullptr;
}

// the first parameter of row r
__device__ __forceinline__ unsigned row_param0(const GnArgs &g, unsigned r) { return (r - quotient(r, g.by_G) * g.G) * g.D; }

// ---- joins ----
__device__ __forceinline__ void wave_sum2(double &a, double &b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
}
// all lanes of the workgroup (WAVES waves) get the same bits; part: 2 . WAVES doubles of LDS
template <int WAVES>
__device__ __forceinline__ void group_sum2(double &a, double &b, double *part) {
    wave_sum2(a, b);
    if (WAVES == 1) return;
    __syncthreads();   // the previous join's readers are done with part
    if ((threadIdx.x & 63) == 0) part[2 * (threadIdx.x >> 6)] = a, part[2 * (threadIdx.x >> 6) + 1] = b;
    __syncthreads();
    a = part[0], b = part[1];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) a += part[2 * w], b += part[2 * w + 1];
}

// ---- SHORT: W lanes per row, one value per lane ----
template <int OP>
__global__ __launch_bounds__(256) void gn_short_kernel(const GnArgs g) {
    const unsigned W = g.W, rows_per_wave = 64u >> g.Wlog, lane = threadIdx.x & 63, seg = lane >> g.Wlog, t = lane & (W - 1);
    const unsigned L = (unsigned)g.L;
    const size_t items = ((size_t)g.M + rows_per_wave - 1) / rows_per_wave;
    const bool param = needs_param<OP>(g);
    for (size_t item = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += (size_t)gridDim.x * 4) {
        const size_t r = item * rows_per_wave + seg;
        const bool row_ok = r < g.M, ok = row_ok && t < L;
        const size_t off = r * L + t;
        Row rw = {0.0f, 0.0f, 0.0f, 0.0f};
        double K = 0.0;
        float xv = 0.0f, dv = 0.0f;
        unsigned p = 0;
        if (ok) {
            xv = g.x[off];
            if (param) p = row_param0(g, (unsigned)r) + quotient(t, g.by_inner);
            if (OP == OP_BWD) {
                dv = g.dy[off];
                if (g.gamma) dv = dv * g.gamma[p];
            }
        }
        if (row_ok) {
            if (OP == OP_FWD) K = (double)g.x[r * L];
            else rw.mean = g.save_mean[r], rw.invstd = g.save_invstd[r];
        }
        double a = 0.0, b = 0.0;
        if (ok) add_terms<OP>(xv, dv, K, rw, a, b);
        for (unsigned o = W >> 1; o > 0; o >>= 1) {   // the wave is converged here: the trip counts above are wave-uniform
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        float o1, o2;
        finish_row<OP>(g, K, a, b, o1, o2);
        if (OP == OP_FWD) {
            rw.mean = o1, rw.invstd = o2;
            if (row_ok && t == 0) g.save_mean[r] = o1, g.save_invstd[r] = o2;
        } else {
            rw.mb = o1, rw.mg = o2;
        }
        if (ok) g.out[off] = OP == OP_FWD ? fwd_value(xv, rw, g, p) : bwd_value(xv, dv, rw);
    }
}

// ---- WAVE and GROUP: a row in the registers of LANES lanes, NCH groups of four a lane ----
// chunk c of the row holds the elements 4c .. 4c + 3; lane t holds the chunks t, t + LANES, ...
template <int OP, int LANES, int NCH>
__device__ __forceinline__ void row_in_registers(const GnArgs &g, unsigned r, unsigned t, double *part) {
    const unsigned L = (unsigned)g.L;
    const size_t base = (size_t)r * L;
    const bool param = needs_param<OP>(g);
    const unsigned p0 = param ? row_param0(g, r) : 0u;
    const unsigned inner = (unsigned)g.inner;
    Row rw = {0.0f, 0.0f, 0.0f, 0.0f};
    double K = 0.0;
    if (OP == OP_FWD) K = (double)g.x[base];
    else rw.mean = g.save_mean[r], rw.invstd = g.save_invstd[r];
    v4f xv[NCH], dv[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned j = 4u * (k * LANES + t);
        xv[k] = v4f{0.0f, 0.0f, 0.0f, 0.0f}, dv[k] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        if (j < L) {
            if (g.vec) {   // L % 4 == 0: j + 3 < L
                xv[k] = *(const v4f_u *)(g.x + base + j);
                if (OP == OP_BWD) dv[k] = *(const v4f_u *)(g.dy + base + j);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < L) {
                        xv[k][e] = g.x[base + j + e];
                        if (OP == OP_BWD) dv[k][e] = g.dy[base + j + e];
                    }
            }
            if (OP == OP_BWD && param) {   // g = f32(dy . gamma[p]) takes dy's place
                unsigned q = quotient(j, g.by_inner), i = j - q * inner;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (j + e < L) dv[k][e] = dv[k][e] * g.gamma[p0 + q];
                    if (++i == inner) i = 0, ++q;
                }
            }
        }
    }
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned j = 4u * (k * LANES + t);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < L) add_terms<OP>(xv[k][e], dv[k][e], K, rw, a, b);
    }
    group_sum2<LANES / 64>(a, b, part);
    float o1, o2;
    finish_row<OP>(g, K, a, b, o1, o2);
    if (OP == OP_FWD) {
        rw.mean = o1, rw.invstd = o2;
        if (t == 0) g.save_mean[r] = o1, g.save_invstd[r] = o2;
    } else {
        rw.mb = o1, rw.mg = o2;
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const unsigned j = 4u * (k * LANES + t);
        if (j < L) {
            v4f res;
            unsigned q = 0, i = 0;
            if (OP == OP_FWD && param) q = quotient(j, g.by_inner), i = j - q * inner;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                res[e] = 0.0f;
                if (j + e < L) res[e] = OP == OP_FWD ? fwd_value(xv[k][e], rw, g, p0 + q) : bwd_value(xv[k][e], dv[k][e], rw);
                if (OP == OP_FWD && param && ++i == inner) i = 0, ++q;
            }
            if (g.vec) {
                *(v4f_u *)(g.out + base + j) = res;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < L) g.out[base + j + e] = res[e];
            }
        }
    }
}

template <int OP, int NCH>
__global__ __launch_bounds__(256) void gn_wave_kernel(const GnArgs g) {
    for (size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < g.M; r += (size_t)gridDim.x * 4)
        row_in_registers<OP, 64, NCH>(g, (unsigned)r, threadIdx.x & 63, nullptr);
}

template <int OP, int WAVES, int NCH>
__global__ __launch_bounds__(WAVES * 64) void gn_group_kernel(const GnArgs g) {
    __shared__ double part[2 * WAVES];
    for (unsigned r = blockIdx.x; r < g.M; r += gridDim.x) row_in_registers<OP, WAVES * 64, NCH>(g, r, threadIdx.x, part);
}

// ---- SPLIT: slices of whole groups of four along a row ----
// i: a position inside a plane of `inner`, q: the planes passed; both move on by `step` elements
__device__ __forceinline__ void advance(const GnArgs &g, size_t &q, size_t &i, unsigned step) {
    i += step;
    if (g.inner_small) {
        const unsigned k = quotient((unsigned)i, g.by_inner);   // i < inner + step < 2^31
        q += k;
        i -= (size_t)k * g.inner;
    } else {
        while (i >= g.inner) i -= g.inner, ++q;
    }
}

// slice s of row r: f(j, q, i, cnt) for the group of four at element j of the row (cnt = 4: all four inside the row and one
// access; cnt = 1: take the elements j .. j + 3 below L one by one), the first at position i of the row's plane q
template <class F>
__device__ __forceinline__ void walk_row_slice(const GnArgs &g, unsigned s, bool param, F f) {
    const size_t groups = (g.L + 3) / 4, c0 = (size_t)s * g.per, c1 = c0 + g.per < groups ? c0 + g.per : groups;
    size_t q = 0, i = 0;
    if (param) {
        q = (c0 * 4) / g.inner, i = c0 * 4 - q * g.inner;   // the slice's first element: once per workgroup
        advance(g, q, i, threadIdx.x * 4);
    }
    for (size_t c = c0 + threadIdx.x; c < c1; c += 256) {
        f(c * 4, q, i, g.vec ? 4 : 1);
        if (param) advance(g, q, i, 1024);
    }
}

template <int OP>
__global__ __launch_bounds__(256) void gn_stats_kernel(const GnArgs g) {
    __shared__ double part[8];
    const size_t items = (size_t)g.M * g.S;
    const bool param = OP == OP_BWD && g.gamma != nullptr;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned r = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)r * g.S);
        const size_t base = (size_t)r * g.L;
        const unsigned p0 = param ? row_param0(g, r) : 0u;
        Row rw = {0.0f, 0.0f, 0.0f, 0.0f};
        double K = 0.0;
        if (OP == OP_FWD) K = (double)g.x[base];
        else rw.mean = g.save_mean[r], rw.invstd = g.save_invstd[r];
        double a = 0.0, b = 0.0;
        walk_row_slice(g, s, param, [&](size_t j, size_t q, size_t i, int cnt) {
            v4f xv = {0.0f, 0.0f, 0.0f, 0.0f}, dv = {0.0f, 0.0f, 0.0f, 0.0f};
            if (cnt == 4) {
                xv = *(const v4f_u *)(g.x + base + j);
                if (OP == OP_BWD) dv = *(const v4f_u *)(g.dy + base + j);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < g.L) {
                        xv[e] = g.x[base + j + e];
                        if (OP == OP_BWD) dv[e] = g.dy[base + j + e];
                    }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j + e < g.L) {
                    const float v = param ? dv[e] * g.gamma[p0 + q] : dv[e];
                    add_terms<OP>(xv[e], v, K, rw, a, b);
                }
                if (param && ++i == g.inner) i = 0, ++q;
            }
        });
        group_sum2<4>(a, b, part);
        if (threadIdx.x == 0) g.part[2 * w] = a, g.part[2 * w + 1] = b;
    }
}

// a wave per row: the partials in slice order (lane l takes l, l + 64, ...; then the butterfly), then the row's scalars
template <int OP>
__global__ __launch_bounds__(64) void gn_fold_kernel(const GnArgs g) {
    for (unsigned r = blockIdx.x; r < g.M; r += gridDim.x) {
        double a = 0.0, b = 0.0;
        for (unsigned s = threadIdx.x; s < g.S; s += 64) {
            const size_t w = (size_t)r * g.S + s;
            a += g.part[2 * w], b += g.part[2 * w + 1];
        }
        wave_sum2(a, b);
        const double K = OP == OP_FWD ? (double)g.x[(size_t)r * g.L] : 0.0;
        float o1, o2;
        finish_row<OP>(g, K, a, b, o1, o2);
        if (threadIdx.x == 0) {
            if (OP == OP_FWD) g.save_mean[r] = o1, g.save_invstd[r] = o2;
            else g.mbmg[2 * (size_t)r] = o1, g.mbmg[2 * (size_t)r + 1] = o2;
        }
    }
}

template <int OP>
__global__ __launch_bounds__(256) void gn_apply_kernel(const GnArgs g) {
    const size_t items = (size_t)g.M * g.S;
    const bool param = needs_param<OP>(g);
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned r = (unsigned)(w / g.S), s = (unsigned)(w - (size_t)r * g.S);
        const size_t base = (size_t)r * g.L;
        const unsigned p0 = param ? row_param0(g, r) : 0u;
        Row rw = {g.save_mean[r], g.save_invstd[r], 0.0f, 0.0f};
        if (OP == OP_BWD) rw.mb = g.mbmg[2 * (size_t)r], rw.mg = g.mbmg[2 * (size_t)r + 1];
        walk_row_slice(g, s, param, [&](size_t j, size_t q, size_t i, int cnt) {
            v4f xv = {0.0f, 0.0f, 0.0f, 0.0f}, dv = {0.0f, 0.0f, 0.0f, 0.0f}, res;
            if (cnt == 4) {
                xv = *(const v4f_u *)(g.x + base + j);
                if (OP == OP_BWD) dv = *(const v4f_u *)(g.dy + base + j);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < g.L) {
                        xv[e] = g.x[base + j + e];
                        if (OP == OP_BWD) dv[e] = g.dy[base + j + e];
                    }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned p = p0 + (unsigned)q;
                if (OP == OP_FWD) {
                    res[e] = j + e < g.L ? fwd_value(xv[e], rw, g, p) : 0.0f;
                } else {
                    const float v = param && j + e < g.L ? dv[e] * g.gamma[p] : dv[e];
                    res[e] = bwd_value(xv[e], v, rw);
                }
                if (param && ++i == g.inner) i = 0, ++q;
            }
            if (cnt == 4) {
                *(v4f_u *)(g.out + base + j) = res;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < g.L) g.out[base + j + e] = res[e];
            }
        });
    }
}

// ---- the parameter gradients ----
// COLUMNS: inner == 1, x is (N, P).  Lane t: parameter lane t % CW, row lane t / CW; a work item is (parameter block, slice of N)
__global__ __launch_bounds__(256) void gn_param_columns_kernel(const GnArgs g) {
    __shared__ double sh[512];
    const unsigned CW = g.CW, RL = 256 / CW, cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW;
    const size_t items = (size_t)((g.P + CW - 1) / CW) * g.PS;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned cb = (unsigned)(w / g.PS), s = (unsigned)(w - (size_t)cb * g.PS), p = cb * CW + cl;
        const size_t n0 = (size_t)s * g.pper, n1 = n0 + g.pper < g.N ? n0 + g.pper : g.N;
        double a = 0.0, b = 0.0;
        if (p < g.P) {
            const unsigned gi = quotient(p, g.by_D);
#pragma unroll 4
            for (size_t n = n0 + rl; n < n1; n += RL) {
                const size_t off = n * g.P + p, row = n * g.G + gi;
                const Row rw = {g.save_mean[row], g.save_invstd[row], 0.0f, 0.0f};
                const float dy = g.dy[off];
                a += (double)dy;
                b += (double)dy * (double)xhat(g.x[off], rw);
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
        if (rl == 0 && p < g.P) {
            const size_t at = (size_t)p * g.PS + s;
            g.ppart[2 * at] = a, g.ppart[2 * at + 1] = b;
        }
    }
}

// PLANES: a workgroup per (parameter, slice); the n = N.inner values of a parameter in groups of four
__global__ __launch_bounds__(256) void gn_param_planes_kernel(const GnArgs g) {
    __shared__ double part[8];
    const size_t items = (size_t)g.P * g.PS;
    for (size_t w = blockIdx.x; w < items; w += gridDim.x) {
        const unsigned p = (unsigned)(w / g.PS), s = (unsigned)(w - (size_t)p * g.PS), gi = p / g.D;
        const size_t groups = (g.n + 3) / 4, c0 = (size_t)s * g.pper, c1 = c0 + g.pper < groups ? c0 + g.pper : groups;
        size_t ni = (c0 * 4) / g.inner, i = c0 * 4 - ni * g.inner;   // the slice's first element: once per workgroup
        advance(g, ni, i, threadIdx.x * 4);
        double a = 0.0, b = 0.0;
        for (size_t c = c0 + threadIdx.x; c < c1; c += 256) {
            if (g.pvec) {   // inner % 4 == 0: the group never leaves its plane
                const size_t off = (ni * g.P + p) * g.inner + i, row = ni * g.G + gi;
                const Row rw = {g.save_mean[row], g.save_invstd[row], 0.0f, 0.0f};
                const v4f xv = *(const v4f_u *)(g.x + off), dv = *(const v4f_u *)(g.dy + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a += (double)dv[e];
                    b += (double)dv[e] * (double)xhat(xv[e], rw);
                }
            } else {
                size_t nn = ni, ii = i;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c * 4 + e < g.n) {
                        const size_t off = (nn * g.P + p) * g.inner + ii, row = nn * g.G + gi;
                        const Row rw = {g.save_mean[row], g.save_invstd[row], 0.0f, 0.0f};
                        const float dy = g.dy[off];
                        a += (double)dy;
                        b += (double)dy * (double)xhat(g.x[off], rw);
                    }
                    if (++ii == g.inner) ii = 0, ++nn;
                }
            }
            advance(g, ni, i, 1024);
        }
        group_sum2<4>(a, b, part);
        if (threadIdx.x == 0) g.ppart[2 * w] = a, g.ppart[2 * w + 1] = b;
    }
}

// a wave per parameter: the partials in slice order, then dbeta and dgamma
__global__ __launch_bounds__(64) void gn_param_fold_kernel(const GnArgs g) {
    for (unsigned p = blockIdx.x; p < g.P; p += gridDim.x) {
        double a = 0.0, b = 0.0;
        for (unsigned s = threadIdx.x; s < g.PS; s += 64) {
            const size_t w = (size_t)p * g.PS + s;
            a += g.ppart[2 * w], b += g.ppart[2 * w + 1];
        }
        wave_sum2(a, b);
        if (threadIdx.x == 0) {
            if (g.dbeta) g.dbeta[p] = (float)a;
            if (g.dgamma) g.dgamma[p] = (float)b;
        }
    }
}

// ---- host ----
bool row_serves(int form, size_t L) {
    switch (form) {
    case ROW_SHORT: return L <= kShortMaxL;
    case ROW_WAVE: return L <= kWaveMaxL;
    case ROW_GROUP: return L <= kGroupMaxL;
    case ROW_SPLIT: return true;
    default: return false;
    }
}

bool param_serves(int form, size_t inner) { return form == PARAM_PLANES || (form == PARAM_COLUMNS && inner == 1); }

// the forms come from (D, inner) alone, and from the A-B switch
int pick_forms(const char *who, size_t L, size_t inner, int &row_form, int &param_form) {
    row_form = L <= kShortMaxL ? ROW_SHORT : L <= kWaveMaxL ? ROW_WAVE : L <= kGroupMaxL ? ROW_GROUP : ROW_SPLIT;
    param_form = inner == 1 ? PARAM_COLUMNS : PARAM_PLANES;
    if (g_gn_force_row >= 0) {
        if (!row_serves(g_gn_force_row, L)) return np::fail(NP_ERR_INVALID, "%s: the forced row form %d cannot serve L = %zu", who, g_gn_force_row, L);
        row_form = g_gn_force_row;
    }
    if (g_gn_force_param >= 0) {
        if (!param_serves(g_gn_force_param, inner))
            return np::fail(NP_ERR_INVALID, "%s: the forced parameter form %d cannot serve inner = %zu", who, g_gn_force_param, inner);
        param_form = g_gn_force_param;
    }
    return NP_OK;
}

size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// slices from the extents alone: `units` of work (groups of four, or rows) cut so that a slice holds at least kSliceMinSteps
// steps of a workgroup, the grid aims at kTargetGroups workgroups over `blocks` rows or parameter blocks, and S <= kMaxSlices
void plan_slices(size_t units, size_t per_step, size_t blocks, unsigned &S, size_t &per) {
    const size_t steps = ceil_div(units, per_step);
    size_t s = steps / kSliceMinSteps;
    if (s > kTargetGroups / blocks) s = kTargetGroups / blocks;
    if (s > kMaxSlices) s = kMaxSlices;
    if (s < 1) s = 1;
    per = ceil_div(units, s);
    S = (unsigned)ceil_div(units, per);
}

unsigned grid_of(size_t blocks) { return (unsigned)(blocks < kMaxGrid ? (blocks < 1 ? 1 : blocks) : kMaxGrid); }

void set_geometry(GnArgs &g, size_t N, size_t G, size_t D, size_t inner) {
    g.N = N, g.inner = inner, g.L = D * inner, g.n = N * inner;
    g.M = (unsigned)(N * G), g.G = (unsigned)G, g.D = (unsigned)D, g.P = (unsigned)(G * D);
    g.inner_small = inner <= kFastDivMax;
    g.by_inner = fast_div(g.inner_small ? (unsigned)inner : 1u);
    g.by_G = fast_div(g.G);
    g.by_D = fast_div(g.D);
    g.vec = g.L % 4 == 0;
    g.pvec = inner % 4 == 0;
}

// the row pass in the form given; adds its launches to `launches`
template <int OP>
int launch_rows(int form, GnArgs &g, int &launches) {
    g.S = 0;
    hipStream_t st = np::stream();
    if (form == ROW_SHORT) {
        g.W = 1, g.Wlog = 0;
        while (g.W < g.L) g.W *= 2, ++g.Wlog;
        const size_t waves = ceil_div(g.M, 64u >> g.Wlog);
        gn_short_kernel<OP><<<grid_of(ceil_div(waves, 4)), 256, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_short_kernel");
        launches += 1;
    } else if (form == ROW_WAVE) {
        const unsigned grid = grid_of(ceil_div(g.M, 4));
        if (g.L <= 256) gn_wave_kernel<OP, 1><<<grid, 256, 0, st>>>(g);
        else if (g.L <= 512) gn_wave_kernel<OP, 2><<<grid, 256, 0, st>>>(g);
        else gn_wave_kernel<OP, 4><<<grid, 256, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_wave_kernel");
        launches += 1;
    } else if (form == ROW_GROUP) {
        const unsigned grid = grid_of(g.M);
        if (g.L <= kGroupSmallL / 2) gn_group_kernel<OP, 4, 2><<<grid, 256, 0, st>>>(g);
        else if (g.L <= kGroupSmallL) gn_group_kernel<OP, 4, 4><<<grid, 256, 0, st>>>(g);
        else gn_group_kernel<OP, 16, 2><<<grid, 1024, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_group_kernel");
        launches += 1;
    } else {
        plan_slices(ceil_div(g.L, 4), 256, g.M, g.S, g.per);
        const size_t items = (size_t)g.M * g.S;
        np::Scratch part, mbmg;   // released on every path below
        if (int rc = part.alloc(2 * items * sizeof(double))) return rc;
        g.part = (double *)part.ptr;
        if (OP == OP_BWD) {
            if (int rc = mbmg.alloc(2 * (size_t)g.M * sizeof(float))) return rc;
            g.mbmg = (float *)mbmg.ptr;
        }
        gn_stats_kernel<OP><<<grid_of(items), 256, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_stats_kernel");
        gn_fold_kernel<OP><<<grid_of(g.M), 64, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_fold_kernel");
        gn_apply_kernel<OP><<<grid_of(items), 256, 0, st>>>(g);
        NP_LAUNCH_CHECK("gn_apply_kernel");
        launches += 3;
    }
    return NP_OK;
}

int launch_params(int form, GnArgs &g, int &launches) {
    g.CW = 1;
    size_t items;
    if (form == PARAM_COLUMNS) {
        while (g.CW < 64 && g.CW < g.P) g.CW *= 2;
        plan_slices(g.N, 256 / g.CW, ceil_div(g.P, g.CW), g.PS, g.pper);
        items = ceil_div(g.P, g.CW) * g.PS;
    } else {
        plan_slices(ceil_div(g.n, 4), 256, g.P, g.PS, g.pper);
        items = (size_t)g.P * g.PS;
    }
    np::Scratch ppart;   // released on every path below
    if (int rc = ppart.alloc(2 * (size_t)g.P * g.PS * sizeof(double))) return rc;
    g.ppart = (double *)ppart.ptr;
    hipStream_t st = np::stream();
    if (form == PARAM_COLUMNS) gn_param_columns_kernel<<<grid_of(items), 256, 0, st>>>(g);
    else gn_param_planes_kernel<<<grid_of(items), 256, 0, st>>>(g);
    NP_LAUNCH_CHECK("gn_param_kernel");
    gn_param_fold_kernel<<<grid_of(g.P), 64, 0, st>>>(g);
    NP_LAUNCH_CHECK("gn_param_fold_kernel");
    launches += 2;
    return NP_OK;
}

// the extents of a call; numel is written when they are accepted.  No device is touched.
int check_extents(const char *who, size_t N, size_t G, size_t D, size_t inner, size_t &numel) {
    if (N < 1 || G < 1 || D < 1 || inner < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (N >= kIndexLim || G >= kIndexLim || N * G >= kIndexLim) return np::fail(NP_ERR_INVALID, "%s: N.G = %zu rows is 2^31 or more", who, N * G);
    if (D >= kIndexLim || G * D >= kIndexLim) return np::fail(NP_ERR_INVALID, "%s: G.D = %zu parameters is 2^31 or more", who, G * D);
    const size_t lim = SIZE_MAX / sizeof(float), M = N * G;
    if (D > lim / M || M * D > lim / inner) return np::fail(NP_ERR_INVALID, "%s: N.G.D.inner does not fit a size_t", who);
    numel = M * D * inner;
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

// The order is the pointers, the extents, the parameters, the aliasing, the forms, ensure_init, then work: a refused call has touched no device.
int np_groupnorm_forward(const float *x, const float *gamma, const float *beta, size_t N, size_t G, size_t D, size_t inner, double eps, float *y,
                         float *save_mean, float *save_invstd) {
    const char *who = "np_groupnorm_forward";
    if (!x || !y || !save_mean || !save_invstd) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    size_t numel = 0;
    if (int rc = check_extents(who, N, G, D, inner, numel)) return rc;
    if (!(eps >= 0.0)) return np::fail(NP_ERR_INVALID, "%s: eps must not be negative", who);
    const size_t M = N * G, P = G * D;
    const Range in[] = {{x, numel}, {gamma, P}, {beta, P}};
    const Range out[] = {{y, numel}, {save_mean, M}, {save_invstd, M}};
    if (any_overlap(out, 3, in, 3)) return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output", who);
    int row_form = 0, param_form = 0;
    if (int rc = pick_forms(who, D * inner, inner, row_form, param_form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    GnArgs g = {};
    g.x = x, g.gamma = gamma, g.beta = beta, g.out = y, g.save_mean = save_mean, g.save_invstd = save_invstd, g.eps = eps;
    set_geometry(g, N, G, D, inner);
    int launches = 0;
    if (int rc = launch_rows<OP_FWD>(row_form, g, launches)) return rc;
    g_gn_last_row_form = row_form, g_gn_last_param_form = 0, g_gn_last_launches = launches;
    g_gn_last_row_slices = g.S, g_gn_last_param_slices = 0;
    return NP_OK;
}

int np_groupnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd, size_t N, size_t G,
                          size_t D, size_t inner, float *dx, float *dgamma, float *dbeta) {
    const char *who = "np_groupnorm_backward";
    if (!x || !dy || !save_mean || !save_invstd || !dx) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    size_t numel = 0;
    if (int rc = check_extents(who, N, G, D, inner, numel)) return rc;
    const size_t M = N * G, P = G * D;
    const Range in[] = {{x, numel}, {dx == dy ? nullptr : dy, numel}, {gamma, P}, {save_mean, M}, {save_invstd, M}};
    const Range out[] = {{dx, numel}, {dgamma, P}, {dbeta, P}};
    if (any_overlap(out, 3, in, 5) || overlap({dy, numel}, {dgamma, P}) || overlap({dy, numel}, {dbeta, P}))
        return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output (dx == dy is allowed)", who);
    int row_form = 0, param_form = 0;
    if (int rc = pick_forms(who, D * inner, inner, row_form, param_form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    GnArgs g = {};
    g.x = x, g.dy = dy, g.gamma = gamma, g.out = dx, g.save_mean = (float *)save_mean, g.save_invstd = (float *)save_invstd;
    g.dgamma = dgamma, g.dbeta = dbeta;
    set_geometry(g, N, G, D, inner);
    int launches = 0;
    const bool params = dgamma || dbeta;
    g.PS = 0;
    if (params)   // first: it reads dy, which dx may alias
        if (int rc = launch_params(param_form, g, launches)) return rc;
    if (int rc = launch_rows<OP_BWD>(row_form, g, launches)) return rc;
    g_gn_last_row_form = row_form, g_gn_last_param_form = params ? param_form : 0, g_gn_last_launches = launches;
    g_gn_last_row_slices = g.S, g_gn_last_param_slices = g.PS;
    return NP_OK;
}

int np_debug_groupnorm_last_path(int *row_form, int *param_form, int *launches, size_t *row_slices, size_t *param_slices) {
    if (!row_form || !param_form || !launches || !row_slices || !param_slices)
        return np::fail(NP_ERR_INVALID, "np_debug_groupnorm_last_path: null pointer");
    *row_form = g_gn_last_row_form, *param_form = g_gn_last_param_form, *launches = g_gn_last_launches;
    *row_slices = g_gn_last_row_slices, *param_slices = g_gn_last_param_slices;
    return NP_OK;
}

int np_debug_groupnorm_force_form(int row_form, int param_form) {
    if (row_form != -1 && (row_form < ROW_SHORT || row_form > ROW_SPLIT))
        return np::fail(NP_ERR_INVALID, "np_debug_groupnorm_force_form: row_form must be -1 (by the extents) or 1 .. 4");
    if (param_form != -1 && (param_form < PARAM_COLUMNS || param_form > PARAM_PLANES))
        return np::fail(NP_ERR_INVALID, "np_debug_groupnorm_force_form: param_form must be -1 (by the extents) or 1 .. 2");
    g_gn_force_row = row_form, g_gn_force_param = param_form;
    return NP_OK;
}

int np_debug_groupnorm_bounds(size_t bounds[], int n) {
    if (!bounds) return np::fail(NP_ERR_INVALID, "np_debug_groupnorm_bounds: null pointer");
    if (n < kNumBounds) return np::fail(NP_ERR_INVALID, "np_debug_groupnorm_bounds: room for %d values is needed", kNumBounds);
    bounds[0] = kShortMaxL, bounds[1] = kWaveMaxL, bounds[2] = kGroupSmallL, bounds[3] = kGroupMaxL;
    bounds[4] = kTargetGroups, bounds[5] = kMaxSlices, bounds[6] = kSliceMinSteps;
    return NP_OK;
}

}  // extern "C"
