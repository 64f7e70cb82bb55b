// Optimizer steps for GPU arrays: np_sgd_step, np_adam_step over a LIST of tensors in one launch, and
// np_grad_norm, the gradient norm and clip coefficient of a list.  The rules are in np_hip.h; this comment says how the kernels
// keep them.
//
// The list travels in the kernel arguments, by value (OptimList: kOptimMaxTensors entries of four pointers and a size, a prefix
// array of chunk counts, a mode byte per tensor): no device table, no copy, no scratch, no synchronisation, so a step can sit
// inside a stream capture.  T tensors take ceil(T / kOptimMaxTensors) launches, packed by tensor count alone.
//
// Work is cut into chunks of kChunk elements.  A workgroup walks the chunk index grid-stride (the grid comes from the CU count),
// finds the chunk's tensor by a binary search of the prefix array — nothing grows with the element count — and updates the
// chunk's elements.  An element's result is element_sgd / element_adam of that element's operands and the uniform coefficients:
// which lane computes it, in which chunk, through which access width cannot change a bit.
//
// Access width, per tensor (mode_of): when every pointer of the tensor has the same residue mod 16 the tensor is seen from the
// 16-byte boundary at or below its first element, o = residue / 4 floats before it; chunks cut that view, a lane takes groups of
// four floats, a group that lies inside the tensor is one 16-byte access per stream, a group that straddles an end (the head of
// the first chunk, the tail of the last) is walked by element.  Otherwise (and under np_debug_optim_force_scalar) chunks cut the
// tensor itself and every access is one float, consecutive lanes on consecutive floats.
//
// np_grad_norm: chunks of kNormChunk elements, one fp64 partial per chunk in pool scratch (per lane in ascending order, lanes by
// a xor butterfly, waves in ascending order), then ONE workgroup adds the partials (thread t takes t, t + 256, ... ascending,
// then the same join) and writes both floats.  The order is a function of (n_t, T) alone; loads are 16 bytes wide at any 4-byte
// alignment, so the alignment does not enter it either.  No atomics anywhere in this unit.
#include <algorithm>
#include <vector>

#include "np_internal.h"

#pragma clang fp contract(off)

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_u __attribute__((aligned(4)));   // float4 access that only assumes dword alignment

constexpr unsigned kChunk = 4096;            // elements of a step chunk: 256 lanes x 4 groups of four (np_debug_optim_bounds reports these; tests/optim_family.py restates the dispatcher)
constexpr unsigned kOptimMaxTensors = 64;    // tensors of one launch
constexpr unsigned kNormChunk = 8192;        // elements behind one partial of np_grad_norm
constexpr unsigned kWgPerCu = 8;             // the grid: at most CUs x this many workgroups, made odd when capped
constexpr int kNumBounds = 5;
constexpr unsigned kGroups = kChunk / 1024;  // groups of four a lane holds per chunk
constexpr unsigned char kModeScalar = 4;     // OptimList::mode: 0 .. 3 = 16-byte accesses, the tensor starts o floats past a 16-byte boundary

// the kernel argument: 64 x 40 + 65 x 8 + 64 + 8 = 3152 bytes, under the 4096 bytes a launch is sure to carry
struct OptimList {
    float *p[kOptimMaxTensors];
    const float *g[kOptimMaxTensors];
    float *s1[kOptimMaxTensors];             // momentum buffer | exp_avg
    float *s2[kOptimMaxTensors];             // exp_avg_sq
    size_t n[kOptimMaxTensors];
    size_t first[kOptimMaxTensors + 1];      // first[t]: chunks before tensor t; first[T]: chunks of the launch
    unsigned char mode[kOptimMaxTensors];
    unsigned T;
};
static_assert(sizeof(OptimList) + 64 <= 4096, "the list and the coefficients fit the kernel-argument segment");

// coefficients: each computed in double on the host and rounded to fp32 once (np_hip.h states each)
struct SgdCoef {
    float lr, wd, mu, omd;                   // omd = f32(1 - dampening)
    int has_wd, has_mom, nesterov, first;
    const float *scale;                      // device float or nullptr
};
struct AdamCoef {
    float wd, lrwd, b1, omb1, b2, omb2, bc2s, eps, step;   // lrwd = f32(lr . wd); bc2s = f32(sqrt(1 - b2^t)); step = f32(lr / (1 - b1^t))
    int has_wd, decoupled;
    const float *scale;
};

int g_optim_launches = 0;                    // np_debug_optim_last_path
size_t g_optim_chunks = 0;
int g_optim_vec = 0, g_optim_scalar = 0;
int g_optim_force_scalar = 0;                // np_debug_optim_force_scalar

// The correctly rounded square root: sqrtf, which hipcc expands to the hardware's estimate and a correction (the default of
// -fhip-fp32-correctly-rounded-divide-sqrt).  __fsqrt_rn is NOT: without OCML's rounded operations it is the bare estimate, 1 ulp.
__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }

// ---- element values: every access form writes through these ----
__device__ __forceinline__ void element_sgd(const SgdCoef &k, float s, float &p, float g, float &b) {
    if (k.scale) g = g * s;
    if (k.has_wd) {
        const float t = k.wd * p;
        g = g + t;
    }
    float d = g;
    if (k.has_mom) {
        if (k.first) {
            b = g;
        } else {
            const float t1 = k.mu * b, t2 = k.omd * g;
            b = t1 + t2;
        }
        if (k.nesterov) {
            const float t = k.mu * b;
            d = g + t;
        } else {
            d = b;
        }
    }
    const float u = k.lr * d;
    p = p - u;
}

__device__ __forceinline__ void element_adam(const AdamCoef &k, float s, float &p, float g, float &m, float &v) {
    if (k.scale) g = g * s;
    float p1 = p;
    if (k.has_wd) {
        if (k.decoupled) {
            const float t = k.lrwd * p;
            p1 = p - t;
        } else {
            const float t = k.wd * p;
            g = g + t;
        }
    }
    const float m1 = k.b1 * m, m2 = k.omb1 * g;
    m = m1 + m2;
    const float v1 = k.b2 * v, v2 = k.omb2 * g, v3 = v2 * g;
    v = v1 + v3;
    const float r = sqrt_rn(v), q = __fdiv_rn(r, k.bc2s), den = q + k.eps;
    const float w = __fdiv_rn(m, den), u = k.step * w;
    p = p1 - u;
}

// ALG 0: SGD (s1 = the buffer when has_mom), 1: Adam (s1 = m, s2 = v)
template <int ALG, class Coef>
__device__ __forceinline__ void one_element(const Coef &k, float s, float *p, const float *g, float *s1, float *s2, size_t i) {
    float pv = p[i];
    if constexpr (ALG == 0) {
        float b = 0.0f;
        if (k.has_mom && !k.first) b = s1[i];
        element_sgd(k, s, pv, g[i], b);
        if (k.has_mom) s1[i] = b;
    } else {
        float m = s1[i], v = s2[i];
        element_adam(k, s, pv, g[i], m, v);
        s1[i] = m, s2[i] = v;
    }
    p[i] = pv;
}

// four contiguous elements at i, every pointer 16-byte aligned there
template <int ALG, class Coef>
__device__ __forceinline__ void load_group(const Coef &k, const float *p, const float *g, const float *s1, const float *s2, size_t i, v4f &pv,
                                           v4f &gv, v4f &av, v4f &bv) {
    pv = *(const v4f *)(p + i), gv = *(const v4f *)(g + i);
    av = v4f{0.0f, 0.0f, 0.0f, 0.0f}, bv = av;
    if constexpr (ALG == 0) {
        if (k.has_mom && !k.first) av = *(const v4f *)(s1 + i);
    } else {
        av = *(const v4f *)(s1 + i), bv = *(const v4f *)(s2 + i);
    }
}
template <int ALG, class Coef>
__device__ __forceinline__ void finish_group(const Coef &k, float s, float *p, float *s1, float *s2, size_t i, v4f pv, v4f gv, v4f av, v4f bv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = pv[e], ae = av[e], be = bv[e];
        if constexpr (ALG == 0) element_sgd(k, s, pe, gv[e], ae);
        else element_adam(k, s, pe, gv[e], ae, be);
        pv[e] = pe, av[e] = ae, bv[e] = be;
    }
    *(v4f *)(p + i) = pv;
    if constexpr (ALG == 0) {
        if (k.has_mom) *(v4f *)(s1 + i) = av;
    } else {
        *(v4f *)(s1 + i) = av, *(v4f *)(s2 + i) = bv;
    }
}

template <int ALG, class Coef>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimList L, const Coef k) {
    const float s = k.scale ? *k.scale : 1.0f;
    const size_t total = L.first[L.T];
    for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
        unsigned lo = 0, hi = L.T;               // the tensor of chunk c: first[lo] <= c < first[lo + 1]
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) / 2;
            if (L.first[mid] <= c) lo = mid;
            else hi = mid;
        }
        float *p = L.p[lo], *s1 = L.s1[lo], *s2 = L.s2[lo];
        const float *g = L.g[lo];
        const size_t n = L.n[lo], v0 = (c - L.first[lo]) * kChunk;   // the chunk's first position
        const unsigned mode = L.mode[lo];
        if (mode == kModeScalar) {
#pragma unroll 4
            for (unsigned j = 0; j < kChunk / 256; ++j) {
                const size_t i = v0 + j * 256 + threadIdx.x;
                if (i < n) one_element<ALG>(k, s, p, g, s1, s2, i);
            }
            continue;
        }
        // positions count from the 16-byte boundary o floats before the tensor: the tensor is [o, o + n)
        const size_t o = mode, end = o + n;
        if (v0 >= o && v0 + kChunk <= end) {     // an interior chunk: every load of the chunk is issued before the first use
            v4f pv[kGroups], gv[kGroups], av[kGroups], bv[kGroups];
#pragma unroll
            for (unsigned j = 0; j < kGroups; ++j)
                load_group<ALG>(k, p, g, s1, s2, v0 + 4 * (size_t)(j * 256 + threadIdx.x) - o, pv[j], gv[j], av[j], bv[j]);
#pragma unroll
            for (unsigned j = 0; j < kGroups; ++j)
                finish_group<ALG>(k, s, p, s1, s2, v0 + 4 * (size_t)(j * 256 + threadIdx.x) - o, pv[j], gv[j], av[j], bv[j]);
            continue;
        }
        for (unsigned j = 0; j < kGroups; ++j) {
            const size_t v = v0 + 4 * (size_t)(j * 256 + threadIdx.x);
            if (v >= end) break;
            if (v >= o && v + 4 <= end) {
                v4f pv, gv, av, bv;
                load_group<ALG>(k, p, g, s1, s2, v - o, pv, gv, av, bv);
                finish_group<ALG>(k, s, p, s1, s2, v - o, pv, gv, av, bv);
            } else {
                for (unsigned e = 0; e < 4; ++e)
                    if (v + e >= o && v + e < end) one_element<ALG>(k, s, p, g, s1, s2, v + e - o);
            }
        }
    }
}

// ---- the norm ----
struct NormList {
    const float *g[kOptimMaxTensors];
    size_t n[kOptimMaxTensors];
    size_t first[kOptimMaxTensors + 1];
    unsigned T;
};

// every lane of the workgroup gets the sum; part: 4 doubles of LDS
__device__ __forceinline__ double group_sum(double a, double *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    __syncthreads();   // the previous join's readers are done with part
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    a = part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) a += part[w];
    return a;
}

// partial[base + c] = the sum of squares of chunk c of the launch
__global__ __launch_bounds__(256) void norm_partial_kernel(const NormList L, double *partial) {
    __shared__ double part[4];
    const size_t total = L.first[L.T];
    for (size_t c = blockIdx.x; c < total; c += gridDim.x) {
        unsigned lo = 0, hi = L.T;
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) / 2;
            if (L.first[mid] <= c) lo = mid;
            else hi = mid;
        }
        const float *g = L.g[lo];
        const size_t n = L.n[lo], i0 = (c - L.first[lo]) * kNormChunk;
        double a = 0.0;
        if (i0 + kNormChunk <= n) {
            v4f x[kNormChunk / 1024];
#pragma unroll
            for (unsigned j = 0; j < kNormChunk / 1024; ++j) x[j] = *(const v4f_u *)(g + i0 + 4 * (size_t)(j * 256 + threadIdx.x));
#pragma unroll
            for (unsigned j = 0; j < kNormChunk / 1024; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) a += (double)x[j][e] * (double)x[j][e];
        } else {
            for (unsigned j = 0; j < kNormChunk / 1024; ++j)
                for (unsigned e = 0; e < 4; ++e) {
                    const size_t i = i0 + 4 * (size_t)(j * 256 + threadIdx.x) + e;
                    if (i < n) a += (double)g[i] * (double)g[i];
                }
        }
        a = group_sum(a, part);
        if (threadIdx.x == 0) partial[c] = a;
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in ascending order, the same join, then both floats
__global__ __launch_bounds__(256) void norm_fold_kernel(const double *partial, size_t count, double max_norm, float *out) {
    __shared__ double part[4];
    double a = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 256) a += partial[i];
    a = group_sum(a, part);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(a);
        const double c = max_norm / ((double)norm + 1e-6);
        out[0] = norm;
        out[1] = (float)(c < 1.0 ? c : c != c ? c : 1.0);   // min(1, c) that keeps a NaN
    }
}

// ---- host ----
size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

unsigned grid_of(size_t chunks) { return (unsigned)np::capped_grid(chunks, (size_t)np::num_cus() * kWgPerCu); }

// 0 .. 3: every pointer of the tensor has the residue 4 . mode mod 16; kModeScalar otherwise
unsigned char mode_of(const float *p, const float *g, const float *s1, const float *s2) {
    const uintptr_t r = (uintptr_t)p & 15;
    if (g_optim_force_scalar || ((uintptr_t)g & 15) != r || (s1 && ((uintptr_t)s1 & 15) != r) || (s2 && ((uintptr_t)s2 & 15) != r)) return kModeScalar;
    return (unsigned char)(r / 4);
}

struct Range {
    uintptr_t lo, hi;
    bool written;
};

// true when a written range overlaps any other range (two gradients may share bytes): sorted by their start, a range
// overlaps an earlier one exactly when it starts below the largest end seen so far
bool written_overlap(std::vector<Range> &r) {
    std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
    uintptr_t end_any = 0, end_written = 0;
    for (const Range &x : r) {
        if (x.lo < (x.written ? end_any : end_written)) return true;
        if (x.hi > end_any) end_any = x.hi;
        if (x.written && x.hi > end_written) end_written = x.hi;
    }
    return false;
}

// pointers, then extents, of a list; s1 / s2: nullptr when the call has no such state
int check_list(const char *who, float *const *params, const float *const *grads, float *const *s1, bool need_s1, float *const *s2, bool need_s2,
               const size_t *counts, size_t T) {
    if (!params || !grads || !counts || (need_s1 && !s1) || (need_s2 && !s2)) return np::fail(NP_ERR_INVALID, "%s: null pointer (a list)", who);
    for (size_t t = 0; t < T; ++t)
        if (!params[t] || !grads[t] || (need_s1 && !s1[t]) || (need_s2 && !s2[t])) return np::fail(NP_ERR_INVALID, "%s: null pointer (tensor %zu)", who, t);
    if (T < 1) return np::fail(NP_ERR_INVALID, "%s: the list is empty", who);
    for (size_t t = 0; t < T; ++t) {
        if (counts[t] < 1) return np::fail(NP_ERR_INVALID, "%s: tensor %zu has no elements", who, t);
        if (counts[t] > SIZE_MAX / sizeof(float) / 2) return np::fail(NP_ERR_INVALID, "%s: tensor %zu does not fit a size_t", who, t);
    }
    return NP_OK;
}

int check_aliasing(const char *who, float *const *params, const float *const *grads, float *const *s1, float *const *s2, const size_t *counts, size_t T,
                   const float *scale) {
    std::vector<Range> r;
    r.reserve(4 * T + 1);
    for (size_t t = 0; t < T; ++t) {
        const size_t bytes = counts[t] * sizeof(float);
        r.push_back({(uintptr_t)params[t], (uintptr_t)params[t] + bytes, true});
        r.push_back({(uintptr_t)grads[t], (uintptr_t)grads[t] + bytes, false});
        if (s1) r.push_back({(uintptr_t)s1[t], (uintptr_t)s1[t] + bytes, true});
        if (s2) r.push_back({(uintptr_t)s2[t], (uintptr_t)s2[t] + bytes, true});
    }
    if (scale) r.push_back({(uintptr_t)scale, (uintptr_t)scale + sizeof(float), false});
    if (written_overlap(r))
        return np::fail(NP_ERR_INVALID, "%s: a parameter or a state overlaps another one, a gradient or grad_scale (two gradients may share memory)", who);
    return NP_OK;
}

bool finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

template <int ALG, class Coef>
int launch_steps(const char *name, float *const *params, const float *const *grads, float *const *s1, float *const *s2, const size_t *counts, size_t T,
                 const Coef &k) {
    int launches = 0, vec = 0, scalar = 0;
    size_t chunks = 0;
    for (size_t t0 = 0; t0 < T; t0 += kOptimMaxTensors) {
        OptimList L = {};
        L.T = (unsigned)(T - t0 < kOptimMaxTensors ? T - t0 : kOptimMaxTensors);
        for (unsigned j = 0; j < L.T; ++j) {
            const size_t t = t0 + j;
            L.p[j] = params[t], L.g[j] = grads[t], L.s1[j] = s1 ? s1[t] : nullptr, L.s2[j] = s2 ? s2[t] : nullptr, L.n[j] = counts[t];
            L.mode[j] = mode_of(L.p[j], L.g[j], L.s1[j], L.s2[j]);
            const size_t o = L.mode[j] == kModeScalar ? 0 : L.mode[j];
            L.first[j + 1] = L.first[j] + ceil_div(o + counts[t], kChunk);
            L.mode[j] == kModeScalar ? ++scalar : ++vec;
        }
        optim_step_kernel<ALG, Coef><<<grid_of(L.first[L.T]), 256, 0, np::stream()>>>(L, k);
        NP_LAUNCH_CHECK(name);
        ++launches, chunks += L.first[L.T];
    }
    g_optim_launches = launches, g_optim_chunks = chunks, g_optim_vec = vec, g_optim_scalar = scalar;
    return NP_OK;
}

}  // namespace

extern "C" {

// The order is the pointers, the extents, the parameters, the aliasing, ensure_init, then work: a refused call has touched no device.
int np_sgd_step(float *const *params, const float *const *grads, float *const *bufs, const size_t *counts, size_t T, double lr, double momentum,
                double dampening, double weight_decay, int nesterov, int first_step, const float *grad_scale) {
    const char *who = "np_sgd_step";
    const bool has_mom = momentum != 0.0;   // a NaN momentum has the buffers checked, then is refused below
    if (int rc = check_list(who, params, grads, bufs, has_mom, nullptr, false, counts, T)) return rc;
    if (!finite_nonneg(lr)) return np::fail(NP_ERR_INVALID, "%s: lr must be finite and not negative", who);
    if (!finite_nonneg(weight_decay)) return np::fail(NP_ERR_INVALID, "%s: weight_decay must be finite and not negative", who);
    if (!(momentum >= 0.0 && momentum <= 1.0)) return np::fail(NP_ERR_INVALID, "%s: momentum must lie in [0, 1]", who);
    if (!(dampening >= 0.0 && dampening <= 1.0)) return np::fail(NP_ERR_INVALID, "%s: dampening must lie in [0, 1]", who);
    if (nesterov && (momentum == 0.0 || dampening != 0.0)) return np::fail(NP_ERR_INVALID, "%s: nesterov needs a momentum and zero dampening", who);
    if (int rc = check_aliasing(who, params, grads, has_mom ? bufs : nullptr, nullptr, counts, T, grad_scale)) return rc;
    if (int rc = np::ensure_init()) return rc;
    SgdCoef k = {};
    k.lr = (float)lr, k.wd = (float)weight_decay, k.mu = (float)momentum, k.omd = (float)(1.0 - dampening);
    k.has_wd = weight_decay != 0.0, k.has_mom = has_mom, k.nesterov = nesterov != 0, k.first = first_step != 0, k.scale = grad_scale;
    return launch_steps<0>("optim_step_kernel (sgd)", params, grads, has_mom ? bufs : nullptr, nullptr, counts, T, k);
}

int np_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const size_t *counts, size_t T,
                 long long step, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, const float *grad_scale) {
    const char *who = "np_adam_step";
    if (int rc = check_list(who, params, grads, exp_avg, true, exp_avg_sq, true, counts, T)) return rc;
    if (!finite_nonneg(lr)) return np::fail(NP_ERR_INVALID, "%s: lr must be finite and not negative", who);
    if (!finite_nonneg(weight_decay)) return np::fail(NP_ERR_INVALID, "%s: weight_decay must be finite and not negative", who);
    if (!finite_nonneg(eps)) return np::fail(NP_ERR_INVALID, "%s: eps must be finite and not negative", who);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return np::fail(NP_ERR_INVALID, "%s: the betas must lie in [0, 1)", who);
    if (step < 1) return np::fail(NP_ERR_INVALID, "%s: step must be at least 1", who);
    if (int rc = check_aliasing(who, params, grads, exp_avg, exp_avg_sq, counts, T, grad_scale)) return rc;
    if (int rc = np::ensure_init()) return rc;
    AdamCoef k = {};
    k.wd = (float)weight_decay, k.lrwd = (float)(lr * weight_decay);
    k.b1 = (float)beta1, k.omb1 = (float)(1.0 - beta1), k.b2 = (float)beta2, k.omb2 = (float)(1.0 - beta2);
    k.bc2s = (float)sqrt(1.0 - pow(beta2, (double)step)), k.eps = (float)eps, k.step = (float)(lr / (1.0 - pow(beta1, (double)step)));
    k.has_wd = weight_decay != 0.0, k.decoupled = decoupled != 0, k.scale = grad_scale;
    return launch_steps<1>("optim_step_kernel (adam)", params, grads, exp_avg, exp_avg_sq, counts, T, k);
}

int np_grad_norm(const float *const *grads, const size_t *counts, size_t T, double max_norm, float *dev_out2) {
    const char *who = "np_grad_norm";
    if (!grads || !counts || !dev_out2) return np::fail(NP_ERR_INVALID, "%s: null pointer (a list or the result)", who);
    for (size_t t = 0; t < T; ++t)
        if (!grads[t]) return np::fail(NP_ERR_INVALID, "%s: null pointer (tensor %zu)", who, t);
    if (T < 1) return np::fail(NP_ERR_INVALID, "%s: the list is empty", who);
    for (size_t t = 0; t < T; ++t) {
        if (counts[t] < 1) return np::fail(NP_ERR_INVALID, "%s: tensor %zu has no elements", who, t);
        if (counts[t] > SIZE_MAX / sizeof(float) / 2) return np::fail(NP_ERR_INVALID, "%s: tensor %zu does not fit a size_t", who, t);
    }
    if (!(max_norm >= 0.0)) return np::fail(NP_ERR_INVALID, "%s: max_norm must not be negative (+Inf: no clipping)", who);
    std::vector<Range> r;
    r.reserve(T + 1);
    for (size_t t = 0; t < T; ++t) r.push_back({(uintptr_t)grads[t], (uintptr_t)grads[t] + counts[t] * sizeof(float), false});
    r.push_back({(uintptr_t)dev_out2, (uintptr_t)dev_out2 + 2 * sizeof(float), true});
    if (written_overlap(r)) return np::fail(NP_ERR_INVALID, "%s: the result overlaps a gradient", who);
    if (int rc = np::ensure_init()) return rc;
    size_t total = 0;
    for (size_t t = 0; t < T; ++t) total += ceil_div(counts[t], kNormChunk);
    np::Scratch partial;   // released on every path below
    if (int rc = partial.alloc(total * sizeof(double))) return rc;
    int launches = 0;
    size_t base = 0;
    for (size_t t0 = 0; t0 < T; t0 += kOptimMaxTensors) {
        NormList L = {};
        L.T = (unsigned)(T - t0 < kOptimMaxTensors ? T - t0 : kOptimMaxTensors);
        for (unsigned j = 0; j < L.T; ++j) {
            L.g[j] = grads[t0 + j], L.n[j] = counts[t0 + j];
            L.first[j + 1] = L.first[j] + ceil_div(counts[t0 + j], kNormChunk);
        }
        norm_partial_kernel<<<grid_of(L.first[L.T]), 256, 0, np::stream()>>>(L, (double *)partial.ptr + base);
        NP_LAUNCH_CHECK("norm_partial_kernel");
        ++launches, base += L.first[L.T];
    }
    norm_fold_kernel<<<1, 256, 0, np::stream()>>>((const double *)partial.ptr, total, max_norm, dev_out2);
    NP_LAUNCH_CHECK("norm_fold_kernel");
    g_optim_launches = launches + 1, g_optim_chunks = total, g_optim_vec = 0, g_optim_scalar = 0;
    return NP_OK;
}

int np_debug_optim_last_path(int *launches, size_t *chunks, int *vec_tensors, int *scalar_tensors) {
    if (!launches || !chunks || !vec_tensors || !scalar_tensors) return np::fail(NP_ERR_INVALID, "np_debug_optim_last_path: null pointer");
    *launches = g_optim_launches, *chunks = g_optim_chunks, *vec_tensors = g_optim_vec, *scalar_tensors = g_optim_scalar;
    return NP_OK;
}

int np_debug_optim_bounds(size_t bounds[], int n) {
    if (!bounds) return np::fail(NP_ERR_INVALID, "np_debug_optim_bounds: null pointer");
    if (n < kNumBounds) return np::fail(NP_ERR_INVALID, "np_debug_optim_bounds: room for %d values is needed", kNumBounds);
    bounds[0] = kChunk, bounds[1] = kOptimMaxTensors, bounds[2] = kNormChunk, bounds[3] = kWgPerCu, bounds[4] = sizeof(OptimList);
    return NP_OK;
}

int np_debug_optim_force_scalar(int on) {
    g_optim_force_scalar = on != 0;
    return NP_OK;
}

}  // extern "C"
