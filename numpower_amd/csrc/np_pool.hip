// Pooling layers for GPU arrays: np_pool2d_shape, np_pool2d_forward, np_pool2d_backward.
//
// x (planes, H, W) row-major fp32 with planes = N.C, window (kh, kw), stride (sh, sw), zero-width padding (ph, pw) with
// 2 ph <= kh and 2 pw <= kw, so every window holds at least one real cell.  y and idx (planes, oh, ow).  No dilation, no ceil
// mode.  Streaming kernels with reuse kh.kw / (sh.sw): no MFMA.
//
//   forward   two forms of ONE scan (pool_scan), chosen from the extents alone and reported by np_debug_pool_last_path:
//             1 DIRECT  one lane per output, flattened over planes.oh.ow with j fastest, so a wave's stores are consecutive;
//                       taps are read through the cache.  Planes of more than kStageCells cells.
//             2 STAGED  planes of at most kStageCells cells: a workgroup takes floor(kStageCells / (H.W)) whole planes, which
//                       are ONE contiguous run of x, copies the run to LDS with consecutive lanes on consecutive words, and
//                       its lanes then take the planes' outputs in turn, taps from LDS.  A 7 x 7 plane read directly costs a
//                       wave 64 cache lines per load instruction and the lines are evicted before their next word is wanted;
//                       staged, every word of x crosses the memory system once.
//             The output is decoded once (two quotients, FastDiv), the window is clipped to the image once, the scan is two
//             plain loops over real cells in row-major order: padding is never read and never a candidate.  Both forms run the
//             same scan in the same order: the same bits.
//               max        best = -Inf, idx = the first real cell; a cell is taken when v > best || v != v: the first of equal
//                          maxima, -0.0 == +0.0, a NaN wins and the LAST NaN keeps the index.  idx = u.W + v inside the plane.
//               average    ONE chain of fp32 adds from +0.0f, then ONE correctly rounded division by (float) divisor: kh.kw
//                          (NP_POOL_AVG, padding counts) or the number of real cells (NP_POOL_AVG_VALID).  No reciprocal.
//   backward  a GATHER, one lane per dx cell with v fastest: the covering ranges [i_lo, i_hi] x [j_lo, j_hi] are computed once
//             per cell (four quotients, FastDiv), then the windows are walked with i ascending, then j ascending, and the terms added
//             from +0.0f: dy[i,j] where idx[i,j] == u.W + v (max), dy[i,j] / (float) divisor(i,j) rounded on its own
//             (average).  There is no integer division inside the term loop: the valid divisor is a product of two clipped
//             lengths.  Cells no window covers keep +0.0f.  No float atomics, no scatter: bit-identical from run to run, and a
//             plane's result does not depend on the planes around it.
//
// The unit is compiled like the others: no fast-math, so the division is the correctly rounded one (v_div_scale / v_div_fmas /
// v_div_fixup) and `+0.0f + v` is not folded to v.  There is no multiply next to an add: nothing can contract.
//
// Indexing: numel(x) and numel(y) are below 2^31 (refused otherwise), so element indices are 32-bit unsigned, idx fits an
// int32 and the launch is one lane per element; the plane's base offset and every pointer step are formed in 64 bits.
#include <limits.h>

#include "np_internal.h"

namespace {

constexpr int kPoolBlock = 256;           // lanes per workgroup, every kernel (tests/test_gpu_dnn_pool.py mirrors both constants)
constexpr int kStageCells = 8192;         // the staged forward form: planes of at most this many cells, 32 KiB of LDS a workgroup
constexpr size_t kLim = (size_t)1 << 31;
constexpr size_t kWindowLim = (size_t)1 << 24;   // kh.kw below this: (float) divisor is exact

// np_debug_pool_last_path: 0 = none yet; forward 1 = direct, 2 = staged; backward 1 = gather
int g_pool_last_forward = 0, g_pool_last_backward = 0;
// np_debug_pool_forward_form: 0 = by the extents, 1 = direct for every shape
int g_pool_force_direct = 0;

// n / d for 0 <= n < 2^31 and 1 <= d < 2^31 as one high multiply and a shift: with p = 31 + ceil(log2 d) and
// mul = ceil(2^p / d) (which fits 32 bits), mul.d - 2^p = e in [0, d), so n.mul / 2^p = n / d + n.e / (d.2^p) and
// n.e < 2^31 . 2^ceil(log2 d) = 2^p: the excess stays below 1 / d and the floor is the quotient.  d = 1 passes n through.
// Both kernels decode their lane's index with these: an integer division is some thirty instructions, and a pooling lane
// has only a handful of loads to hide them behind.
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

struct PoolArgs {
    int H, W, kh, kw, ph, pw, sh, sw, oh, ow;
    unsigned numel_x, numel_y;
    FastDiv by_H, by_W, by_oh, by_ow, by_sh, by_sw;
};

// rows (or columns) of window i that lie inside the image: [lo, hi)
__device__ __forceinline__ void clip_window(int i, int s, int p, int k, int extent, int &lo, int &hi) {
    const int t = i * s - p;
    lo = t < 0 ? 0 : t;
    hi = t + k < extent ? t + k : extent;
}

// output (i, j) of the plane at xp (global memory or LDS): the scan of np_hip.h, real cells in row-major order
template <int MODE>
__device__ __forceinline__ void pool_scan(const float *xp, const PoolArgs &a, int i, int j, float &out, int &at) {
    int r_lo, r_hi, c_lo, c_hi;
    clip_window(i, a.sh, a.ph, a.kh, a.H, r_lo, r_hi);
    clip_window(j, a.sw, a.pw, a.kw, a.W, c_lo, c_hi);
    if (MODE == NP_POOL_MAX) {
        float best = -INFINITY;
        at = r_lo * a.W + c_lo;
        for (int u = r_lo; u < r_hi; ++u) {
            const float *row = xp + (size_t)u * (size_t)a.W;
            for (int v = c_lo; v < c_hi; ++v) {
                const float val = row[v];
                if (val > best || val != val) {
                    best = val;
                    at = u * a.W + v;
                }
            }
        }
        out = best;
    } else {
        float sum = 0.0f;
        for (int u = r_lo; u < r_hi; ++u) {
            const float *row = xp + (size_t)u * (size_t)a.W;
            for (int v = c_lo; v < c_hi; ++v) sum += row[v];
        }
        const int divisor = MODE == NP_POOL_AVG ? a.kh * a.kw : (r_hi - r_lo) * (c_hi - c_lo);
        out = sum / (float)divisor;
        at = 0;
    }
}

template <int MODE, bool WITH_IDX>
__global__ __launch_bounds__(kPoolBlock) void pool_fwd_direct_kernel(const float *__restrict__ x, float *__restrict__ y, int32_t *__restrict__ idx,
                                                                     const PoolArgs a) {
    const unsigned o = blockIdx.x * (unsigned)kPoolBlock + threadIdx.x;
    if (o >= a.numel_y) return;
    const unsigned t = quotient(o, a.by_ow), plane = quotient(t, a.by_oh);
    const int j = (int)(o - t * (unsigned)a.ow), i = (int)(t - plane * (unsigned)a.oh);
    float out;
    int at;
    pool_scan<MODE>(x + (size_t)plane * ((size_t)a.H * (size_t)a.W), a, i, j, out, at);
    y[o] = out;
    if (WITH_IDX) idx[o] = at;
}

// workgroup b takes planes [b.per_group, min((b + 1).per_group, planes)): per_group.H.W <= kStageCells
template <int MODE, bool WITH_IDX>
__global__ __launch_bounds__(kPoolBlock) void pool_fwd_staged_kernel(const float *__restrict__ x, float *__restrict__ y, int32_t *__restrict__ idx,
                                                                     const PoolArgs a, unsigned planes, unsigned per_group) {
    __shared__ float tile[kStageCells];
    const unsigned first = blockIdx.x * per_group, held = planes - first < per_group ? planes - first : per_group;
    const unsigned hw = (unsigned)a.H * (unsigned)a.W, ohw = (unsigned)a.oh * (unsigned)a.ow;
    const unsigned cells = held * hw, outs = held * ohw;
    const float *src = x + (size_t)first * hw;
    for (unsigned e = threadIdx.x; e < cells; e += kPoolBlock) tile[e] = src[e];
    __syncthreads();
    float *dst = y + (size_t)first * ohw;
    int32_t *dst_idx = WITH_IDX ? idx + (size_t)first * ohw : nullptr;
    for (unsigned o = threadIdx.x; o < outs; o += kPoolBlock) {
        const unsigned t = quotient(o, a.by_ow), plane = quotient(t, a.by_oh);
        const int j = (int)(o - t * (unsigned)a.ow), i = (int)(t - plane * (unsigned)a.oh);
        float out;
        int at;
        pool_scan<MODE>(tile + plane * hw, a, i, j, out, at);
        dst[o] = out;
        if (WITH_IDX) dst_idx[o] = at;
    }
}

// the windows that cover cell u along one axis: i.s - p <= u <= i.s - p + k - 1, clipped to [0, n_out); empty when lo > hi
__device__ __forceinline__ void covering(int u, const FastDiv &by_s, int p, int k, int n_out, int &lo, int &hi) {
    const int top = u + p, low = top - k + 1;
    hi = (int)quotient((unsigned)top, by_s);
    if (hi > n_out - 1) hi = n_out - 1;
    lo = low <= 0 ? 0 : (int)quotient((unsigned)(low - 1), by_s) + 1;     // ceil(low / s) without low + s, which may pass 2^31
}

template <int MODE>
__global__ __launch_bounds__(kPoolBlock) void pool_bwd_gather_kernel(const float *__restrict__ dy, const int32_t *__restrict__ idx,
                                                                     float *__restrict__ dx, const PoolArgs a) {
    const unsigned c = blockIdx.x * (unsigned)kPoolBlock + threadIdx.x;
    if (c >= a.numel_x) return;
    const unsigned t = quotient(c, a.by_W), plane = quotient(t, a.by_H);
    const int v = (int)(c - t * (unsigned)a.W), u = (int)(t - plane * (unsigned)a.H);
    int i_lo, i_hi, j_lo, j_hi;
    covering(u, a.by_sh, a.ph, a.kh, a.oh, i_lo, i_hi);
    covering(v, a.by_sw, a.pw, a.kw, a.ow, j_lo, j_hi);
    const size_t base = (size_t)plane * ((size_t)a.oh * (size_t)a.ow);
    const float *gp = dy + base;
    const int me = u * a.W + v;
    const float full = (float)(a.kh * a.kw);
    float sum = 0.0f;
    for (int i = i_lo; i <= i_hi; ++i) {
        const size_t row = (size_t)i * (size_t)a.ow;
        int rows = 0;
        if (MODE == NP_POOL_AVG_VALID) {
            int r_lo, r_hi;
            clip_window(i, a.sh, a.ph, a.kh, a.H, r_lo, r_hi);
            rows = r_hi - r_lo;
        }
        for (int j = j_lo; j <= j_hi; ++j) {
            if (MODE == NP_POOL_MAX) {
                const float term = gp[row + j];      // read whether or not it is taken: the two loads travel together
                if (idx[base + row + j] == me) sum += term;
            } else if (MODE == NP_POOL_AVG) {
                sum += gp[row + j] / full;
            } else {
                int c_lo, c_hi;
                clip_window(j, a.sw, a.pw, a.kw, a.W, c_lo, c_hi);
                sum += gp[row + j] / (float)(rows * (c_hi - c_lo));
            }
        }
    }
    dx[c] = sum;
}

// a * b, saturating at kLim (both factors at most kLim)
size_t mul_lim(size_t a, size_t b) { return (a >= kLim || b >= kLim || a * b >= kLim) ? kLim : a * b; }

// the whole shape -> the kernels' extents; oh and ow are written only when the shape is accepted.  No device is touched.
int check_pool(const char *who, size_t planes, size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, PoolArgs &a) {
    if (planes < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1)
        return np::fail(NP_ERR_INVALID, "%s: every extent, window and stride must be at least 1", who);
    if (ph > kh / 2 || pw > kw / 2)     // 2 p > k, without the product
        return np::fail(NP_ERR_INVALID, "%s: the padding (%zu, %zu) must be at most half the window (%zu, %zu)", who, ph, pw, kh, kw);
    if (kh - 2 * ph > H || kw - 2 * pw > W)     // k > extent + 2 p, without the sum
        return np::fail(NP_ERR_INVALID, "%s: the window (%zu, %zu) is larger than the padded image (H + 2 ph, W + 2 pw)", who, kh, kw);
    if (kh >= kWindowLim || kw >= kWindowLim || kh * kw >= kWindowLim)
        return np::fail(NP_ERR_INVALID, "%s: the window (%zu, %zu) has 2^24 cells or more", who, kh, kw);
    // from here ph, pw < 2^23.  The kernels form i.sh - ph + kh and u.W + v as ints
    const size_t hw = mul_lim(H, W), numel_x = mul_lim(planes, hw);
    if (hw >= kLim || numel_x >= kLim || sh >= kLim || sw >= kLim || H + 2 * ph >= kLim || W + 2 * pw >= kLim)
        return np::fail(NP_ERR_INVALID, "%s: H.W, numel(x), a stride or a padded extent is 2^31 or more", who);
    const size_t oh = (H + 2 * ph - kh) / sh + 1, ow = (W + 2 * pw - kw) / sw + 1;
    const size_t numel_y = mul_lim(planes, mul_lim(oh, ow));
    if (numel_y >= kLim) return np::fail(NP_ERR_INVALID, "%s: numel(y) is 2^31 or more", who);
    a.H = (int)H, a.W = (int)W, a.kh = (int)kh, a.kw = (int)kw, a.ph = (int)ph, a.pw = (int)pw, a.sh = (int)sh, a.sw = (int)sw;
    a.oh = (int)oh, a.ow = (int)ow, a.numel_x = (unsigned)numel_x, a.numel_y = (unsigned)numel_y;
    a.by_H = fast_div((unsigned)H), a.by_W = fast_div((unsigned)W), a.by_oh = fast_div((unsigned)oh), a.by_ow = fast_div((unsigned)ow);
    a.by_sh = fast_div((unsigned)sh), a.by_sw = fast_div((unsigned)sw);
    return NP_OK;
}

bool known_mode(int mode) { return mode == NP_POOL_MAX || mode == NP_POOL_AVG || mode == NP_POOL_AVG_VALID; }

template <int MODE, bool WITH_IDX>
void launch_forward_as(bool staged, const float *x, float *y, int32_t *idx, const PoolArgs &a, unsigned planes) {
    if (staged) {
        const unsigned per_group = (unsigned)kStageCells / ((unsigned)a.H * (unsigned)a.W);
        const dim3 grid((planes + per_group - 1) / per_group);
        pool_fwd_staged_kernel<MODE, WITH_IDX><<<grid, dim3(kPoolBlock), 0, np::stream()>>>(x, y, idx, a, planes, per_group);
    } else {
        const dim3 grid((a.numel_y + kPoolBlock - 1) / kPoolBlock);
        pool_fwd_direct_kernel<MODE, WITH_IDX><<<grid, dim3(kPoolBlock), 0, np::stream()>>>(x, y, idx, a);
    }
}

int launch_forward(const float *x, float *y, int32_t *idx, const PoolArgs &a, unsigned planes, int mode) {
    const bool staged = !g_pool_force_direct && (size_t)a.H * (size_t)a.W <= (size_t)kStageCells;
    if (mode == NP_POOL_MAX && idx) launch_forward_as<NP_POOL_MAX, true>(staged, x, y, idx, a, planes);
    else if (mode == NP_POOL_MAX) launch_forward_as<NP_POOL_MAX, false>(staged, x, y, nullptr, a, planes);
    else if (mode == NP_POOL_AVG) launch_forward_as<NP_POOL_AVG, false>(staged, x, y, nullptr, a, planes);
    else launch_forward_as<NP_POOL_AVG_VALID, false>(staged, x, y, nullptr, a, planes);
    NP_LAUNCH_CHECK(staged ? "pool_fwd_staged_kernel" : "pool_fwd_direct_kernel");
    g_pool_last_forward = staged ? 2 : 1;
    return NP_OK;
}

int launch_backward(const float *dy, const int32_t *idx, float *dx, const PoolArgs &a, int mode) {
    const dim3 grid((a.numel_x + kPoolBlock - 1) / kPoolBlock), block(kPoolBlock);
    if (mode == NP_POOL_MAX) pool_bwd_gather_kernel<NP_POOL_MAX><<<grid, block, 0, np::stream()>>>(dy, idx, dx, a);
    else if (mode == NP_POOL_AVG) pool_bwd_gather_kernel<NP_POOL_AVG><<<grid, block, 0, np::stream()>>>(dy, nullptr, dx, a);
    else pool_bwd_gather_kernel<NP_POOL_AVG_VALID><<<grid, block, 0, np::stream()>>>(dy, nullptr, dx, a);
    NP_LAUNCH_CHECK("pool_bwd_gather_kernel");
    g_pool_last_backward = 1;
    return NP_OK;
}

}  // namespace

extern "C" {

int np_pool2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t *oh, size_t *ow) {
    if (!oh || !ow) return np::fail(NP_ERR_INVALID, "np_pool2d_shape: null pointer");
    PoolArgs a = {};
    if (int rc = check_pool("np_pool2d_shape", 1, H, W, kh, kw, ph, pw, sh, sw, a)) return rc;
    *oh = (size_t)a.oh;
    *ow = (size_t)a.ow;
    return NP_OK;
}

// The order is the pointers, the shape, the mode, ensure_init, then work: a refused call has touched no device.
int np_pool2d_forward(const float *x, size_t planes, size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw,
                      int mode, float *y, int32_t *idx) {
    if (!x || !y) return np::fail(NP_ERR_INVALID, "np_pool2d_forward: null pointer");
    PoolArgs a = {};
    if (int rc = check_pool("np_pool2d_forward", planes, H, W, kh, kw, ph, pw, sh, sw, a)) return rc;
    if (!known_mode(mode)) return np::fail(NP_ERR_INVALID, "np_pool2d_forward: unknown mode %d", mode);
    if (int rc = np::ensure_init()) return rc;
    return launch_forward(x, y, idx, a, (unsigned)planes, mode);
}

int np_pool2d_backward(const float *dy, const int32_t *idx, size_t planes, size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw,
                       size_t sh, size_t sw, int mode, float *dx) {
    if (!dy || !dx) return np::fail(NP_ERR_INVALID, "np_pool2d_backward: null pointer");
    if (mode == NP_POOL_MAX && !idx) return np::fail(NP_ERR_INVALID, "np_pool2d_backward: null pointer: the max mode needs idx");
    PoolArgs a = {};
    if (int rc = check_pool("np_pool2d_backward", planes, H, W, kh, kw, ph, pw, sh, sw, a)) return rc;
    if (!known_mode(mode)) return np::fail(NP_ERR_INVALID, "np_pool2d_backward: unknown mode %d", mode);
    if (int rc = np::ensure_init()) return rc;
    return launch_backward(dy, idx, dx, a, mode);
}

int np_debug_pool_forward_form(int form) {
    if (form != 0 && form != 1) return np::fail(NP_ERR_INVALID, "np_debug_pool_forward_form: form must be 0 (by the extents) or 1 (direct)");
    g_pool_force_direct = form;
    return NP_OK;
}

int np_debug_pool_last_path(int *forward_form, int *backward_form) {
    if (!forward_form || !backward_form) return np::fail(NP_ERR_INVALID, "np_debug_pool_last_path: null pointer");
    *forward_form = g_pool_last_forward;
    *backward_form = g_pool_last_backward;
    return NP_OK;
}

}  // extern "C"
