// Softmax, log-softmax and cross-entropy for GPU arrays: np_softmax_forward, np_softmax_backward,
// np_cross_entropy.  The rules are in np_hip.h; this comment says how the kernels keep them.
//
// The operand is (outer, cols, inner), contiguous fp32; the softmax runs over cols.  Every kernel is built from the same
// pieces, so that a value has the same bits wherever the same form computes it:
//   row statistics   m = the maximum (a NaN never wins: `b > a ? b : a` from -Inf), s = the sum of fast_exp(x - m).
//   element values   fwd_value / bwd_value / grad_value below, each evaluated from the INPUT element and the row's statistics
//                    when the element is written: no e_i is kept between the sum and the output, fast_exp(x - m) is simply
//                    evaluated again (the same instruction sequence, the same bits).  The kernels move 8 bytes per element
//                    and have some hundred lane-instructions per element to spend at the copy rate; two fast_exp are 20.
// Special values need no branch: a NaN, or +Inf - +Inf, or -Inf - -Inf, makes some d_i NaN, so s is NaN and every element
// of the row divides by it or subtracts its logarithm.  Lanes past the end of a row hold -Inf (fast_exp gives +0.0f, which
// changes no sum that started from +0.0f) or, in the backward sums, +0.0f.
//
// Five forms, chosen from (cols, inner) alone (pick_form) and reported by np_debug_softmax_last_path:
//   1 SHORT    inner == 1, cols <= kShortMaxCols.  A workgroup copies a slab of R = min(kSlabRowsMax, kSlabFloats / (cols | 1))
//              whole rows, one contiguous run, into LDS with float4 loads (scalar up to the first 16-byte boundary and after the
//              last), row pitch cols | 1 words so that lanes one row apart sit on different banks.  Lane r owns row r: three
//              serial walks in ascending column order.  The result overwrites the slab and goes out as the run came in.
//   2 WAVE     inner == 1, cols <= kWaveMaxCols.  A wave per row, four rows a workgroup, the row in registers: lane l holds
//              the float4 groups l, l + 64, ... (NV of them, NV = 1, 2, 4 by cols).  A 16-byte aligned row is read with
//              float4 loads, any other row with four dword loads per group into the SAME registers: the order of every sum
//              is the same.  Per lane a chain in ascending register order, then a xor butterfly (32, 16, ... 1).
//   3 BLOCK    inner == 1, cols <= kBlockMaxCols.  The same with a workgroup per row: 256 lanes with NV = 2, 4, 8 up to 8192
//              columns, 1024 lanes with NV = 4, 8 above.  Waves join through LDS, wave 0 first.  32 floats a lane at
//              1024 lanes is 128 KiB of registers for the row: a workgroup of 16 waves at 95 - 128 VGPRs, so ONE workgroup per
//              CU (4 waves per SIMD): its loads, its two joins and its stores do not overlap another row's.  The
//              probability-target kernel with 32 floats a lane is the one kernel that spills (168 bytes a lane).
//   4 STREAM   inner == 1, any cols: one workgroup of 1024 lanes per row, two reads and one write.  Pass 1 keeps a running
//              maximum and a rescaled sum per lane over chunks of kChunk elements (online_add), the lanes' pairs are joined
//              once; pass 2 reads the row again and writes.
//   5 STRIDED  inner > 1: a lane owns one (outer, inner) column, lanes adjacent along inner, so every access of a wave is one
//              contiguous run.  The same running pair over chunks of kChunk elements along cols, then a second walk.
// A row is never split over workgroups: few rows of 10^7 columns use as many CUs as there are rows.
//
// Indexing: cols < 2^31 (refused otherwise); every row offset is formed in size_t, so outer.cols.inner may pass 2^31.  Every
// kernel walks its rows (slabs, columns) with a grid-stride loop, the grid capped at kMaxGrid workgroups.
// The unit includes np_elementwise_ops.h for fast_exp: fp contraction is off, every multiply and add is rounded on its own,
// and `/` is the correctly rounded division.
#include <float.h>

#include "np_elementwise_ops.h"

namespace {

constexpr unsigned kShortMaxCols = 64;      // form boundaries (np_debug_softmax_bounds reports them; tests/test_gpu_softmax.py reads them)
constexpr unsigned kWaveMaxCols = 1024;
constexpr unsigned kBlockMaxCols = 32768;
constexpr unsigned kSlabFloats = 8192;      // SHORT: LDS words per operand slab (32 KiB; two operands at most)
constexpr unsigned kSlabRowsMax = 256;      // SHORT: rows per slab at most, one per lane
constexpr unsigned kMaxGrid = 1u << 20;
constexpr int kChunk = 8;                   // STREAM / STRIDED: elements per running-maximum step
constexpr int kNumBounds = 5;
constexpr size_t kColsLim = (size_t)1 << 31;

enum { FORM_SHORT = 1, FORM_WAVE = 2, FORM_BLOCK = 3, FORM_STREAM = 4, FORM_STRIDED = 5 };
enum { OP_FWD = 0, OP_BWD = 1, OP_XENT = 2 };

int g_smx_last_form = 0;    // np_debug_softmax_last_path
int g_smx_force_form = -1;  // np_debug_softmax_force_form

struct SmxArgs {
    const float *a;   // x | y | logits
    const float *b;   // - | dy | target
    float *out;       // y | dx | dlogits (nullptr: no gradient)
    float *loss;      // cross-entropy only
    size_t rows;      // outer; the rows of the cross-entropy
    unsigned cols;
    size_t inner;
    int mode;         // np_softmax_mode | np_xent_target
    float scale;
};

// ---- element values: every form writes through these ----
__device__ __forceinline__ float row_max(float a, float b) { return np::dev::r_combine<NP_MAX>(a, b); }
// k = s (softmax) or logf(s) (log-softmax)
__device__ __forceinline__ float fwd_value(float x, float m, float k, int mode) {
    const float d = x - m;
    return mode == NP_SOFTMAX ? __fdiv_rn(fast_exp(d), k) : d - k;
}
__device__ __forceinline__ float fwd_norm(float s, int mode) { return mode == NP_SOFTMAX ? s : logf(s); }
// the term of the backward sum, and dx from the finished sum t
__device__ __forceinline__ float bwd_term(float y, float dy, int mode) { return mode == NP_SOFTMAX ? dy * y : dy; }
__device__ __forceinline__ float bwd_value(float y, float dy, float t, int mode) {
    return mode == NP_SOFTMAX ? y * (dy - t) : dy - fast_exp(y) * t;
}
__device__ __forceinline__ float grad_value(float x, float m, float s, float t, float scale) {
    return (__fdiv_rn(fast_exp(x - m), s) - t) * scale;
}
// a class index stored as fp32: an integer in [0, cols).  A NaN fails the first comparison.
__device__ __forceinline__ bool label_of(float f, unsigned cols, unsigned &li) {
    if (!(f >= 0.0f && f < 2147483648.0f)) return false;
    const unsigned i = (unsigned)f;
    if ((float)i != f || i >= cols) return false;   // li keeps its in-range value: nothing is read out of bounds
    li = i;
    return true;
}
// the target of column c for an index row: the one-hot of the label, NaN everywhere for an invalid label
__device__ __forceinline__ float onehot(bool valid, unsigned li, unsigned c) { return valid ? (c == li ? 1.0f : 0.0f) : NAN; }
// one term of the probability-target loss; t == 0 is skipped by the caller
__device__ __forceinline__ float prob_term(float t, float x, float m, float ls) { return t * (ls - (x - m)); }

// ---- the running pair of STREAM and STRIDED ----
// s is the sum of fast_exp(x - ref(m)) over what has been seen, ref(m) = m floored at -FLT_MAX: before the first finite
// element the reference is finite, so -Inf elements add +0.0f instead of fast_exp(-Inf + Inf).  A chunk raises the maximum at
// most once: s is multiplied by ONE fast_exp of the step, then the chunk's own chain from +0.0f is added.
struct Online {
    float m, s;
};
__device__ __forceinline__ float floor_ref(float m) { return m > -FLT_MAX ? m : -FLT_MAX; }
__device__ __forceinline__ void online_add(Online &o, const float (&x)[kChunk]) {
    float cm = -INFINITY;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) cm = row_max(cm, x[i]);
    if (cm > o.m) {
        o.s = o.s * fast_exp(floor_ref(o.m) - floor_ref(cm));
        o.m = cm;
    }
    const float ref = floor_ref(o.m);
    float c = 0.0f;
#pragma unroll
    for (int i = 0; i < kChunk; ++i) c += fast_exp(x[i] - ref);
    o.s += c;
}

// ---- joins ----
// all lanes of the group (WAVES waves) get the same bits; part: WAVES words of LDS
template <int WAVES>
__device__ __forceinline__ float group_sum(float v, float *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (WAVES > 1) {
        __syncthreads();   // the previous join's readers are done with part
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
        __syncthreads();
        v = part[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += part[w];
    }
    return v;
}
template <int WAVES>
__device__ __forceinline__ float group_max(float v, float *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = row_max(v, __shfl_xor(v, off, 64));
    v = __shfl(v, 0, 64);   // -0.0 and +0.0 compare equal: one lane's choice for the whole wave
    if (WAVES > 1) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
        __syncthreads();
        v = part[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v = row_max(v, part[w]);
    }
    return v;
}

// ---- float4 groups of a row: group v holds elements 4v .. 4v + 3.  An aligned pointer and a whole group: one 16-byte
// access; otherwise element by element into the same places.
__device__ __forceinline__ void load_group(const float *p, bool aligned, unsigned e0, unsigned cols, float fill, float *x) {
    if (aligned && e0 + 3 < cols) {
        const v4f a = *(const v4f *)(p + e0);
        x[0] = a[0], x[1] = a[1], x[2] = a[2], x[3] = a[3];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = e0 + i < cols ? p[e0 + i] : fill;
    }
}
__device__ __forceinline__ void store_group(float *p, bool aligned, unsigned e0, unsigned cols, const float *x) {
    if (aligned && e0 + 3 < cols) {
        v4f a;
        a[0] = x[0], a[1] = x[1], a[2] = x[2], a[3] = x[3];
        *(v4f *)(p + e0) = a;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (e0 + i < cols) p[e0 + i] = x[i];
    }
}
__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- SHORT ----
// e / cols for e < 2^16 (magic = ceil(2^32 / cols); cols == 1 passes e through)
__device__ __forceinline__ unsigned slab_row(unsigned e, unsigned cols, unsigned magic) { return cols == 1 ? e : __umulhi(e, magic); }

// a contiguous run of `total` words <-> a slab of rows at `pitch`
template <bool IN>
__device__ __forceinline__ void slab_copy(float *slab, const float *src, float *dst, unsigned total, unsigned cols, unsigned pitch,
                                          unsigned magic) {
    const uintptr_t addr = IN ? (uintptr_t)src : (uintptr_t)dst;
    unsigned head = (unsigned)(((16u - (unsigned)(addr & 15u)) & 15u) / 4u);
    if (head > total) head = total;
    const unsigned nvec = (total - head) / 4;
    if (threadIdx.x < head) {
        const unsigned r = slab_row(threadIdx.x, cols, magic), at = r * pitch + (threadIdx.x - r * cols);
        if (IN) slab[at] = src[threadIdx.x];
        else dst[threadIdx.x] = slab[at];
    }
    for (unsigned v = threadIdx.x; v < nvec; v += blockDim.x) {
        const unsigned e = head + v * 4;
        unsigned r = slab_row(e, cols, magic), c = e - r * cols;
        v4f a;
        if (IN) a = *(const v4f *)(src + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (IN) slab[r * pitch + c] = a[k];
            else a[k] = slab[r * pitch + c];
            if (++c == cols) c = 0, ++r;
        }
        if (!IN) *(v4f *)(dst + e) = a;
    }
    for (unsigned e = head + nvec * 4 + threadIdx.x; e < total; e += blockDim.x) {
        const unsigned r = slab_row(e, cols, magic), at = r * pitch + (e - r * cols);
        if (IN) slab[at] = src[e];
        else dst[e] = slab[at];
    }
}

template <int OP>
__global__ __launch_bounds__(256) void smx_short_kernel(const SmxArgs g, unsigned R, unsigned magic) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned cols = g.cols, pitch = cols | 1u;
    const bool two = OP == OP_BWD || (OP == OP_XENT && g.mode == NP_XENT_PROB);
    float *sa = lds, *sb = lds + R * pitch;
    float *so = OP == OP_BWD ? sb : sa;   // the slab the result overwrites
    const size_t nslabs = (g.rows + R - 1) / R;
    for (size_t sl = blockIdx.x; sl < nslabs; sl += gridDim.x) {
        const size_t row0 = sl * R, off = row0 * cols;
        const unsigned rows = (unsigned)(g.rows - row0 < R ? g.rows - row0 : R), total = rows * cols;
        slab_copy<true>(sa, g.a + off, nullptr, total, cols, pitch, magic);
        if (two) slab_copy<true>(sb, g.b + off, nullptr, total, cols, pitch, magic);
        __syncthreads();
        if (threadIdx.x < rows) {
            float *p = sa + threadIdx.x * pitch, *q = sb + threadIdx.x * pitch;
            if (OP == OP_BWD) {
                float t = 0.0f;
                for (unsigned c = 0; c < cols; ++c) t += bwd_term(p[c], q[c], g.mode);
                for (unsigned c = 0; c < cols; ++c) q[c] = bwd_value(p[c], q[c], t, g.mode);
            } else {
                float m = -INFINITY, s = 0.0f;
                for (unsigned c = 0; c < cols; ++c) m = row_max(m, p[c]);
                for (unsigned c = 0; c < cols; ++c) s += fast_exp(p[c] - m);
                if (OP == OP_FWD) {
                    const float k = fwd_norm(s, g.mode);
                    for (unsigned c = 0; c < cols; ++c) p[c] = fwd_value(p[c], m, k, g.mode);
                } else {
                    const float ls = logf(s);
                    float loss = 0.0f;
                    if (g.mode == NP_XENT_INDEX) {
                        unsigned li = 0;
                        const bool valid = label_of(g.b[row0 + threadIdx.x], cols, li);
                        loss = valid ? ls - (p[li] - m) : NAN;
                        if (g.out)
                            for (unsigned c = 0; c < cols; ++c) p[c] = grad_value(p[c], m, s, onehot(valid, li, c), g.scale);
                    } else {
                        for (unsigned c = 0; c < cols; ++c)
                            if (q[c] != 0.0f) loss += prob_term(q[c], p[c], m, ls);
                        if (g.out)
                            for (unsigned c = 0; c < cols; ++c) p[c] = grad_value(p[c], m, s, q[c], g.scale);
                    }
                    g.loss[row0 + threadIdx.x] = loss;
                }
            }
        }
        __syncthreads();
        if (g.out) slab_copy<false>(so, nullptr, g.out + off, total, cols, pitch, magic);
        __syncthreads();   // the next slab overwrites what is being read
    }
}

// ---- WAVE (WAVES == 1, four rows a workgroup) and BLOCK (WAVES == 4 or 16, one row a workgroup) ----
// KIND: the target kind of a cross-entropy, known at compile time so that the index kernels carry no target registers
template <int OP, int NV, int WAVES, int KIND>
__global__ __launch_bounds__(WAVES == 1 ? 256 : WAVES * 64) void smx_reg_kernel(const SmxArgs g) {
    __shared__ float part[WAVES];
    constexpr unsigned G = WAVES * 64, RPB = WAVES == 1 ? 4 : 1;
    const unsigned gl = WAVES == 1 ? (threadIdx.x & 63u) : threadIdx.x, cols = g.cols;
    const size_t nblk = (g.rows + RPB - 1) / RPB;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t row = blk * RPB + (WAVES == 1 ? threadIdx.x >> 6 : 0);
        if (WAVES == 1 && row >= g.rows) continue;   // a whole wave; the wave form has no barrier
        const size_t off = row * cols;
        const float *pa = g.a + off;
        const bool al_a = aligned16(pa);
        float x[NV * 4];
#pragma unroll
        for (int k = 0; k < NV; ++k) load_group(pa, al_a, (k * G + gl) * 4, cols, OP == OP_BWD ? 0.0f : -INFINITY, x + 4 * k);
        if (OP == OP_BWD) {
            const float *pb = g.b + off;
            const bool al_b = aligned16(pb);
            float dy[NV * 4];
#pragma unroll
            for (int k = 0; k < NV; ++k) load_group(pb, al_b, (k * G + gl) * 4, cols, 0.0f, dy + 4 * k);
            float t = 0.0f;
#pragma unroll
            for (int i = 0; i < NV * 4; ++i) t += bwd_term(x[i], dy[i], g.mode);
            t = group_sum<WAVES>(t, part);
#pragma unroll
            for (int i = 0; i < NV * 4; ++i) dy[i] = bwd_value(x[i], dy[i], t, g.mode);
            float *po = g.out + off;
            const bool al_o = aligned16(po);
#pragma unroll
            for (int k = 0; k < NV; ++k) store_group(po, al_o, (k * G + gl) * 4, cols, dy + 4 * k);
            continue;
        }
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NV * 4; ++i) m = row_max(m, x[i]);
        m = group_max<WAVES>(m, part);
        const bool keep_e = OP == OP_FWD && g.mode == NP_SOFTMAX;   // the row is in registers: e_i stays where x_i was
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < NV * 4; ++i) {
            const float e = fast_exp(x[i] - m);
            s += e;
            if (keep_e) x[i] = e;
        }
        s = group_sum<WAVES>(s, part);
        float *po = g.out ? g.out + off : nullptr;
        const bool al_o = aligned16(po);
        if (OP == OP_FWD) {
            if (keep_e) {
#pragma unroll
                for (int i = 0; i < NV * 4; ++i) x[i] = __fdiv_rn(x[i], s);   // fwd_value's quotient of the same e_i
            } else {
                const float k = fwd_norm(s, g.mode);
#pragma unroll
                for (int i = 0; i < NV * 4; ++i) x[i] = fwd_value(x[i], m, k, g.mode);
            }
        } else {
            const float ls = logf(s);
            float loss;
            if (KIND == NP_XENT_INDEX) {
                unsigned li = 0;
                const bool valid = label_of(g.b[row], cols, li);
                loss = valid ? ls - (pa[li] - m) : NAN;
                if (po) {
#pragma unroll
                    for (int k = 0; k < NV; ++k)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            x[4 * k + i] = grad_value(x[4 * k + i], m, s, onehot(valid, li, (k * G + gl) * 4 + i), g.scale);
                }
            } else {
                const float *pb = g.b + off;
                const bool al_b = aligned16(pb);
                float t[NV * 4];
#pragma unroll
                for (int k = 0; k < NV; ++k) load_group(pb, al_b, (k * G + gl) * 4, cols, 0.0f, t + 4 * k);
                loss = 0.0f;
#pragma unroll
                for (int i = 0; i < NV * 4; ++i)
                    if (t[i] != 0.0f) loss += prob_term(t[i], x[i], m, ls);
                loss = group_sum<WAVES>(loss, part);
                if (po) {
#pragma unroll
                    for (int i = 0; i < NV * 4; ++i) x[i] = grad_value(x[i], m, s, t[i], g.scale);
                }
            }
            if (gl == 0) g.loss[row] = loss;
        }
        if (po) {
#pragma unroll
            for (int k = 0; k < NV; ++k) store_group(po, al_o, (k * G + gl) * 4, cols, x + 4 * k);
        }
    }
}

// ---- STREAM: one workgroup of 1024 lanes per row ----
constexpr int kStreamWaves = 16;
constexpr unsigned kStreamLanes = kStreamWaves * 64;
constexpr unsigned kStreamStep = kStreamLanes * kChunk;   // elements a pass of the workgroup covers

template <int OP>
__global__ __launch_bounds__(kStreamLanes) void smx_stream_kernel(const SmxArgs g) {
    __shared__ float part[kStreamWaves];
    const unsigned cols = g.cols, gl = threadIdx.x;
    for (size_t row = blockIdx.x; row < g.rows; row += gridDim.x) {
        const size_t off = row * cols;
        const float *pa = g.a + off, *pb = (OP == OP_BWD || (OP == OP_XENT && g.mode == NP_XENT_PROB)) ? g.b + off : nullptr;
        float *po = g.out ? g.out + off : nullptr;
        const bool al_a = aligned16(pa), al_b = aligned16(pb), al_o = aligned16(po);
        // lane gl takes the groups (2 it) . 1024 + gl and (2 it + 1) . 1024 + gl of every step
        if (OP == OP_BWD) {
            float t = 0.0f;
            for (unsigned base = 0; base < cols; base += kStreamStep) {
                float y[kChunk], dy[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk / 4; ++u) {
                    load_group(pa, al_a, base + (u * kStreamLanes + gl) * 4, cols, 0.0f, y + 4 * u);
                    load_group(pb, al_b, base + (u * kStreamLanes + gl) * 4, cols, 0.0f, dy + 4 * u);
                }
#pragma unroll
                for (int i = 0; i < kChunk; ++i) t += bwd_term(y[i], dy[i], g.mode);
            }
            t = group_sum<kStreamWaves>(t, part);
            for (unsigned base = 0; base < cols; base += kStreamStep) {
                float y[kChunk], dy[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk / 4; ++u) {
                    load_group(pa, al_a, base + (u * kStreamLanes + gl) * 4, cols, 0.0f, y + 4 * u);
                    load_group(pb, al_b, base + (u * kStreamLanes + gl) * 4, cols, 0.0f, dy + 4 * u);
                }
#pragma unroll
                for (int i = 0; i < kChunk; ++i) dy[i] = bwd_value(y[i], dy[i], t, g.mode);
#pragma unroll
                for (int u = 0; u < kChunk / 4; ++u) store_group(po, al_o, base + (u * kStreamLanes + gl) * 4, cols, dy + 4 * u);
            }
            continue;
        }
        Online o = {-INFINITY, 0.0f};
        for (unsigned base = 0; base < cols; base += kStreamStep) {
            float x[kChunk];
#pragma unroll
            for (int u = 0; u < kChunk / 4; ++u) load_group(pa, al_a, base + (u * kStreamLanes + gl) * 4, cols, -INFINITY, x + 4 * u);
            online_add(o, x);
        }
        const float m = group_max<kStreamWaves>(o.m, part);
        const float s = group_sum<kStreamWaves>(o.s * fast_exp(floor_ref(o.m) - floor_ref(m)), part);
        if (OP == OP_FWD) {
            const float k = fwd_norm(s, g.mode);
            for (unsigned base = 0; base < cols; base += kStreamStep) {
                float x[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk / 4; ++u) load_group(pa, al_a, base + (u * kStreamLanes + gl) * 4, cols, -INFINITY, x + 4 * u);
#pragma unroll
                for (int i = 0; i < kChunk; ++i) x[i] = fwd_value(x[i], m, k, g.mode);
#pragma unroll
                for (int u = 0; u < kChunk / 4; ++u) store_group(po, al_o, base + (u * kStreamLanes + gl) * 4, cols, x + 4 * u);
            }
        } else {
            const float ls = logf(s);
            const bool index = g.mode == NP_XENT_INDEX;
            unsigned li = 0;
            const bool valid = index && label_of(g.b[row], cols, li);
            float loss = 0.0f;
            if (po || !index) {
                for (unsigned base = 0; base < cols; base += kStreamStep) {
                    float x[kChunk], t[kChunk];
#pragma unroll
                    for (int u = 0; u < kChunk / 4; ++u) {
                        const unsigned e0 = base + (u * kStreamLanes + gl) * 4;
                        load_group(pa, al_a, e0, cols, -INFINITY, x + 4 * u);
                        if (index) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) t[4 * u + i] = onehot(valid, li, e0 + i);
                        } else {
                            load_group(pb, al_b, e0, cols, 0.0f, t + 4 * u);
                        }
                    }
                    if (!index) {
#pragma unroll
                        for (int i = 0; i < kChunk; ++i)
                            if (t[i] != 0.0f) loss += prob_term(t[i], x[i], m, ls);
                    }
                    if (po) {
#pragma unroll
                        for (int i = 0; i < kChunk; ++i) x[i] = grad_value(x[i], m, s, t[i], g.scale);
#pragma unroll
                        for (int u = 0; u < kChunk / 4; ++u) store_group(po, al_o, base + (u * kStreamLanes + gl) * 4, cols, x + 4 * u);
                    }
                }
            }
            if (index) loss = valid ? ls - (pa[li] - m) : NAN;
            else loss = group_sum<kStreamWaves>(loss, part);
            if (gl == 0) g.loss[row] = loss;
        }
    }
}

// ---- STRIDED: a lane per (outer, inner) column ----
template <int OP>
__global__ __launch_bounds__(256) void smx_strided_kernel(const SmxArgs g) {
    const size_t n = g.rows * g.inner, inner = g.inner;
    const unsigned cols = g.cols;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (size_t)gridDim.x * 256) {
        const size_t o = idx / inner, base = o * cols * inner + (idx - o * inner);
        const float *pa = g.a + base;
        float *po = g.out + base;
        if (OP == OP_BWD) {
            const float *pb = g.b + base;
            float t = 0.0f;
            for (unsigned j0 = 0; j0 < cols; j0 += kChunk) {
                float y[kChunk], dy[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    y[u] = j0 + u < cols ? pa[(size_t)(j0 + u) * inner] : 0.0f;
                    dy[u] = j0 + u < cols ? pb[(size_t)(j0 + u) * inner] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < kChunk; ++u) t += bwd_term(y[u], dy[u], g.mode);
            }
            for (unsigned j = 0; j < cols; ++j) po[(size_t)j * inner] = bwd_value(pa[(size_t)j * inner], pb[(size_t)j * inner], t, g.mode);
        } else {
            Online on = {-INFINITY, 0.0f};
            for (unsigned j0 = 0; j0 < cols; j0 += kChunk) {
                float x[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk; ++u) x[u] = j0 + u < cols ? pa[(size_t)(j0 + u) * inner] : -INFINITY;
                online_add(on, x);
            }
            const float k = fwd_norm(on.s, g.mode);
            for (unsigned j = 0; j < cols; ++j) po[(size_t)j * inner] = fwd_value(pa[(size_t)j * inner], on.m, k, g.mode);
        }
    }
}

// ---- host ----
bool serves(int form, unsigned cols, size_t inner, bool xent) {
    switch (form) {
    case FORM_SHORT: return inner == 1 && cols <= kShortMaxCols;
    case FORM_WAVE: return inner == 1 && cols <= kWaveMaxCols;
    case FORM_BLOCK: return inner == 1 && cols <= kBlockMaxCols;
    case FORM_STREAM: return inner == 1;
    case FORM_STRIDED: return !xent;
    default: return false;
    }
}

// the form comes from (cols, inner) alone, and from the A-B switch
int pick_form(const char *who, unsigned cols, size_t inner, bool xent, int &form) {
    form = inner > 1 ? FORM_STRIDED : cols <= kShortMaxCols ? FORM_SHORT : cols <= kWaveMaxCols ? FORM_WAVE : cols <= kBlockMaxCols ? FORM_BLOCK : FORM_STREAM;
    if (g_smx_force_form < 0) return NP_OK;
    if (!serves(g_smx_force_form, cols, inner, xent))
        return np::fail(NP_ERR_INVALID, "%s: the forced form %d cannot serve cols = %u, inner = %zu", who, g_smx_force_form, cols, inner);
    form = g_smx_force_form;
    return NP_OK;
}

unsigned grid_of(size_t blocks) { return (unsigned)(blocks < kMaxGrid ? (blocks < 1 ? 1 : blocks) : kMaxGrid); }

template <int OP, int NV, int WAVES>
void launch_reg(const SmxArgs &g) {
    constexpr unsigned rpb = WAVES == 1 ? 4 : 1;
    const dim3 grid(grid_of((g.rows + rpb - 1) / rpb)), block(WAVES == 1 ? 256 : WAVES * 64);
    if constexpr (OP == OP_XENT) {
        if (g.mode == NP_XENT_PROB) {
            smx_reg_kernel<OP, NV, WAVES, NP_XENT_PROB><<<grid, block, 0, np::stream()>>>(g);
            return;
        }
    }
    smx_reg_kernel<OP, NV, WAVES, NP_XENT_INDEX><<<grid, block, 0, np::stream()>>>(g);
}

template <int OP>
int launch(int form, const SmxArgs &g) {
    const unsigned cols = g.cols;
    switch (form) {
    case FORM_SHORT: {
        const unsigned pitch = cols | 1u, fit = kSlabFloats / pitch, R = fit < kSlabRowsMax ? fit : kSlabRowsMax;
        const unsigned magic = cols == 1 ? 0u : (unsigned)((((uint64_t)1 << 32) + cols - 1) / cols);
        const bool two = OP == OP_BWD || (OP == OP_XENT && g.mode == NP_XENT_PROB);
        const size_t lds = (size_t)(two ? 2 : 1) * R * pitch * sizeof(float);
        smx_short_kernel<OP><<<grid_of((g.rows + R - 1) / R), 256, lds, np::stream()>>>(g, R, magic);
        NP_LAUNCH_CHECK("smx_short_kernel");
        break;
    }
    case FORM_WAVE:
        if (cols <= 256) launch_reg<OP, 1, 1>(g);
        else if (cols <= 512) launch_reg<OP, 2, 1>(g);
        else launch_reg<OP, 4, 1>(g);
        NP_LAUNCH_CHECK("smx_reg_kernel (wave)");
        break;
    case FORM_BLOCK:
        if (cols <= 2048) launch_reg<OP, 2, 4>(g);
        else if (cols <= 4096) launch_reg<OP, 4, 4>(g);
        else if (cols <= 8192) launch_reg<OP, 8, 4>(g);
        else if (cols <= 16384) launch_reg<OP, 4, 16>(g);
        else launch_reg<OP, 8, 16>(g);
        NP_LAUNCH_CHECK("smx_reg_kernel (block)");
        break;
    case FORM_STREAM:
        smx_stream_kernel<OP><<<grid_of(g.rows), kStreamLanes, 0, np::stream()>>>(g);
        NP_LAUNCH_CHECK("smx_stream_kernel");
        break;
    default:
        if (OP == OP_XENT) return np::fail(NP_ERR_INVALID, "np_cross_entropy: no strided form");
        smx_strided_kernel<OP == OP_XENT ? OP_FWD : OP><<<grid_of((g.rows * g.inner + 255) / 256), 256, 0, np::stream()>>>(g);
        NP_LAUNCH_CHECK("smx_strided_kernel");
        break;
    }
    g_smx_last_form = form;
    return NP_OK;
}

// the extents of a call; numel is written when they are accepted.  No device is touched.
int check_extents(const char *who, size_t outer, size_t cols, size_t inner, size_t &numel) {
    if (outer < 1 || cols < 1 || inner < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (cols >= kColsLim) return np::fail(NP_ERR_INVALID, "%s: cols = %zu is 2^31 or more", who, cols);
    const size_t lim = SIZE_MAX / sizeof(float);
    if (outer > lim / cols || outer * cols > lim / inner) return np::fail(NP_ERR_INVALID, "%s: outer.cols.inner does not fit a size_t", who);
    numel = outer * cols * inner;
    return NP_OK;
}

bool overlap(const void *p, size_t np_, const void *q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq * sizeof(float) && b < a + np_ * sizeof(float);
}

bool known_mode(int mode) { return mode == NP_SOFTMAX || mode == NP_LOG_SOFTMAX; }

}  // namespace

extern "C" {

// The order is the pointers, the extents, the mode, the aliasing, the form, ensure_init, then work: a refused call has touched no device.
int np_softmax_forward(const float *x, size_t outer, size_t cols, size_t inner, int mode, float *y) {
    if (!x || !y) return np::fail(NP_ERR_INVALID, "np_softmax_forward: null pointer");
    size_t numel = 0;
    if (int rc = check_extents("np_softmax_forward", outer, cols, inner, numel)) return rc;
    if (!known_mode(mode)) return np::fail(NP_ERR_INVALID, "np_softmax_forward: unknown mode %d", mode);
    if (overlap(x, numel, y, numel)) return np::fail(NP_ERR_INVALID, "np_softmax_forward: y overlaps x");
    int form = 0;
    if (int rc = pick_form("np_softmax_forward", (unsigned)cols, inner, false, form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    const SmxArgs g = {x, nullptr, y, nullptr, outer, (unsigned)cols, inner, mode, 1.0f};
    return launch<OP_FWD>(form, g);
}

int np_softmax_backward(const float *y, const float *dy, size_t outer, size_t cols, size_t inner, int mode, float *dx) {
    if (!y || !dy || !dx) return np::fail(NP_ERR_INVALID, "np_softmax_backward: null pointer");
    size_t numel = 0;
    if (int rc = check_extents("np_softmax_backward", outer, cols, inner, numel)) return rc;
    if (!known_mode(mode)) return np::fail(NP_ERR_INVALID, "np_softmax_backward: unknown mode %d", mode);
    if (overlap(y, numel, dx, numel) || (dx != dy && overlap(dy, numel, dx, numel)))
        return np::fail(NP_ERR_INVALID, "np_softmax_backward: dx overlaps y, or dy in part (dx == dy is allowed)");
    int form = 0;
    if (int rc = pick_form("np_softmax_backward", (unsigned)cols, inner, false, form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    const SmxArgs g = {y, dy, dx, nullptr, outer, (unsigned)cols, inner, mode, 1.0f};
    return launch<OP_BWD>(form, g);
}

int np_cross_entropy(const float *logits, const float *target, size_t rows, size_t cols, int target_kind, float scale, float *loss_rows,
                     float *dlogits) {
    if (!logits || !target || !loss_rows) return np::fail(NP_ERR_INVALID, "np_cross_entropy: null pointer");
    size_t numel = 0;
    if (int rc = check_extents("np_cross_entropy", rows, cols, 1, numel)) return rc;
    if (target_kind != NP_XENT_INDEX && target_kind != NP_XENT_PROB) return np::fail(NP_ERR_INVALID, "np_cross_entropy: unknown target kind %d", target_kind);
    const size_t nt = target_kind == NP_XENT_INDEX ? rows : numel;
    if (overlap(logits, numel, loss_rows, rows) || overlap(target, nt, loss_rows, rows) ||
        (dlogits && (overlap(logits, numel, dlogits, numel) || overlap(target, nt, dlogits, numel) || overlap(loss_rows, rows, dlogits, numel))))
        return np::fail(NP_ERR_INVALID, "np_cross_entropy: an output overlaps an input or the other output");
    int form = 0;
    if (int rc = pick_form("np_cross_entropy", (unsigned)cols, 1, true, form)) return rc;
    if (int rc = np::ensure_init()) return rc;
    const SmxArgs g = {logits, target, dlogits, loss_rows, rows, (unsigned)cols, 1, target_kind, scale};
    return launch<OP_XENT>(form, g);
}

int np_debug_softmax_last_path(int *form) {
    if (!form) return np::fail(NP_ERR_INVALID, "np_debug_softmax_last_path: null pointer");
    *form = g_smx_last_form;
    return NP_OK;
}

int np_debug_softmax_force_form(int form) {
    if (form != -1 && (form < FORM_SHORT || form > FORM_STRIDED))
        return np::fail(NP_ERR_INVALID, "np_debug_softmax_force_form: form must be -1 (by the extents) or 1 .. 5");
    g_smx_force_form = form;
    return NP_OK;
}

int np_debug_softmax_bounds(size_t bounds[], int n) {
    if (!bounds) return np::fail(NP_ERR_INVALID, "np_debug_softmax_bounds: null pointer");
    if (n < kNumBounds) return np::fail(NP_ERR_INVALID, "np_debug_softmax_bounds: room for %d values is needed", kNumBounds);
    bounds[0] = kShortMaxCols, bounds[1] = kWaveMaxCols, bounds[2] = kBlockMaxCols, bounds[3] = kSlabFloats, bounds[4] = kSlabRowsMax;
    return NP_OK;
}

}  // extern "C"
