// Convolution layers for GPU arrays: np_conv2d_forward, np_conv2d_backward_data, np_conv2d_backward_filter.
//
// and their _ex forms with a window stride (sh, sw) and a tap dilation (dh, dw).
//
// x (N, C, H, W), w (F, C, kh, kw), y (N, F, oh, ow), row-major fp32; cross-correlation, zero padding (ph, pw).
// Everything is an implicit GEMM on v_mfma_f32_32x32x2_f32; no im2col matrix is ever written.
//
//   forward   Y (F x N.P) = Wm (F x K) . Col (K x N.P),  K = C.kh.kw with k = (c.kh + p).kw + q — the filters' own memory, so
//             Wm is a plain row-major matrix — and the pixel index flattened over the batch, jg = n.P + i.ow + j, P = oh.ow.
//             Col[k][jg] = x~[n, c, i + p - ph, j + q - pw] is gathered from x while a tile is staged; taps outside the image are
//             STORED zeros (an Inf tap over the padding gives NaN, as a materialised padded array would).
//   dX        the same kernel: dX = forward(dy as an input with F channels, w', pad (kh - 1 - ph, kw - 1 - pw)), where
//             w'[c, f, p, q] = w[f, c, kh - 1 - p, kw - 1 - q] is written to pool scratch by dnn_filter_flip_kernel.
//   dW        dW (F x K) = dYm (F x N.P) . Col^T, the same gather on the other operand.  The output is small and the reduction
//             long: it is cut into S slices of whole kTK-steps, each slice's tile goes to pool scratch and dnn_wgrad_fold_kernel
//             adds the slices in slice order (S == 1 writes dW directly).  No float atomics.
//
// The general gather.  A kernel is compiled in three FORMs of one gather: position t = i.s - pad + p.d on the grid of the
// gathered operand dilated by l reads in[t / l] when t >= 0, t mod l == 0 and t / l < extent, and a stored zero otherwise.
//   0  unit: s = d = l = 1, the text above and the code it always was
//   1  window stride s and tap dilation d, l = 1: the forward pass and dW of a strided / dilated layer, dX of a dilated one
//   2  input dilation l with s = 1: dX of a strided layer is the forward pass over dy dilated by (sh, sw), taps dilated by
//      (dh, dw), pad (keh - 1 - ph, kew - 1 - pw), out (H, W).  It spends sh.sw times the useful MACs on stored zeros.
// No form divides per gathered element: the pixel is decoded once (form 2: into quotient and residue mod l), the step's tap
// table holds p.d and q.d (form 2: their quotients and residues), and a residue sum is 0, l (carry one) or no multiple of l.
//
// Tiles: a workgroup of 4 waves computes TM x kTN outputs through LDS in reduction steps of kTK; TM is 32, 64 or 128 and is the
// smallest that covers F (beyond 128: 128), so a layer with few filters does not burn a 128-row tile.  Out-of-range taps, the
// reduction's tail and the tile edges are zero-filled on BOTH operands: nothing outside the receptive field reaches an output.
//
// Reduction order: every output is ONE fp32 fmaf chain from +0.0f over its reduction index in ascending order (the MFMA is
// bit for bit that chain), continued over the zero-filled tail of the last step.  For y and dX the order depends on (C, kh, kw)
// resp. (F, kh, kw) alone — not on N, the position of the pixel, TM or any device state — so the same image gives the same bits
// at any batch size and position.  For dW the chain runs over jg inside a slice and the slices are then added in order; S is a
// function of the extents alone.  Results are bit-identical from run to run.
//
// The layer (np_conv2d_forward_act, np_conv2d_backward_act).  The forward kernel has a second store loop, selected at compile
// time (EPI) for gather forms 0 and 1: v = acc + bias[f] — ONE fp32 add after the chain, not the chain's start value — and
// y = act(v), the activation a wave-uniform switch taken once, around one store loop each.  The plain instantiations, their
// kernel argument and their instruction stream are what they were: the epilogue's operands travel in EpiArgs, which only the EPI forms read.
// tanh and sigmoid evaluate the functions of np_elementwise_ops.h (tanhf; fast_exp), so a fused result is bit for bit the
// unfused one.  The backward pass of the activation is one streaming kernel over y and dy (N, F, P): dz = dy . act'(y), the
// derivative expressed through the OUTPUT, and db[f] = sum_{n,pixel} dz.  A workgroup owns one filter f and one slice of the
// flattened index m = n.P + pixel; a lane adds its elements m0 + lane, m0 + lane + 256, ... in ascending order, the workgroup
// folds its 256 lanes in a fixed tree, slices go to pool scratch and dnn_bias_fold_kernel adds them in slice order (S == 1
// writes db directly).  No float atomics; S is a function of (N, F, P) alone; bit-identical from run to run.  The walk decodes
// m into (n, pixel) ONCE per lane and then steps by 256 = q.P + r with one compare: no division per element, consecutive lanes
// read consecutive addresses inside an (n, f) plane, whatever P is.
#include <limits.h>

#include <type_traits>

#include "np_dnn_tile.h"   // act_apply / act_grad, the tile constants and mma_step: the text np_linear.hip compiles too

namespace {

// ---- tile constants: np_dnn_tile.h; a tile's columns are pixels jg (forward) or reduction columns k (dW) ----

// db (tests/test_gpu_dnn_act.py mirrors the rule): the M = N.P elements of a filter are cut into S slices,
//   want = min(M / kActMinSlice, ceil(kActTargetGroups / F), kActMaxSlices), at least 1
//   L = ceil(M / want) rounded up to a multiple of kActBlock,  S = ceil(M / L)
constexpr int kActBlock = 256, kActMinSlice = 4096, kActTargetGroups = 2048, kActMaxSlices = 256;

int g_dnn_last_tm = 0, g_dnn_last_slices = 0, g_dnn_last_form = 0;
int g_dnn_last_act = 0, g_dnn_last_has_bias = 0, g_dnn_last_bias_slices = 0;

// what the unit form reads: its kernel arguments, and with them its instruction stream, are what they were before the general gather
struct ConvCore {
    const float *x;   // the gathered operand (N, C, H, W)
    const float *w;   // forward: the filters (F, C, kh, kw) as Wm; dW: dy (N, F, oh, ow)
    float *out;
    int N, C, H, W, F, kh, kw, ph, pw, oh, ow;
    int K, P, NP;     // C.kh.kw, oh.ow, N.P
};

struct ConvArgs : ConvCore {
    int sh, sw, dh, dw, lh, lw;   // window stride, tap dilation, input dilation (H, W are the extents BEFORE that dilation)
};

// a kernel's argument: forms 1 and 2 read the whole of ConvArgs
template <int FORM>
using KernelArgs = std::conditional_t<FORM == 0, ConvCore, ConvArgs>;

// the same with the epilogue's operands behind it: the argument of the EPI instantiations alone
template <int FORM>
struct EpiArgs : KernelArgs<FORM> {
    const float *bias;   // F floats or nullptr
    int act;             // np_conv_act
};

template <int FORM, bool EPI>
using FpropArgs = std::conditional_t<EPI, EpiArgs<FORM>, KernelArgs<FORM>>;

int form_of(const ConvArgs &a) { return (a.lh != 1 || a.lw != 1) ? 2 : (a.sh != 1 || a.sw != 1 || a.dh != 1 || a.dw != 1) ? 1 : 0; }

// k = (c.kh + p).kw + q -> the tap's offset inside one image of x and its (p.dh, q.dw); koff = -1 marks the reduction's tail.
// Form 2: (kp, kq) are the quotients of p.dh, q.dw by the input dilation and (rp, rq) the residues, koff is built from the quotients.
template <int FORM>
__device__ __forceinline__ void decode_tap(const KernelArgs<FORM> &p, int k, int &koff, int &kp, int &kq, int &rp, int &rq) {
    koff = -1;
    kp = kq = rp = rq = 0;
    if (k < p.K) {
        const int khw = p.kh * p.kw, c = k / khw, r = k - c * khw;
        kp = r / p.kw;
        kq = r - kp * p.kw;
        if constexpr (FORM != 0) kp *= p.dh, kq *= p.dw;
        if constexpr (FORM == 2) {
            rp = kp % p.lh, kp /= p.lh;
            rq = kq % p.lw, kq /= p.lw;
        }
        koff = (c * p.H + kp) * p.W + kq;
    }
}

// where the window of output pixel (oi, oj) begins: (ih0, iw0) on the operand's grid; form 2: floor quotient and residue of that
// position on the dilated grid
struct Corner {
    int ih0, iw0, rh0, rw0;
};

template <int FORM>
__device__ __forceinline__ Corner corner_of(const KernelArgs<FORM> &p, int oi, int oj) {
    Corner c = {oi - p.ph, oj - p.pw, 0, 0};
    if constexpr (FORM == 1) c.ih0 = oi * p.sh - p.ph, c.iw0 = oj * p.sw - p.pw;
    if constexpr (FORM == 2) {
        const int th = c.ih0, tw = c.iw0;   // >= -(keh - 1), -(kew - 1)
        c.ih0 = th / p.lh, c.rh0 = th - c.ih0 * p.lh;
        if (c.rh0 < 0) c.rh0 += p.lh, --c.ih0;
        c.iw0 = tw / p.lw, c.rw0 = tw - c.iw0 * p.lw;
        if (c.rw0 < 0) c.rw0 += p.lw, --c.iw0;
    }
    return c;
}

// one element of Col: x at the corner xo (+ (ih0, iw0)) plus the tap, or a stored zero
template <int FORM>
__device__ __forceinline__ float gather(const KernelArgs<FORM> &p, bool pixel, long long xo, const Corner &c, int koff, int kp, int kq, int rp, int rq) {
    int ih = c.ih0 + kp, iw = c.iw0 + kq;
    if constexpr (FORM == 2) {
        // residue sums lie in [0, 2l - 2]: 0 and l are the multiples of l, l carries one into the quotient
        const int rh = c.rh0 + rp, rw = c.rw0 + rq;
        const bool ch = rh == p.lh, cw = rw == p.lw;
        if ((rh != 0 && !ch) || (rw != 0 && !cw)) return 0.0f;
        if (ch) ++ih, xo += p.W;
        if (cw) ++iw, ++xo;
    }
    if (pixel && koff >= 0 && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) return p.x[xo + koff];
    return 0.0f;
}

// the layer's store loop for one activation: v = acc + bias[f] (one add after the chain), y = act(v).  fw is the first row of
// the wave's blocks; a row's bias is read once, and only for rows below F; yb[nj] == nullptr: the column lies beyond N.P
template <int TM, int ACT>
__device__ __forceinline__ void epi_store(const dnn_v16f (&acc)[Tile<TM>::MI][Tile<TM>::NJ], float *const (&yb)[Tile<TM>::NJ], const float *bias, int fw,
                                          int kq, int F, int P) {
    using T = Tile<TM>;
    const bool has_bias = bias != nullptr;
#pragma unroll
    for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = fw + mi * 32 + acc_row(r, kq);
            if (f >= F) continue;
            const float b = has_bias ? bias[f] : 0.0f;
#pragma unroll
            for (int nj = 0; nj < T::NJ; ++nj) {
                const float v = has_bias ? acc[mi][nj][r] + b : acc[mi][nj][r];
                if (yb[nj]) yb[nj][(size_t)f * P] = act_apply<ACT>(v);
            }
        }
}

// grid.x = F-tiles x pixel-tiles, F-tiles fastest: neighbouring workgroups gather the same pixels
template <int TM, int FORM, bool EPI = false>
__global__ __launch_bounds__(256, 2) void dnn_fprop_kernel(const FpropArgs<FORM, EPI> p) {
    static_assert(!EPI || FORM != 2, "the data gradient has no bias and no activation");
    using T = Tile<TM>;
    __shared__ float As[TM * kAStr];
    __shared__ float Bs[kTK * kBStr];
    __shared__ int s_koff[kTK], s_kp[kTK], s_kq[kTK];   // the step's offset table: one decode per k, none per element
    __shared__ int s_rp[FORM == 2 ? kTK : 1], s_rq[FORM == 2 ? kTK : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / T::WN, wn = wave % T::WN;
    const int tiles_f = (p.F + TM - 1) / TM;
    const int f0 = (int)(blockIdx.x % tiles_f) * TM, j0 = (int)(blockIdx.x / tiles_f) * kTN;

    dnn_v16f acc[T::MI][T::NJ];
#pragma unroll
    for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
        for (int nj = 0; nj < T::NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nj][r] = 0.0f;

    // a thread gathers ONE pixel for the whole reduction: for a fixed k consecutive pixels of an output row are consecutive addresses
    const int jl = tid & (kTN - 1), krow0 = tid >> 7;
    const int jg = j0 + jl;
    const bool pixel = jg < p.NP;
    Corner cr = {0, 0, 0, 0};
    long long xo = 0;   // the window's corner in x: outside the array where the padding begins, only ever added to a valid tap
    if (pixel) {
        const int n = jg / p.P, pix = jg - n * p.P, oi = pix / p.ow, oj = pix - oi * p.ow;
        cr = corner_of<FORM>(p, oi, oj);
        xo = (long long)n * p.C * p.H * p.W + (long long)cr.ih0 * p.W + cr.iw0;
    }
    const int kc = tid & 31, fr = tid >> 5;

    for (int k0 = 0; k0 < p.K; k0 += kTK) {
        if (tid < kTK) {
            int rp, rq;
            decode_tap<FORM>(p, k0 + tid, s_koff[tid], s_kp[tid], s_kq[tid], rp, rq);
            if constexpr (FORM == 2) s_rp[tid] = rp, s_rq[tid] = rq;
        }
        __syncthreads();   // also: every wave is done with the previous step's tiles
#pragma unroll
        for (int u = 0; u < TM / 8; ++u) {
            const int f = f0 + fr + 8 * u, k = k0 + kc;
            As[(fr + 8 * u) * kAStr + kc] = (f < p.F && k < p.K) ? p.w[(size_t)f * p.K + k] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kTK / 2; ++u) {
            const int kr = krow0 + 2 * u;
            Bs[kr * kBStr + jl] = gather<FORM>(p, pixel, xo, cr, s_koff[kr], s_kp[kr], s_kq[kr], FORM == 2 ? s_rp[kr] : 0, FORM == 2 ? s_rq[kr] : 0);
        }
        __syncthreads();
        mma_step<TM>(As, Bs, acc, wm, wn, lane);
    }

    const int i = lane & 31, kq = lane >> 5;
    if constexpr (EPI) {
        // the layer's store loop: one add after the chain, then the activation.  A lane's rows are the same for every nj: their
        // bias is read once, and only for rows below F (the tile rows the K loop zero-filled never touch the array)
        float *yb[T::NJ];   // nullptr: the column lies beyond N.P
#pragma unroll
        for (int nj = 0; nj < T::NJ; ++nj) {
            const int col = j0 + (wn * T::NJ + nj) * 32 + i;
            const int n = col / p.P, pix = col - n * p.P;
            yb[nj] = col < p.NP ? p.out + ((size_t)n * p.F * p.P + pix) : nullptr;
        }
        // one compact loop per activation: the switch is taken once, not once per output
        const int fw = f0 + wm * T::MI * 32;
        switch (p.act) {
        case NP_ACT_RELU: epi_store<TM, NP_ACT_RELU>(acc, yb, p.bias, fw, kq, p.F, p.P); break;
        case NP_ACT_TANH: epi_store<TM, NP_ACT_TANH>(acc, yb, p.bias, fw, kq, p.F, p.P); break;
        case NP_ACT_SIGMOID: epi_store<TM, NP_ACT_SIGMOID>(acc, yb, p.bias, fw, kq, p.F, p.P); break;
        default: epi_store<TM, NP_ACT_NONE>(acc, yb, p.bias, fw, kq, p.F, p.P); break;
        }
        return;
    }
#pragma unroll
    for (int nj = 0; nj < T::NJ; ++nj) {
        const int col = j0 + (wn * T::NJ + nj) * 32 + i;
        if (col >= p.NP) continue;
        const int n = col / p.P, pix = col - n * p.P;
        float *yb = p.out + ((size_t)n * p.F * p.P + pix);
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = f0 + (wm * T::MI + mi) * 32 + acc_row(r, kq);
                if (f < p.F) yb[(size_t)f * p.P] = acc[mi][nj][r];
            }
    }
}

// w'[c, f, p, q] = w[f, c, kh - 1 - p, kw - 1 - q]
__global__ __launch_bounds__(256) void dnn_filter_flip_kernel(const float *__restrict__ w, float *__restrict__ wf, int F, int C, int kh, int kw,
                                                              unsigned n) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    const int khw = kh * kw;
    const int cf = (int)(idx / (unsigned)khw), r = (int)(idx - (unsigned)cf * (unsigned)khw);
    const int c = cf / F, f = cf - c * F, pp = r / kw, q = r - pp * kw;
    wf[idx] = w[((size_t)f * C + c) * khw + (size_t)(kh - 1 - pp) * kw + (kw - 1 - q)];
}

// grid.x = F-tiles x k-tiles, grid.y = slices; a slice reduces steps [slice * steps_per_slice, ...) of kTK pixels jg each and
// stores its F x K tile at out + slice * F * K
template <int TM, int FORM>
__global__ __launch_bounds__(256, 2) void dnn_wgrad_kernel(const KernelArgs<FORM> p, int steps_per_slice) {
    static_assert(FORM != 2, "the filter gradient gathers x itself: no input dilation");
    using T = Tile<TM>;
    __shared__ float As[TM * kAStr];
    __shared__ float Bs[kTK * kBStr];
    __shared__ int s_koff[kTN], s_kp[kTN], s_kq[kTN];   // the tile's columns, decoded once
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / T::WN, wn = wave % T::WN;
    const int tiles_f = (p.F + TM - 1) / TM;
    const int f0 = (int)(blockIdx.x % tiles_f) * TM, kc0 = (int)(blockIdx.x / tiles_f) * kTN;

    dnn_v16f acc[T::MI][T::NJ];
#pragma unroll
    for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
        for (int nj = 0; nj < T::NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nj][r] = 0.0f;

    if (tid < kTN) {
        int rp, rq;
        decode_tap<FORM>(p, kc0 + tid, s_koff[tid], s_kp[tid], s_kq[tid], rp, rq);
    }
    const int steps = (p.NP + kTK - 1) / kTK;
    const int s0 = (int)blockIdx.y * steps_per_slice, s1 = s0 + steps_per_slice < steps ? s0 + steps_per_slice : steps;
    const int kr = tid & 31, g = tid >> 5;   // a thread stages one pixel of the step: consecutive lanes, consecutive addresses

    for (int s = s0; s < s1; ++s) {
        const int jg = s * kTK + kr;
        const bool pixel = jg < p.NP;
        int n = 0, pix = 0;
        Corner cr = {0, 0, 0, 0};
        if (pixel) {
            n = jg / p.P;
            pix = jg - n * p.P;
            const int oi = pix / p.ow, oj = pix - oi * p.ow;
            cr = corner_of<FORM>(p, oi, oj);
        }
        const long long xo = (long long)n * p.C * p.H * p.W + (long long)cr.ih0 * p.W + cr.iw0;
        const float *db = p.w + ((size_t)n * p.F * p.P + pix);
        __syncthreads();   // the table (first step); every wave is done with the previous step's tiles
#pragma unroll
        for (int u = 0; u < TM / 8; ++u) {
            const int f = f0 + g + 8 * u;
            As[(g + 8 * u) * kAStr + kr] = (pixel && f < p.F) ? db[(size_t)f * p.P] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kTN / 8; ++u) {
            const int col = g + 8 * u;
            Bs[kr * kBStr + col] = gather<FORM>(p, pixel, xo, cr, s_koff[col], s_kp[col], s_kq[col], 0, 0);
        }
        __syncthreads();
        mma_step<TM>(As, Bs, acc, wm, wn, lane);
    }

    float *out = p.out + (size_t)blockIdx.y * p.F * p.K;
    const int i = lane & 31, kq = lane >> 5;
#pragma unroll
    for (int nj = 0; nj < T::NJ; ++nj) {
        const int k = kc0 + (wn * T::NJ + nj) * 32 + i;
        if (k >= p.K) continue;
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = f0 + (wm * T::MI + mi) * 32 + acc_row(r, kq);
                if (f < p.F) out[(size_t)f * p.K + k] = acc[mi][nj][r];
            }
    }
}

// dw[e] = part[0][e] + part[1][e] + ... in slice order
__global__ __launch_bounds__(256) void dnn_wgrad_fold_kernel(const float *__restrict__ part, float *__restrict__ dw, unsigned n, int slices) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    float acc = part[idx];
    for (int s = 1; s < slices; ++s) acc += part[(size_t)s * n + idx];
    dw[idx] = acc;
}

// grid.x = F, grid.y = slices.  Workgroup (f, s) walks m = n.P + pixel over [s.slice_len, (s + 1).slice_len) of filter f's M = N.P
// elements: lane t takes m0 + t, m0 + t + 256, ... and adds them in that order.  (n, pixel) is decoded once; a step of
// 256 = q.P + r moves the address by q planes of the batch and r pixels, and by one more plane when the pixel wraps.
// dz == nullptr: no dz is written; out == nullptr: no sum is formed.  out[s.F + f] is the workgroup's sum (out is db when S == 1).
template <int ACT>
__global__ __launch_bounds__(kActBlock) void dnn_act_grad_kernel(const float *__restrict__ y, const float *__restrict__ dy, float *__restrict__ dz,
                                                                  float *__restrict__ out, int F, int P, unsigned M, unsigned slice_len) {
    __shared__ float lds4[4];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    // M < 2^31 and slice_len <= M + 255: every sum below fits 32 unsigned bits
    const unsigned m0 = blockIdx.y * slice_len, m1 = (M - m0 < slice_len) ? M : m0 + slice_len, mt = m0 + (unsigned)tid;
    const unsigned n0 = mt / (unsigned)P;
    int pix = (int)(mt - n0 * (unsigned)P);
    const int q = kActBlock / P, r = kActBlock - q * P;   // uniform
    const size_t plane = (size_t)F * P, step = (size_t)q * plane + r, wrap = plane - P;
    size_t idx = (size_t)n0 * plane + (size_t)f * P + pix;
    float sum = 0.0f;
    // four elements in flight per lane; an element is loaded, and its address used, only where its index is below m1 <= M.
    // m is the element's index minus m1: negative inside the slice
    for (long long m = (long long)mt - (long long)m1; m < 0; m += 4 * kActBlock) {
        size_t at[4];
        float g[4], yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            at[u] = idx;
            idx += step, pix += r;
            if (pix >= P) pix -= P, idx += wrap;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = m + u * kActBlock < 0;
            g[u] = in ? dy[at[u]] : 0.0f;
            yv[u] = 1.0f;
            if constexpr (ACT != NP_ACT_NONE) yv[u] = in ? y[at[u]] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (m + u * kActBlock < 0) {
                const float d = act_grad<ACT>(yv[u], g[u]);
                if constexpr (ACT != NP_ACT_NONE)
                    if (dz) dz[at[u]] = d;
                sum += d;
            }
        }
    }
    if (!out) return;
    sum = np::dev::block_reduce<NP_SUM>(sum, lds4);   // lanes 32 apart, 16, ..., 1, then the four waves in order
    if (tid == 0) out[(size_t)blockIdx.y * F + f] = sum;
}

// db[f] = part[0][f] + part[1][f] + ... in slice order
__global__ __launch_bounds__(256) void dnn_bias_fold_kernel(const float *__restrict__ part, float *__restrict__ db, unsigned F, int slices) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= F) return;
    float acc = part[f];
    for (int s = 1; s < slices; ++s) acc += part[(size_t)s * F + f];
    db[f] = acc;
}

// a layer as the C ABI names it; the plain entry points have stride and dilation 1, np_conv2d_shape* N = C = F = 1
struct LayerShape {
    size_t N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw;
};

// the spatial half of the shape -> the output extents, written only when the shape is accepted
int check_spatial(const char *who, const LayerShape &s, size_t &oh, size_t &ow) {
    if (s.H < 1 || s.W < 1 || s.kh < 1 || s.kw < 1 || s.sh < 1 || s.sw < 1 || s.dh < 1 || s.dw < 1)
        return np::fail(NP_ERR_INVALID, "%s: every extent, stride and dilation must be at least 1", who);
    const size_t keh = mul_lim(s.dh, s.kh - 1) + 1, kew = mul_lim(s.dw, s.kw - 1) + 1;   // the effective window
    if (s.H >= kLim || s.W >= kLim || s.kh >= kLim || s.kw >= kLim || s.sh >= kLim || s.sw >= kLim || keh >= kLim || kew >= kLim)
        return np::fail(NP_ERR_INVALID, "%s: an extent, a stride or an effective window is 2^31 or more", who);
    if (s.ph >= keh || s.pw >= kew)
        return np::fail(NP_ERR_INVALID, "%s: the padding (%zu, %zu) must be smaller than the effective window (%zu, %zu)", who, s.ph, s.pw, keh, kew);
    if (keh > s.H + 2 * s.ph || kew > s.W + 2 * s.pw)
        return np::fail(NP_ERR_INVALID, "%s: the effective window (%zu, %zu) is larger than the padded image (%zu, %zu)", who, keh, kew,
                        s.H + 2 * s.ph, s.W + 2 * s.pw);
    // the kernels form the row index oi.sh - ph + p.dh as an int: it must not reach 2^31
    if (s.H + 2 * s.ph >= kLim || s.W + 2 * s.pw >= kLim) return np::fail(NP_ERR_INVALID, "%s: a padded extent is 2^31 or more", who);
    oh = (s.H + 2 * s.ph - keh) / s.sh + 1;
    ow = (s.W + 2 * s.pw - kew) / s.sw + 1;
    return NP_OK;
}

// the whole shape of a layer; fills the kernel's extents (out and the operand pointers are the caller's)
int check_layer(const char *who, const LayerShape &s, ConvArgs &a) {
    if (s.N < 1 || s.C < 1 || s.F < 1) return np::fail(NP_ERR_INVALID, "%s: every extent, stride and dilation must be at least 1", who);
    size_t oh, ow;
    if (int rc = check_spatial(who, s, oh, ow)) return rc;
    const size_t khw = mul_lim(s.kh, s.kw), P = mul_lim(oh, ow), numel_x = mul_lim(mul_lim(s.N, s.C), mul_lim(s.H, s.W));
    const size_t numel_w = mul_lim(mul_lim(s.F, s.C), khw), numel_y = mul_lim(mul_lim(s.N, s.F), P);
    const size_t NP = mul_lim(s.N, P), K = mul_lim(s.C, khw), Kt = mul_lim(s.F, khw);
    if (numel_x >= kLim || numel_w >= kLim || numel_y >= kLim || NP >= kLim || K >= kLim || Kt >= kLim)
        return np::fail(NP_ERR_INVALID, "%s: an operand, the result, N.P or the reduction length has 2^31 elements or more", who);
    a.N = (int)s.N, a.C = (int)s.C, a.H = (int)s.H, a.W = (int)s.W, a.F = (int)s.F, a.kh = (int)s.kh, a.kw = (int)s.kw;
    a.ph = (int)s.ph, a.pw = (int)s.pw, a.oh = (int)oh, a.ow = (int)ow, a.K = (int)K, a.P = (int)P, a.NP = (int)NP;
    a.sh = (int)s.sh, a.sw = (int)s.sw, a.dh = (int)s.dh, a.dw = (int)s.dw, a.lh = a.lw = 1;
    return NP_OK;
}

// the data gradient of layer l as a forward layer over dy: F channels of oh x ow in, dilated by the stride; C channels of H x W
// out; taps dilated as the layer's, pad (keh - 1 - ph, kew - 1 - pw), stride 1
ConvArgs dgrad_layer(const ConvArgs &l, const float *dy, const float *flipped, float *dx) {
    ConvArgs a = {};
    a.x = dy;
    a.w = flipped;
    a.out = dx;
    a.N = l.N, a.C = l.F, a.H = l.oh, a.W = l.ow, a.F = l.C, a.kh = l.kh, a.kw = l.kw;
    a.ph = l.dh * (l.kh - 1) - l.ph, a.pw = l.dw * (l.kw - 1) - l.pw;
    a.oh = l.H, a.ow = l.W, a.K = l.F * l.kh * l.kw, a.P = l.H * l.W, a.NP = l.N * a.P;
    a.sh = a.sw = 1, a.dh = l.dh, a.dw = l.dw, a.lh = l.sh, a.lw = l.sw;
    return a;
}

// dW's launch shape, from the extents alone: slices of at least kWgradMinSteps steps until tiles x S fills the device
struct WgradPlan {
    int tm;
    size_t tiles, steps_per_slice, slices;
};

int plan_wgrad(const char *who, const ConvArgs &a, WgradPlan &pl) {
    pl.tm = pick_tm((size_t)a.F);
    pl.tiles = (((size_t)a.F + pl.tm - 1) / pl.tm) * (((size_t)a.K + kTN - 1) / kTN);
    if (pl.tiles >= kLim) return np::fail(NP_ERR_INVALID, "%s: %zu tiles are more than one launch holds", who, pl.tiles);
    const size_t steps = ((size_t)a.NP + kTK - 1) / kTK;
    size_t want = steps / kWgradMinSteps, fill = (kWgradTargetGroups + pl.tiles - 1) / pl.tiles;
    if (want > fill) want = fill;
    if (want > (size_t)kWgradMaxSlices) want = kWgradMaxSlices;
    if (want < 1) want = 1;
    pl.steps_per_slice = (steps + want - 1) / want;
    pl.slices = (steps + pl.steps_per_slice - 1) / pl.steps_per_slice;
    return NP_OK;
}

// the kernel's argument is KernelArgs<FORM>, what the plain instantiations always took; only an EPI one gets the epilogue's operands behind it
template <int FORM, bool EPI>
void launch_fprop_form(int tm, dim3 grid, dim3 block, const ConvArgs &a, const float *bias, int act) {
    FpropArgs<FORM, EPI> p;
    static_cast<KernelArgs<FORM> &>(p) = a;
    if constexpr (EPI) p.bias = bias, p.act = act;
    if (tm == kTMSmall) dnn_fprop_kernel<kTMSmall, FORM, EPI><<<grid, block, 0, np::stream()>>>(p);
    else if (tm == kTMMid) dnn_fprop_kernel<kTMMid, FORM, EPI><<<grid, block, 0, np::stream()>>>(p);
    else dnn_fprop_kernel<kTMLarge, FORM, EPI><<<grid, block, 0, np::stream()>>>(p);
}

// the forward kernel for y and for dX (bias == nullptr, NP_ACT_NONE).  Without a bias and an activation: the plain kernels, the
// plain bits.  Form 2 is dX of a strided layer and has no epilogue
int launch_fprop(const ConvArgs &a, const float *bias, int act) {
    const int tm = pick_tm((size_t)a.F);
    const size_t tiles = (((size_t)a.F + tm - 1) / tm) * (((size_t)a.NP + kTN - 1) / kTN);
    if (tiles >= kLim) return np::fail(NP_ERR_INVALID, "np_conv2d: %zu tiles are more than one launch holds", tiles);
    const dim3 grid((unsigned)tiles), block(256);
    const int form = form_of(a);
    const bool epi = bias || act != NP_ACT_NONE;
    if (form == 2) launch_fprop_form<2, false>(tm, grid, block, a, nullptr, NP_ACT_NONE);
    else if (form == 1 && epi) launch_fprop_form<1, true>(tm, grid, block, a, bias, act);
    else if (form == 1) launch_fprop_form<1, false>(tm, grid, block, a, nullptr, NP_ACT_NONE);
    else if (epi) launch_fprop_form<0, true>(tm, grid, block, a, bias, act);
    else launch_fprop_form<0, false>(tm, grid, block, a, nullptr, NP_ACT_NONE);
    NP_LAUNCH_CHECK("dnn_fprop_kernel");
    g_dnn_last_tm = tm;
    g_dnn_last_slices = 0;
    g_dnn_last_form = form;
    g_dnn_last_act = act;
    g_dnn_last_has_bias = bias != nullptr;
    return NP_OK;
}

// db's launch shape, from the extents alone (the rule next to kAct*)
struct ActGradPlan {
    size_t slice_len, slices;
};

ActGradPlan plan_act_grad(size_t F, size_t M) {
    size_t want = M / kActMinSlice, fill = (kActTargetGroups + F - 1) / F;
    if (want > fill) want = fill;
    if (want > (size_t)kActMaxSlices) want = kActMaxSlices;
    if (want < 1) want = 1;
    ActGradPlan pl;
    pl.slice_len = ((M + want - 1) / want + kActBlock - 1) / kActBlock * kActBlock;
    pl.slices = (M + pl.slice_len - 1) / pl.slice_len;
    return pl;
}

template <int ACT>
void launch_act_grad_as(dim3 grid, const float *y, const float *dy, float *dz, float *out, int F, int P, unsigned M, unsigned slice_len) {
    dnn_act_grad_kernel<ACT><<<grid, dim3(kActBlock), 0, np::stream()>>>(y, dy, dz, out, F, P, M, slice_len);
}

// out is db (one slice), the slices' scratch, which is then folded into db, or nullptr (no db wanted)
int launch_act_grad(const ActGradPlan &pl, const float *y, const float *dy, float *dz, float *out, float *db, size_t F, size_t P, size_t M, int act) {
    const dim3 grid((unsigned)F, (unsigned)pl.slices);
    const unsigned len = (unsigned)pl.slice_len;
    if (act == NP_ACT_RELU) launch_act_grad_as<NP_ACT_RELU>(grid, y, dy, dz, out, (int)F, (int)P, (unsigned)M, len);
    else if (act == NP_ACT_TANH) launch_act_grad_as<NP_ACT_TANH>(grid, y, dy, dz, out, (int)F, (int)P, (unsigned)M, len);
    else if (act == NP_ACT_SIGMOID) launch_act_grad_as<NP_ACT_SIGMOID>(grid, y, dy, dz, out, (int)F, (int)P, (unsigned)M, len);
    else launch_act_grad_as<NP_ACT_NONE>(grid, y, dy, nullptr, out, (int)F, (int)P, (unsigned)M, len);
    NP_LAUNCH_CHECK("dnn_act_grad_kernel");
    if (db) {
        if (pl.slices > 1) {
            dnn_bias_fold_kernel<<<dim3((unsigned)((F + 255) / 256)), dim3(256), 0, np::stream()>>>(out, db, (unsigned)F, (int)pl.slices);
            NP_LAUNCH_CHECK("dnn_bias_fold_kernel");
        }
        g_dnn_last_bias_slices = (int)pl.slices;
    }
    return NP_OK;
}

template <int FORM>
void launch_wgrad_form(int tm, dim3 grid, dim3 block, const ConvArgs &a, int steps_per_slice) {
    if (tm == kTMSmall) dnn_wgrad_kernel<kTMSmall, FORM><<<grid, block, 0, np::stream()>>>(a, steps_per_slice);
    else if (tm == kTMMid) dnn_wgrad_kernel<kTMMid, FORM><<<grid, block, 0, np::stream()>>>(a, steps_per_slice);
    else dnn_wgrad_kernel<kTMLarge, FORM><<<grid, block, 0, np::stream()>>>(a, steps_per_slice);
}

// a.out is dw (one slice) or the slices' scratch `part`, which is then folded into dw
int launch_wgrad(const ConvArgs &a, const WgradPlan &pl, const float *part, float *dw) {
    const dim3 grid((unsigned)pl.tiles, (unsigned)pl.slices), block(256);
    const int form = form_of(a);
    if (form == 0) launch_wgrad_form<0>(pl.tm, grid, block, a, (int)pl.steps_per_slice);
    else launch_wgrad_form<1>(pl.tm, grid, block, a, (int)pl.steps_per_slice);
    NP_LAUNCH_CHECK("dnn_wgrad_kernel");
    if (pl.slices > 1) {
        const size_t numel_w = (size_t)a.F * a.K;
        dnn_wgrad_fold_kernel<<<dim3((unsigned)((numel_w + 255) / 256)), dim3(256), 0, np::stream()>>>(part, dw, (unsigned)numel_w, (int)pl.slices);
        NP_LAUNCH_CHECK("dnn_wgrad_fold_kernel");
    }
    g_dnn_last_tm = pl.tm;
    g_dnn_last_slices = (int)pl.slices;
    g_dnn_last_form = form;
    return NP_OK;
}

// w' of layer l into pool scratch
int flip_filters(const ConvArgs &l, const float *w, np::Scratch &flipped) {
    const size_t numel_w = (size_t)l.F * l.K;
    if (int rc = flipped.alloc(numel_w * sizeof(float))) return rc;
    dnn_filter_flip_kernel<<<dim3((unsigned)((numel_w + 255) / 256)), dim3(256), 0, np::stream()>>>(w, (float *)flipped.ptr, l.F, l.C, l.kh, l.kw,
                                                                                                   (unsigned)numel_w);
    NP_LAUNCH_CHECK("dnn_filter_flip_kernel");
    return NP_OK;
}

// The three passes.  Every entry point below is a pointer check under its own name and one call of these: the plain calls
// with stride and dilation 1, the plain and _ex forward with no bias and NP_ACT_NONE.  The order is the shape, the activation,
// ensure_init, then work: a refused call has touched no device.
int conv_forward(const char *who, const float *x, const float *w, const float *bias, const LayerShape &s, int act, float *y) {
    ConvArgs a = {};
    if (int rc = check_layer(who, s, a)) return rc;
    if (act < NP_ACT_NONE || act > NP_ACT_SIGMOID) return np::fail(NP_ERR_INVALID, "%s: unknown activation %d", who, act);
    if (int rc = np::ensure_init()) return rc;
    a.x = x;
    a.w = w;
    a.out = y;
    return launch_fprop(a, bias, act);
}

int conv_backward_data(const char *who, const float *dy, const float *w, const LayerShape &s, float *dx) {
    ConvArgs l = {};
    if (int rc = check_layer(who, s, l)) return rc;
    if (int rc = np::ensure_init()) return rc;
    np::Scratch flipped;   // released on every path below
    if (int rc = flip_filters(l, w, flipped)) return rc;
    return launch_fprop(dgrad_layer(l, dy, (const float *)flipped.ptr, dx), nullptr, NP_ACT_NONE);
}

int conv_backward_filter(const char *who, const float *x, const float *dy, const LayerShape &s, float *dw) {
    ConvArgs a = {};
    if (int rc = check_layer(who, s, a)) return rc;
    if (int rc = np::ensure_init()) return rc;
    WgradPlan pl;
    if (int rc = plan_wgrad(who, a, pl)) return rc;
    np::Scratch part;   // released on every path below
    if (pl.slices > 1)
        if (int rc = part.alloc(pl.slices * (size_t)a.F * a.K * sizeof(float))) return rc;
    a.x = x;
    a.w = dy;
    a.out = pl.slices > 1 ? (float *)part.ptr : dw;
    return launch_wgrad(a, pl, (const float *)part.ptr, dw);
}

}  // namespace

extern "C" {

// ---- the plain calls: stride 1, dilation 1 ----

int np_conv2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t *oh, size_t *ow) {
    if (!oh || !ow) return np::fail(NP_ERR_INVALID, "np_conv2d_shape: null pointer");
    return check_spatial("np_conv2d_shape", {1, 1, H, W, 1, kh, kw, ph, pw, 1, 1, 1, 1}, *oh, *ow);
}

int np_conv2d_forward(const float *x, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw, size_t ph,
                      size_t pw, float *y) {
    if (!x || !w || !y) return np::fail(NP_ERR_INVALID, "np_conv2d_forward: null pointer");
    return conv_forward("np_conv2d_forward", x, w, nullptr, {N, C, H, W, F, kh, kw, ph, pw, 1, 1, 1, 1}, NP_ACT_NONE, y);
}

int np_conv2d_backward_data(const float *dy, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                            size_t ph, size_t pw, float *dx) {
    if (!dy || !w || !dx) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_data: null pointer");
    return conv_backward_data("np_conv2d_backward_data", dy, w, {N, C, H, W, F, kh, kw, ph, pw, 1, 1, 1, 1}, dx);
}

int np_conv2d_backward_filter(const float *x, const float *dy, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                              size_t ph, size_t pw, float *dw) {
    if (!x || !dy || !dw) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_filter: null pointer");
    return conv_backward_filter("np_conv2d_backward_filter", x, dy, {N, C, H, W, F, kh, kw, ph, pw, 1, 1, 1, 1}, dw);
}

// ---- _ex: a window stride and a tap dilation ----

int np_conv2d_shape_ex(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, size_t *oh,
                       size_t *ow) {
    if (!oh || !ow) return np::fail(NP_ERR_INVALID, "np_conv2d_shape_ex: null pointer");
    return check_spatial("np_conv2d_shape_ex", {1, 1, H, W, 1, kh, kw, ph, pw, sh, sw, dh, dw}, *oh, *ow);
}

int np_conv2d_forward_ex(const float *x, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw, size_t ph,
                         size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *y) {
    if (!x || !w || !y) return np::fail(NP_ERR_INVALID, "np_conv2d_forward_ex: null pointer");
    return conv_forward("np_conv2d_forward_ex", x, w, nullptr, {N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw}, NP_ACT_NONE, y);
}

int np_conv2d_backward_data_ex(const float *dy, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                               size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *dx) {
    if (!dy || !w || !dx) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_data_ex: null pointer");
    return conv_backward_data("np_conv2d_backward_data_ex", dy, w, {N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw}, dx);
}

int np_conv2d_backward_filter_ex(const float *x, const float *dy, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                                 size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *dw_out) {
    if (!x || !dy || !dw_out) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_filter_ex: null pointer");
    return conv_backward_filter("np_conv2d_backward_filter_ex", x, dy, {N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw}, dw_out);
}

// ---- _act: the layer's bias and activation ----

int np_conv2d_forward_act(const float *x, const float *w, const float *bias, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh,
                          size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, int act, float *y) {
    if (!x || !w || !y) return np::fail(NP_ERR_INVALID, "np_conv2d_forward_act: null pointer");
    return conv_forward("np_conv2d_forward_act", x, w, bias, {N, C, H, W, F, kh, kw, ph, pw, sh, sw, dh, dw}, act, y);
}

int np_conv2d_backward_act(const float *y, const float *dy, size_t N, size_t F, size_t P, int act, float *dz, float *db) {
    if (!dy) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: null pointer");
    if (!dz && !db) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: null pointer: dz and db are both null, nothing is asked for");
    if (N < 1 || F < 1 || P < 1) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: every extent must be at least 1");
    if (mul_lim(mul_lim(N, F), P) >= kLim) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: the arrays have 2^31 elements or more");
    if (act < NP_ACT_NONE || act > NP_ACT_SIGMOID) return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: unknown activation %d", act);
    if (act != NP_ACT_NONE && (!y || !dz))
        return np::fail(NP_ERR_INVALID, "np_conv2d_backward_act: null pointer: an activation needs y and dz");
    if (act == NP_ACT_NONE && !db) return NP_OK;   // dz = dy is not written and no sum is wanted: nothing to do
    if (int rc = np::ensure_init()) return rc;
    const ActGradPlan pl = plan_act_grad(F, N * P);
    np::Scratch part;   // released on every path below
    if (db && pl.slices > 1)
        if (int rc = part.alloc(pl.slices * F * sizeof(float))) return rc;
    float *out = !db ? nullptr : pl.slices > 1 ? (float *)part.ptr : db;
    return launch_act_grad(pl, y, dy, dz, out, db, F, P, N * P, act);
}

// ---- the probes: what the last launch chose ----

int np_debug_dnn_last_path(int *host_tm, int *host_slices) {
    if (!host_tm || !host_slices) return np::fail(NP_ERR_INVALID, "np_debug_dnn_last_path: null pointer");
    *host_tm = g_dnn_last_tm;
    *host_slices = g_dnn_last_slices;
    return NP_OK;
}

int np_debug_dnn_last_form(int *host_form) {
    if (!host_form) return np::fail(NP_ERR_INVALID, "np_debug_dnn_last_form: null pointer");
    *host_form = g_dnn_last_form;
    return NP_OK;
}

int np_debug_dnn_last_epilogue(int *act, int *has_bias, int *bias_slices) {
    if (!act || !has_bias || !bias_slices) return np::fail(NP_ERR_INVALID, "np_debug_dnn_last_epilogue: null pointer");
    *act = g_dnn_last_act;
    *has_bias = g_dnn_last_has_bias;
    *bias_slices = g_dnn_last_bias_slices;
    return NP_OK;
}

}  // extern "C"
