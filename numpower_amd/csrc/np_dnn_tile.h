// What np_dnn.hip (convolution layers) and np_linear.hip (dense layers) compile from ONE text: the layer's activation and its
// derivative, and the MFMA tile step.  Device code only; every unit that includes it gets its own internal copy.
#ifndef NUMPOWER_AMD_NP_DNN_TILE_H
#define NUMPOWER_AMD_NP_DNN_TILE_H

#include "np_elementwise_ops.h"   // the bodies of NP_TANH and NP_EXP; fp contraction is off in a unit that includes it
#include "np_internal.h"

namespace {

// ---- tile constants (tests/test_gpu_dnn.py and tests/linear_family.py mirror them) ----
constexpr int kTN = 128;                  // columns of a tile
constexpr int kTK = 32;                   // reduction step staged through LDS
constexpr int kTMSmall = 32, kTMMid = 64, kTMLarge = 128;   // the TM instantiations
constexpr int kAStr = kTK + 1, kBStr = kTN + 1;             // LDS row strides (odd: a column walk touches every bank)

// the weight gradients (dW of a convolution, dw of a dense layer): a slice of the reduction is at least kWgradMinSteps steps long,
// slices stop once tiles x S reaches kWgradTargetGroups workgroups
constexpr int kWgradMinSteps = 8, kWgradTargetGroups = 512, kWgradMaxSlices = 256;

constexpr size_t kLim = (size_t)1 << 31;
// a * b, saturating at kLim (both factors at most kLim)
inline size_t mul_lim(size_t a, size_t b) { return (a >= kLim || b >= kLim || a * b >= kLim) ? kLim : a * b; }

typedef float dnn_v16f __attribute__((ext_vector_type(16)));

// y = act(v).  relu: a NaN stays NaN, -0.0 becomes +0.0; sigmoid: 0 and 1 at -+Inf, NaN at NaN
template <int ACT>
__device__ __forceinline__ float act_apply(float v) {
    if constexpr (ACT == NP_ACT_RELU) return (v <= 0.0f) ? 0.0f : v;
    if constexpr (ACT == NP_ACT_TANH) return unary_apply<NP_TANH>(v, 0.0f, 0.0f);
    if constexpr (ACT == NP_ACT_SIGMOID) return 1.0f / (1.0f + unary_apply<NP_EXP>(-v, 0.0f, 0.0f));
    return v;
}

// dz = dy . act'(y) through the output y.  relu is a select: a NaN y passes dy, a dy over y <= 0 reaches nothing
template <int ACT>
__device__ __forceinline__ float act_grad(float y, float dy) {
    if constexpr (ACT == NP_ACT_RELU) return (y <= 0.0f) ? 0.0f : dy;
    if constexpr (ACT == NP_ACT_TANH) return dy * (1.0f - y * y);
    if constexpr (ACT == NP_ACT_SIGMOID) return dy * ((1.0f - y) * y);
    return dy;
}

// how the 4 waves share a TM x kTN tile: 32 x 32 MFMA blocks, MI x NJ of them per wave
template <int TM>
struct Tile {
    static constexpr int WM = TM >= 128 ? 2 : 1, WN = 4 / WM, MI = TM / (WM * 32), NJ = kTN / (WN * 32);
};

// the accumulator's row inside a 32 x 32 block: register r of a lane in half kq
__device__ __forceinline__ int acc_row(int r, int kq) { return (r & 3) + 8 * (r >> 2) + 4 * kq; }

// one staged step: acc += As (TM x kTK) . Bs (kTK x kTN), k ascending
template <int TM>
__device__ __forceinline__ void mma_step(const float *As, const float *Bs, dnn_v16f (&acc)[Tile<TM>::MI][Tile<TM>::NJ], int wm, int wn,
                                         int lane) {
    using T = Tile<TM>;
    const int i = lane & 31, kq = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < kTK; kk += 2) {
        float a[T::MI], b[T::NJ];
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi) a[mi] = As[((wm * T::MI + mi) * 32 + i) * kAStr + kk + kq];
#pragma unroll
        for (int nj = 0; nj < T::NJ; ++nj) b[nj] = Bs[(kk + kq) * kBStr + (wn * T::NJ + nj) * 32 + i];
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
            for (int nj = 0; nj < T::NJ; ++nj) acc[mi][nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[nj], acc[mi][nj], 0, 0, 0);
    }
}

inline int pick_tm(size_t rows) { return rows <= (size_t)kTMSmall ? kTMSmall : rows <= (size_t)kTMMid ? kTMMid : kTMLarge; }

}  // namespace

#endif
