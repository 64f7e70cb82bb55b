// Dense layers for GPU arrays: np_linear_forward and np_linear_backward.
//
// x (M, K), w (N, K) = (out_features, in_features), bias (N), y (M, N), row-major fp32.
//
//   y  (M x N) = x . w^T       reduction over K; both operands have the reduction axis contiguous
//   dx (M x K) = dz . w        reduction over N; dz has it contiguous, w has the OUTPUT axis contiguous
//   dw (N x K) = dz^T . x      reduction over M; both operands have the output axis contiguous
//
// ONE tile kernel on v_mfma_f32_32x32x2_f32 serves the three, templated on where each operand's contiguous axis lies and on the
// epilogue; no transposed copy of anything is ever written.  The tiling is np_dnn.hip's (np_dnn_tile.h is the shared text): 4
// waves, TM x kTN outputs with TM the smallest of 32 / 64 / 128 that covers the rows, reduction steps of kTK through LDS at odd
// pitches, the reduction's tail and the tile's edges zero-filled on BOTH operands.
//
// Staging.  An operand is always read along ITS contiguous axis: stage_red for an operand whose reduction axis is contiguous
// (lanes run along k), stage_out for one whose output axis is contiguous (lanes run along the row or column of the result).
// Each has a 16-byte form, taken when the base pointer is 16-byte aligned and the row length is a multiple of 4 (tile origins are
// multiples of 32, so every vector is then aligned and lies wholly inside or wholly outside the array), and a dword form; both
// put the same values into the same LDS cells.  The lane maps are chosen so that the 32 lanes that share an LDS store cycle
// hit 32 different banks at the odd pitches: in the 16-byte forms a lane's four dwords go to four cells one pitch (or one
// dword) apart, and the 8 vectors x 4 rows (or 4 steps) of a 32-lane group cover bank 4j + c + r.
//
// Reduction order.  Every output is ONE fp32 fmaf chain from +0.0f over its reduction index ascending (the MFMA is bit for bit
// that chain), continued over the zero-filled tail.  The order for y depends on K alone and for dx on N alone: a row of x alone
// gives the bits it gives inside any batch.  dw reduces over M: when N x K has few tiles and M is long, M is cut into S slices
// of whole kTK-steps (S from the extents alone, np_dnn.hip's rule), each slice's tile goes to pool scratch and
// linear_fold_kernel adds the slices in slice order; S == 1 writes dw directly.  No float atomics.
//
// The epilogue of y: v = acc + bias[n], ONE fp32 add after the chain, then the activation, np_dnn.hip's act_apply.  The backward
// pass of the activation and db are one streaming kernel over y and dy (M, N): a workgroup owns 64 columns n and one slice of the
// rows, its lanes run along n (coalesced at any N), four row groups g = 0 .. 3 take rows m0 + g, m0 + g + 4, ... in ascending
// order from +0.0f, the four are added as ((s0 + s1) + s2) + s3, slices go to pool scratch and the fold kernel adds them in slice
// order (S == 1 writes db directly).  S is a function of (M, N) alone.
#include <limits.h>

#include "np_dnn_tile.h"

namespace {

// The multiply-adds M.K.N from which each product takes the library form (the dispatcher below).  In profiles/dnn/linear_sweep.log
// the tile form is the faster one for every product at (32, 32, 32) and (64, 64, 32), work 2^15 and 2^17, and the library form at
// (128, 64, 64), work 2^19, and at every larger y and dx: each constant is 2^18, the middle of the interval in which the faster form
// changes.  Two dw rows are on the other side of it, both with few rows M: (16, 1024, 1024), tile / library 0.74, and
// (128, 4096, 4096), 0.99; the rule is kept to one constant and the rows are recorded as findings.
#define NP_LINEAR_LIB_MIN_WORK_Y ((size_t)1 << 18)
#define NP_LINEAR_LIB_MIN_WORK_DX ((size_t)1 << 18)
#define NP_LINEAR_LIB_MIN_WORK_DW ((size_t)1 << 18)

// dz / db (tests/linear_family.py mirrors the rule): the M rows are cut into S slices,
//   want = min(M / kActMinRows, ceil(kActTargetGroups / ceil(N / kActCols)), kActMaxSlices), at least 1
//   R = ceil(M / want) rounded up to a multiple of kActGroups,  S = ceil(M / R)
constexpr int kActCols = 64, kActGroups = 4, kActMinRows = 256, kActTargetGroups = 1024, kActMaxSlices = 256;

// the products, as the probe numbers them
enum { kProdY = 0, kProdDx = 1, kProdDw = 2, kProdAct = 3, kProducts = 4 };
struct LastPath {
    int form, tm, slices, launches;
};
LastPath g_linear_last[kProducts] = {};

struct LinArgs {
    const float *a;      // the row operand: (R, L) with A_RED, (L, R) otherwise
    const float *b;      // the column operand: (Cn, L) with B_RED, (L, Cn) otherwise
    float *out;          // (R, Cn), slice s at out + s.R.Cn
    const float *bias;   // Cn floats or nullptr (EPI only)
    int R, Cn, L;
    int act;             // np_conv_act (EPI only)
    int steps_per_slice;
};

// An operand whose REDUCTION axis is contiguous: element (i, l) is src[(i0 + i).L + l0 + l] and goes to lds[i.SI + l.SL], zero
// where i0 + i >= I or l0 + l >= L.  ROWS is the tile's extent along i.  Element offsets fit 32 bits: every array has fewer than
// 2^31 elements.
template <int ROWS, int SI, int SL, bool VEC>
__device__ __forceinline__ void stage_red(float *lds, const float *__restrict__ src, int i0, int l0, int I, int L, int tid) {
    if constexpr (VEC) {
        const int l = (tid & 7) * 4, ir = tid >> 3;   // 8 vectors cover a step; 32 rows per pass
        float4 v[ROWS / 32];
#pragma unroll
        for (int u = 0; u < ROWS / 32; ++u) {
            const int i = ir + 32 * u;
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i0 + i < I && l0 + l < L) v[u] = *reinterpret_cast<const float4 *>(src + ((unsigned)(i0 + i) * (unsigned)L + (unsigned)(l0 + l)));
        }
#pragma unroll
        for (int u = 0; u < ROWS / 32; ++u) {
            float *d = lds + (ir + 32 * u) * SI + l * SL;
            d[0] = v[u].x, d[SL] = v[u].y, d[2 * SL] = v[u].z, d[3 * SL] = v[u].w;
        }
    } else {
        const int l = tid & 31, ir = tid >> 5;        // a lane per k; 8 rows per pass
        float v[ROWS / 8];
#pragma unroll
        for (int u = 0; u < ROWS / 8; ++u) {
            const int i = ir + 8 * u;
            v[u] = (i0 + i < I && l0 + l < L) ? src[(unsigned)(i0 + i) * (unsigned)L + (unsigned)(l0 + l)] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < ROWS / 8; ++u) lds[(ir + 8 * u) * SI + l * SL] = v[u];
    }
}

// An operand whose OUTPUT axis is contiguous: element (i, l) is src[(l0 + l).I + i0 + i], same destination and zero fill.
template <int ROWS, int SI, int SL, bool VEC>
__device__ __forceinline__ void stage_out(float *lds, const float *__restrict__ src, int i0, int l0, int I, int L, int tid) {
    if constexpr (VEC) {
        // 4 steps x 8 vectors per 32 lanes; ROWS / 4 vectors cover the tile's extent, 1024 / ROWS steps per pass
        constexpr int kPass = 1024 / ROWS;
        const int i = ((tid >> 2) % (ROWS / 4)) * 4, lr = (tid & 3) + 4 * (tid / ROWS);
        float4 v[kTK / kPass];
#pragma unroll
        for (int u = 0; u < kTK / kPass; ++u) {
            const int l = lr + kPass * u;
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (l0 + l < L && i0 + i < I) v[u] = *reinterpret_cast<const float4 *>(src + ((unsigned)(l0 + l) * (unsigned)I + (unsigned)(i0 + i)));
        }
#pragma unroll
        for (int u = 0; u < kTK / kPass; ++u) {
            float *d = lds + i * SI + (lr + kPass * u) * SL;
            d[0] = v[u].x, d[SI] = v[u].y, d[2 * SI] = v[u].z, d[3 * SI] = v[u].w;
        }
    } else {
        constexpr int kPass = 256 / ROWS;             // a lane per element of the extent; 256 / ROWS steps per pass
        const int i = tid % ROWS, lr = tid / ROWS;
        float v[kTK / kPass];
#pragma unroll
        for (int u = 0; u < kTK / kPass; ++u) {
            const int l = lr + kPass * u;
            v[u] = (l0 + l < L && i0 + i < I) ? src[(unsigned)(l0 + l) * (unsigned)I + (unsigned)(i0 + i)] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kTK / kPass; ++u) lds[i * SI + (lr + kPass * u) * SL] = v[u];
    }
}

// the layer's store loop for one activation: v = acc + bias[n] (one add after the chain), y = act(v).  A lane's columns are the
// same for every row: their bias is read once, and only for columns below Cn
template <int TM, int ACT>
__device__ __forceinline__ void epi_store(const dnn_v16f (&acc)[Tile<TM>::MI][Tile<TM>::NJ], float *out, const float *bias, int rw, int cw, int kq, int R,
                                          int Cn) {
    using T = Tile<TM>;
    const bool has_bias = bias != nullptr;
#pragma unroll
    for (int nj = 0; nj < T::NJ; ++nj) {
        const int col = cw + nj * 32;
        if (col >= Cn) continue;
        const float b = has_bias ? bias[col] : 0.0f;
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rw + mi * 32 + acc_row(r, kq);
                if (row >= R) continue;
                const float v = has_bias ? acc[mi][nj][r] + b : acc[mi][nj][r];
                out[(size_t)row * Cn + col] = act_apply<ACT>(v);
            }
    }
}

// grid.x = row-tiles x column-tiles, row-tiles fastest; grid.y = slices of the reduction.  Slice s reduces steps
// [s.steps_per_slice, ...) of kTK and stores its R x Cn tile at out + s.R.Cn
template <int TM, bool A_RED, bool B_RED, bool EPI, bool VA, bool VB>
__global__ __launch_bounds__(256, 2) void linear_tile_kernel(const LinArgs p) {
    using T = Tile<TM>;
    __shared__ float As[TM * kAStr];
    __shared__ float Bs[kTK * kBStr];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / T::WN, wn = wave % T::WN;
    const int tiles_r = (p.R + TM - 1) / TM;
    const int r0 = (int)(blockIdx.x % tiles_r) * TM, c0 = (int)(blockIdx.x / tiles_r) * kTN;

    dnn_v16f acc[T::MI][T::NJ];
#pragma unroll
    for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
        for (int nj = 0; nj < T::NJ; ++nj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nj][r] = 0.0f;

    const int steps = (p.L + kTK - 1) / kTK;
    const int s0 = (int)blockIdx.y * p.steps_per_slice, s1 = s0 + p.steps_per_slice < steps ? s0 + p.steps_per_slice : steps;

    for (int s = s0; s < s1; ++s) {
        const int l0 = s * kTK;
        __syncthreads();   // every wave is done with the previous step's tiles
        if constexpr (A_RED) stage_red<TM, kAStr, 1, VA>(As, p.a, r0, l0, p.R, p.L, tid);
        else stage_out<TM, kAStr, 1, VA>(As, p.a, r0, l0, p.R, p.L, tid);
        if constexpr (B_RED) stage_red<kTN, 1, kBStr, VB>(Bs, p.b, c0, l0, p.Cn, p.L, tid);
        else stage_out<kTN, 1, kBStr, VB>(Bs, p.b, c0, l0, p.Cn, p.L, tid);
        __syncthreads();
        mma_step<TM>(As, Bs, acc, wm, wn, lane);
    }

    float *out = p.out + (size_t)blockIdx.y * p.R * p.Cn;
    const int i = lane & 31, kq = lane >> 5;
    const int rw = r0 + wm * T::MI * 32, cw = c0 + wn * T::NJ * 32 + i;
    if constexpr (EPI) {
        // one compact loop per activation: the switch is taken once, not once per output
        switch (p.act) {
        case NP_ACT_RELU: epi_store<TM, NP_ACT_RELU>(acc, out, p.bias, rw, cw, kq, p.R, p.Cn); break;
        case NP_ACT_TANH: epi_store<TM, NP_ACT_TANH>(acc, out, p.bias, rw, cw, kq, p.R, p.Cn); break;
        case NP_ACT_SIGMOID: epi_store<TM, NP_ACT_SIGMOID>(acc, out, p.bias, rw, cw, kq, p.R, p.Cn); break;
        default: epi_store<TM, NP_ACT_NONE>(acc, out, p.bias, rw, cw, kq, p.R, p.Cn); break;
        }
        return;
    }
#pragma unroll
    for (int nj = 0; nj < T::NJ; ++nj) {
        const int col = cw + nj * 32;
        if (col >= p.Cn) continue;
#pragma unroll
        for (int mi = 0; mi < T::MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rw + mi * 32 + acc_row(r, kq);
                if (row < p.R) out[(size_t)row * p.Cn + col] = acc[mi][nj][r];
            }
    }
}

// out[e] = part[0][e] + part[1][e] + ... in slice order (dw: n = N.K; db: n = N)
__global__ __launch_bounds__(256) void linear_fold_kernel(const float *__restrict__ part, float *__restrict__ out, unsigned n, int slices) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    float acc = part[idx];
    for (int s = 1; s < slices; ++s) acc += part[(size_t)s * n + idx];
    out[idx] = acc;
}

// grid.x = ceil(N / kActCols), grid.y = slices.  Lane c of row group g takes column n = blockIdx.x.kActCols + c and rows
// m0 + g, m0 + g + 4, ... of slice [m0, m1).  dz == nullptr: no dz is written; out == nullptr: no sum is formed.  out[s.N + n] is
// the slice's sum (out is db when S == 1).  dz may be dy: an element is read and then written by the same lane.
template <int ACT>
__global__ __launch_bounds__(kActCols *kActGroups) void linear_act_grad_kernel(const float *y, const float *dy, float *dz, float *__restrict__ out, int M,
                                                                                int N, int rows_per_slice) {
    __shared__ float part[kActGroups][kActCols];
    const int c = (int)threadIdx.x & (kActCols - 1), g = (int)threadIdx.x / kActCols;
    const int n = (int)blockIdx.x * kActCols + c;
    const int m0 = (int)blockIdx.y * rows_per_slice, m1 = (M - m0 < rows_per_slice) ? M : m0 + rows_per_slice;
    float sum = 0.0f;
    if (n < N) {
        // four rows in flight per lane; a row is loaded, and its address used, only where it lies below m1 <= M
        for (int m = m0 + g; m < m1; m += 4 * kActGroups) {
            float gv[4], yv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int mu = m + u * kActGroups;
                const bool in = mu < m1;
                const size_t at = (size_t)mu * N + n;
                gv[u] = in ? dy[at] : 0.0f;
                yv[u] = 1.0f;
                if constexpr (ACT != NP_ACT_NONE) yv[u] = in ? y[at] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int mu = m + u * kActGroups;
                if (mu < m1) {
                    const float d = act_grad<ACT>(yv[u], gv[u]);
                    if constexpr (ACT != NP_ACT_NONE)
                        if (dz) dz[(size_t)mu * N + n] = d;
                    sum += d;
                }
            }
        }
    }
    if (!out) return;   // uniform
    part[g][c] = sum;
    __syncthreads();
    if (g == 0 && n < N) out[(size_t)blockIdx.y * N + n] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// [a, a + na) and [b, b + nb) floats share a byte; a null range overlaps nothing
bool overlaps(const float *a, size_t na, const float *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb * sizeof(float) && pb < pa + na * sizeof(float);
}

int check_extents(const char *who, size_t M, size_t K, size_t N, int act) {
    if (M < 1 || K < 1 || N < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (mul_lim(M, N) >= kLim || mul_lim(M, K) >= kLim || mul_lim(N, K) >= kLim)
        return np::fail(NP_ERR_INVALID, "%s: an operand or a result has 2^31 elements or more", who);
    if (act < NP_ACT_NONE || act > NP_ACT_SIGMOID) return np::fail(NP_ERR_INVALID, "%s: unknown activation %d", who, act);
    return NP_OK;
}

bool vec_ok(const float *p, size_t row_length) { return ((uintptr_t)p & 15u) == 0 && (row_length & 3) == 0; }

template <bool A_RED, bool B_RED, bool EPI, bool VA, bool VB>
void launch_tile_as(int tm, dim3 grid, const LinArgs &p) {
    const dim3 block(256);
    if (tm == kTMSmall) linear_tile_kernel<kTMSmall, A_RED, B_RED, EPI, VA, VB><<<grid, block, 0, np::stream()>>>(p);
    else if (tm == kTMMid) linear_tile_kernel<kTMMid, A_RED, B_RED, EPI, VA, VB><<<grid, block, 0, np::stream()>>>(p);
    else linear_tile_kernel<kTMLarge, A_RED, B_RED, EPI, VA, VB><<<grid, block, 0, np::stream()>>>(p);
}

// va, vb: the operand takes 16-byte loads (vec_ok of its pointer and row length)
template <bool A_RED, bool B_RED, bool EPI>
void launch_tile(int tm, dim3 grid, const LinArgs &p, bool va, bool vb) {
    if (va && vb) launch_tile_as<A_RED, B_RED, EPI, true, true>(tm, grid, p);
    else if (va) launch_tile_as<A_RED, B_RED, EPI, true, false>(tm, grid, p);
    else if (vb) launch_tile_as<A_RED, B_RED, EPI, false, true>(tm, grid, p);
    else launch_tile_as<A_RED, B_RED, EPI, false, false>(tm, grid, p);
}

// the launch shape of one product: the tile's rows and, for dw, the slices of its reduction, from the extents alone
struct TilePlan {
    int tm;
    size_t tiles, steps_per_slice, slices;
};

TilePlan plan_tile(size_t R, size_t Cn, size_t L, bool sliced) {
    TilePlan pl;
    pl.tm = pick_tm(R);
    pl.tiles = ((R + pl.tm - 1) / pl.tm) * ((Cn + kTN - 1) / kTN);   // R.Cn < 2^31: fits a launch
    const size_t steps = (L + kTK - 1) / kTK;
    size_t want = 1;
    if (sliced) {
        const size_t fill = (kWgradTargetGroups + pl.tiles - 1) / pl.tiles;
        want = steps / kWgradMinSteps;
        if (want > fill) want = fill;
        if (want > (size_t)kWgradMaxSlices) want = kWgradMaxSlices;
        if (want < 1) want = 1;
    }
    pl.steps_per_slice = (steps + want - 1) / want;
    pl.slices = (steps + pl.steps_per_slice - 1) / pl.steps_per_slice;
    return pl;
}

struct ActPlan {
    size_t rows_per_slice, slices;
};

ActPlan plan_act(size_t M, size_t N) {
    const size_t col_groups = (N + kActCols - 1) / kActCols;
    size_t want = M / kActMinRows, fill = (kActTargetGroups + col_groups - 1) / col_groups;
    if (want > fill) want = fill;
    if (want > (size_t)kActMaxSlices) want = kActMaxSlices;
    if (want < 1) want = 1;
    ActPlan pl;
    pl.rows_per_slice = ((M + want - 1) / want + kActGroups - 1) / kActGroups * kActGroups;
    pl.slices = (M + pl.rows_per_slice - 1) / pl.rows_per_slice;
    return pl;
}

void note(int product, int tm, size_t slices, int launches) { g_linear_last[product] = {1, tm, (int)slices, launches}; }

// ---- the two forms ----
// Form 1, the tile form above: one chain per output, batch invariant.  Form 2, the library form: the product goes through np_sgemm,
// the operand that np_sgemm needs the other way round is first written to pool scratch by np_transpose2d (w for y, dz for dw; dx
// needs none), bias and activation are one in-place pass over y.  Its bits are those of the public calls in that order; np_sgemm's
// plan depends on M, so batch invariance holds for form 1 only.  The form is chosen per product from (M, K, N) alone: the library
// form from kLibMinWork[product] multiply-adds M.K.N up.  The constants are where the faster form changes in
// profiles/dnn/linear_sweep.log (both forms forced per product on the grid of tools/dnn_sweep.py --linear); DESIGN.md 3.21.
constexpr size_t kLibMinWork[3] = {NP_LINEAR_LIB_MIN_WORK_Y, NP_LINEAR_LIB_MIN_WORK_DX, NP_LINEAR_LIB_MIN_WORK_DW};
int g_linear_force_form = 0;   // 0: by the extents; 1, 2: every product takes that form (np_debug_linear_force_form)

int form_for(int product, size_t M, size_t K, size_t N) {
    if (g_linear_force_form) return g_linear_force_form;
    return M * K * N >= kLibMinWork[product] ? 2 : 1;   // M.N < 2^31 and K < 2^31: no overflow
}

// the library form's record: no tile, no slices of this unit's; the launches are counted from the library's counter
void note_lib(int product, unsigned long long launches_before) {
    g_linear_last[product] = {2, 0, 0, (int)(__atomic_load_n(&np::g_launch_count, __ATOMIC_RELAXED) - launches_before)};
}

// y[m, n] = act(y[m, n] + bias[n]) in place: ONE fp32 add, then the activation, the tile form's epilogue on stored values
template <int ACT>
__global__ __launch_bounds__(256) void linear_bias_act_kernel(float *__restrict__ y, const float *__restrict__ bias, unsigned total, unsigned N) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const float v = bias ? y[idx] + bias[idx % N] : y[idx];
    y[idx] = act_apply<ACT>(v);
}

int lib_forward(const float *x, const float *w, const float *bias, size_t M, size_t K, size_t N, int act, float *y) {
    const unsigned long long before = __atomic_load_n(&np::g_launch_count, __ATOMIC_RELAXED);
    np::Scratch wt;   // w^T (K, N); released on every path below
    if (int rc = wt.alloc(N * K * sizeof(float))) return rc;
    if (int rc = np_transpose2d(w, (float *)wt.ptr, 1, N, K)) return rc;
    if (int rc = np_sgemm(M, N, K, x, (const float *)wt.ptr, y)) return rc;
    if (bias || act != NP_ACT_NONE) {
        const unsigned total = (unsigned)(M * N);
        const dim3 grid((total + 255) / 256), block(256);
        if (act == NP_ACT_RELU) linear_bias_act_kernel<NP_ACT_RELU><<<grid, block, 0, np::stream()>>>(y, bias, total, (unsigned)N);
        else if (act == NP_ACT_TANH) linear_bias_act_kernel<NP_ACT_TANH><<<grid, block, 0, np::stream()>>>(y, bias, total, (unsigned)N);
        else if (act == NP_ACT_SIGMOID) linear_bias_act_kernel<NP_ACT_SIGMOID><<<grid, block, 0, np::stream()>>>(y, bias, total, (unsigned)N);
        else linear_bias_act_kernel<NP_ACT_NONE><<<grid, block, 0, np::stream()>>>(y, bias, total, (unsigned)N);
        NP_LAUNCH_CHECK("linear_bias_act_kernel");
    }
    note_lib(kProdY, before);
    return NP_OK;
}

int lib_dx(const float *g, const float *w, size_t M, size_t K, size_t N, float *dx) {
    const unsigned long long before = __atomic_load_n(&np::g_launch_count, __ATOMIC_RELAXED);
    if (int rc = np_sgemm(M, K, N, g, w, dx)) return rc;   // (M, N) . (N, K): both operands lie as np_sgemm takes them
    note_lib(kProdDx, before);
    return NP_OK;
}

int lib_dw(const float *g, const float *x, size_t M, size_t K, size_t N, float *dw) {
    const unsigned long long before = __atomic_load_n(&np::g_launch_count, __ATOMIC_RELAXED);
    np::Scratch gt;   // dz^T (N, M); released on every path below
    if (int rc = gt.alloc(M * N * sizeof(float))) return rc;
    if (int rc = np_transpose2d(g, (float *)gt.ptr, 1, M, N)) return rc;
    if (int rc = np_sgemm(N, K, M, (const float *)gt.ptr, x, dw)) return rc;
    note_lib(kProdDw, before);
    return NP_OK;
}

// y = act(x . w^T + bias)
int launch_forward(const float *x, const float *w, const float *bias, size_t M, size_t K, size_t N, int act, float *y) {
    const TilePlan pl = plan_tile(M, N, K, false);
    const LinArgs p = {x, w, y, bias, (int)M, (int)N, (int)K, act, (int)pl.steps_per_slice};
    launch_tile<true, true, true>(pl.tm, dim3((unsigned)pl.tiles), p, vec_ok(x, K), vec_ok(w, K));
    NP_LAUNCH_CHECK("linear_tile_kernel");
    note(kProdY, pl.tm, 1, 1);
    return NP_OK;
}

// dx = g . w
int launch_dx(const float *g, const float *w, size_t M, size_t K, size_t N, float *dx) {
    const TilePlan pl = plan_tile(M, K, N, false);
    const LinArgs p = {g, w, dx, nullptr, (int)M, (int)K, (int)N, NP_ACT_NONE, (int)pl.steps_per_slice};
    launch_tile<true, false, false>(pl.tm, dim3((unsigned)pl.tiles), p, vec_ok(g, N), vec_ok(w, K));
    NP_LAUNCH_CHECK("linear_tile_kernel");
    note(kProdDx, pl.tm, 1, 1);
    return NP_OK;
}

// dw = g^T . x, in slices of M
int launch_dw(const float *g, const float *x, size_t M, size_t K, size_t N, float *dw) {
    const TilePlan pl = plan_tile(N, K, M, true);
    np::Scratch part;   // released on every path below
    if (pl.slices > 1)
        if (int rc = part.alloc(pl.slices * N * K * sizeof(float))) return rc;
    const LinArgs p = {g, x, pl.slices > 1 ? (float *)part.ptr : dw, nullptr, (int)N, (int)K, (int)M, NP_ACT_NONE, (int)pl.steps_per_slice};
    launch_tile<false, false, false>(pl.tm, dim3((unsigned)pl.tiles, (unsigned)pl.slices), p, vec_ok(g, N), vec_ok(x, K));
    NP_LAUNCH_CHECK("linear_tile_kernel");
    if (pl.slices > 1) {
        const size_t numel = N * K;
        linear_fold_kernel<<<dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, np::stream()>>>((const float *)part.ptr, dw, (unsigned)numel,
                                                                                                  (int)pl.slices);
        NP_LAUNCH_CHECK("linear_fold_kernel");
    }
    note(kProdDw, pl.tm, pl.slices, pl.slices > 1 ? 2 : 1);
    return NP_OK;
}

template <int ACT>
void launch_act_as(dim3 grid, const float *y, const float *dy, float *dz, float *out, int M, int N, int rows_per_slice) {
    linear_act_grad_kernel<ACT><<<grid, dim3(kActCols * kActGroups), 0, np::stream()>>>(y, dy, dz, out, M, N, rows_per_slice);
}

// dz = dy . act'(y) (not written with NP_ACT_NONE, or when dz is nullptr) and db (when not nullptr)
int launch_act_grad(const float *y, const float *dy, size_t M, size_t N, int act, float *dz, float *db) {
    const ActPlan pl = plan_act(M, N);
    np::Scratch part;   // released on every path below
    if (db && pl.slices > 1)
        if (int rc = part.alloc(pl.slices * N * sizeof(float))) return rc;
    float *out = !db ? nullptr : pl.slices > 1 ? (float *)part.ptr : db;
    const dim3 grid((unsigned)((N + kActCols - 1) / kActCols), (unsigned)pl.slices);
    const int rows = (int)pl.rows_per_slice;
    if (act == NP_ACT_RELU) launch_act_as<NP_ACT_RELU>(grid, y, dy, dz, out, (int)M, (int)N, rows);
    else if (act == NP_ACT_TANH) launch_act_as<NP_ACT_TANH>(grid, y, dy, dz, out, (int)M, (int)N, rows);
    else if (act == NP_ACT_SIGMOID) launch_act_as<NP_ACT_SIGMOID>(grid, y, dy, dz, out, (int)M, (int)N, rows);
    else launch_act_as<NP_ACT_NONE>(grid, y, dy, nullptr, out, (int)M, (int)N, rows);
    NP_LAUNCH_CHECK("linear_act_grad_kernel");
    const bool fold = db && pl.slices > 1;
    if (fold) {
        linear_fold_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, np::stream()>>>((const float *)part.ptr, db, (unsigned)N, (int)pl.slices);
        NP_LAUNCH_CHECK("linear_fold_kernel");
    }
    note(kProdAct, 0, pl.slices, fold ? 2 : 1);
    return NP_OK;
}

}  // namespace

extern "C" {

int np_linear_forward(const float *x, const float *w, const float *bias, size_t M, size_t K, size_t N, int act, float *y) {
    const char *who = "np_linear_forward";
    if (!x || !w || !y) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    if (int rc = check_extents(who, M, K, N, act)) return rc;
    if (overlaps(y, M * N, x, M * K) || overlaps(y, M * N, w, N * K) || overlaps(y, M * N, bias, N))
        return np::fail(NP_ERR_INVALID, "%s: y overlaps an operand", who);
    if (int rc = np::ensure_init()) return rc;
    if (form_for(kProdY, M, K, N) == 2) return lib_forward(x, w, bias, M, K, N, act, y);
    return launch_forward(x, w, bias, M, K, N, act, y);
}

int np_linear_backward(const float *x, const float *w, const float *y, const float *dy, size_t M, size_t K, size_t N, int act, float *dz, float *dx,
                       float *dw, float *db) {
    const char *who = "np_linear_backward";
    if (!dy) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    if (!dx && !dw && !db) return np::fail(NP_ERR_INVALID, "%s: null pointer: dx, dw and db are all null, nothing is asked for", who);
    if ((dx && !w) || (dw && !x)) return np::fail(NP_ERR_INVALID, "%s: null pointer: dx needs w and dw needs x", who);
    if (int rc = check_extents(who, M, K, N, act)) return rc;
    const bool has_act = act != NP_ACT_NONE;
    if (has_act && (!y || (!dz && (dx || dw))))
        return np::fail(NP_ERR_INVALID, "%s: null pointer: an activation needs y, and dz where dx or dw is asked for", who);
    // the ranges the call reads and writes; with NP_ACT_NONE y and dz are not touched
    const float *yr = has_act ? y : nullptr;
    float *dzw = has_act ? dz : nullptr;
    const float *xr = dw ? x : nullptr, *wr = dx ? w : nullptr;
    const size_t MN = M * N, MK = M * K, NK = N * K;
    if (dzw && dzw != dy && overlaps(dzw, MN, dy, MN)) return np::fail(NP_ERR_INVALID, "%s: dz overlaps dy without being dy", who);
    const bool bad = overlaps(dzw, MN, yr, MN) || overlaps(dzw, MN, xr, MK) || overlaps(dzw, MN, wr, NK) || overlaps(dzw, MN, dx, MK) ||
                     overlaps(dzw, MN, dw, NK) || overlaps(dzw, MN, db, N) ||   //
                     overlaps(dx, MK, xr, MK) || overlaps(dx, MK, wr, NK) || overlaps(dx, MK, yr, MN) || overlaps(dx, MK, dy, MN) ||
                     overlaps(dx, MK, dw, NK) || overlaps(dx, MK, db, N) ||   //
                     overlaps(dw, NK, xr, MK) || overlaps(dw, NK, wr, NK) || overlaps(dw, NK, yr, MN) || overlaps(dw, NK, dy, MN) ||
                     overlaps(dw, NK, db, N) ||   //
                     overlaps(db, N, xr, MK) || overlaps(db, N, wr, NK) || overlaps(db, N, yr, MN) || overlaps(db, N, dy, MN);
    if (bad) return np::fail(NP_ERR_INVALID, "%s: a result overlaps an operand or another result", who);
    if (int rc = np::ensure_init()) return rc;
    g_linear_last[kProdDx] = g_linear_last[kProdDw] = g_linear_last[kProdAct] = {};
    if (has_act || db)
        if (int rc = launch_act_grad(yr, dy, M, N, act, dzw, db)) return rc;
    const float *g = has_act ? dzw : dy;
    if (dx)
        if (int rc = form_for(kProdDx, M, K, N) == 2 ? lib_dx(g, w, M, K, N, dx) : launch_dx(g, w, M, K, N, dx)) return rc;
    if (dw)
        if (int rc = form_for(kProdDw, M, K, N) == 2 ? lib_dw(g, x, M, K, N, dw) : launch_dw(g, x, M, K, N, dw)) return rc;
    return NP_OK;
}

// ---- the probes ----

int np_debug_linear_last_path(int product, int *form, int *tm, int *slices, int *launches) {
    if (!form || !tm || !slices || !launches) return np::fail(NP_ERR_INVALID, "np_debug_linear_last_path: null pointer");
    if (product < 0 || product >= kProducts) return np::fail(NP_ERR_INVALID, "np_debug_linear_last_path: unknown product %d", product);
    const LastPath &l = g_linear_last[product];
    *form = l.form, *tm = l.tm, *slices = l.slices, *launches = l.launches;
    return NP_OK;
}

int np_debug_linear_force_form(int form) {
    if (form != 0 && form != 1 && form != 2) return np::fail(NP_ERR_INVALID, "np_debug_linear_force_form: the form is 0 (by the extents), 1 (tile) or 2 (library)");
    g_linear_force_form = form;
    return NP_OK;
}

int np_debug_linear_bounds(size_t bounds[], int n) {
    if (!bounds || n < 16) return np::fail(NP_ERR_INVALID, "np_debug_linear_bounds: null pointer or fewer than 16 slots");
    const size_t v[16] = {kTMSmall, kTMMid, kTMLarge, kTN, kTK, kWgradMinSteps, kWgradTargetGroups, kWgradMaxSlices,
                          kActCols, kActGroups, kActMinRows, kActTargetGroups, kActMaxSlices, kLibMinWork[0], kLibMinWork[1], kLibMinWork[2]};
    for (int i = 0; i < 16; ++i) bounds[i] = v[i];
    return NP_OK;
}

}  // extern "C"
