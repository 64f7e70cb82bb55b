// Householder QR on ROW-MAJOR m x n matrices, m >= n: np_geqrf (in place, packed reflectors + tau), np_qr (reduced Q and R)
// and np_lstsq (min ||a x - b|| through Q^T b and a back-substitution).  Blocked compact WY with panels of
// kNB columns; convention LAPACK's sgeqr2 / slarfg (include/np_hip.h states it).  Shares with np_lu.hip and np_cholesky.hip
// only what np_linalg_common.h holds.
//
//   per panel   qr_panel_kernel   one workgroup factors the (m - j0) x w panel column by column and builds the w x w
//                                 triangular T (and T^T) of H_j0 ... H_j0+w-1 = I - V T V^T.  The column norm and every
//                                 v . x inner product are accumulated in fp64 and rounded once.
//               qr_unpack_kernel  V (explicit ones and zeros, row stride w) and V^T from the packed panel into scratch:
//                                 np::sgemm_sub_ld takes no transposed operand.  The same kernel serves the factorization,
//                                 the formation of Q and Q^T b, which read the reflectors back from the packed factor.
//               apply_block       C -= V (T' (V^T C)) as three np::sgemm_sub_ld launches on the MFMA tile kernel: into a
//                                 zeroed W it leaves -V^T C, into a zeroed Z with T' it leaves +T' V^T C, then C -= V Z.
//                                 T' = T^T applies the block's H^T (trailing update, Q^T b), T' = T applies H (forming Q).
//   np_qr       factors a pool copy, extracts R (strict lower triangle +0.0f), then applies the blocks in REVERSE order to
//               I[:, :n], block b only to rows and columns >= its first column (the rest of those rows is still zero).
//   np_lstsq    factors a pool copy, finds the first zero on R's diagonal on the device, applies the blocks in forward order
//               to a copy of b and solves R x = (Q^T b)[:n] block by block from the bottom (qr_upper_block_kernel on the
//               diagonal block, np::sgemm_sub_ld for the rows above it).
// No iteration, no float atomics, every fold in a fixed order: bit-identical from run to run.
#include "np_linalg_common.h"

namespace {

using namespace np::linalg;

constexpr int kPanelThreads = 1024;
constexpr int kPanelGroups = kPanelThreads / kNB;   // row groups of the panel kernel: thread (g, k) owns column k of rows g, g + 16, ...
constexpr size_t kQrMaxM = (size_t)1 << 24;         // rows: the GEMM launches and the unpack grid take 32-bit extents
constexpr int kTPair = 2 * kNB * kNB;               // floats per block in the T store: T, then T^T, both with row stride kNB
constexpr int kSolvePad = kNB + 1;

// the sum of one double per thread over the workgroup, in a fixed order, in every thread (lds: kPanelGroups doubles)
__device__ __forceinline__ double panel_sum(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int g = 0; g < kPanelGroups; ++g) r += lds[g];
    __syncthreads();
    return r;
}

// Factors the mp x w panel at A (row stride lda, w <= kNB, mp >= 1) in place: R on and above the diagonal, v_j below it
// (v_j[j] = 1 implied), tau[0 .. w).  T_out: kTPair floats, T and T^T of the block, zero outside the leading w x w.
// slarfg: alpha = a_jj, x = the column below it; x == 0 exactly: tau = 0, nothing else changes.  Otherwise
// beta = -sign(alpha) ||(alpha, x)||, sign(+-0) = +, tau = (beta - alpha) / beta, v = x / (alpha - beta), a_jj = beta.
__global__ __launch_bounds__(kPanelThreads) void qr_panel_kernel(float *A, size_t lda, size_t mp, int w, float *tau, float *T_out) {
    __shared__ double red[kPanelGroups * kNB];
    __shared__ double wsum[kPanelGroups];
    __shared__ float T[kNB * kNB];
    __shared__ float z[kNB];
    __shared__ float s_tau, s_denom, s_beta;
    const int tid = threadIdx.x, k = tid & 63, g = tid >> 6;
    for (int e = tid; e < kNB * kNB; e += kPanelThreads) T[e] = 0.0f;
    __syncthreads();
    for (int j = 0; j < w; ++j) {
        float *col = A + j;
        double s = 0.0;
        for (size_t i = (size_t)j + 1 + tid; i < mp; i += kPanelThreads) {
            const double x = (double)col[i * lda];
            s += x * x;
        }
        const double ssq = panel_sum(s, wsum);
        if (tid == 0) {
            const float alpha = col[(size_t)j * lda];
            float t = 0.0f, beta = alpha, denom = 1.0f;
            if (ssq != 0.0) {   // NaN takes this branch and propagates
                const float nrm = (float)sqrt((double)alpha * (double)alpha + ssq);
                beta = alpha < 0.0f ? nrm : -nrm;
                t = __fdiv_rn(__fsub_rn(beta, alpha), beta);
                denom = __fsub_rn(alpha, beta);
            }
            s_tau = t;
            s_denom = denom;
            s_beta = beta;
            tau[j] = t;
        }
        __syncthreads();
        const float tj = s_tau, denom = s_denom;
        if (tj != 0.0f) {   // the same in every thread
            for (size_t i = (size_t)j + 1 + tid; i < mp; i += kPanelThreads) col[i * lda] = __fdiv_rn(col[i * lda], denom);   // v_j
            if (tid == 0) col[(size_t)j * lda] = s_beta;
            __syncthreads();
            // z_k = v^T (column k): for k > j the inner product the update needs, for k < j (V^T v_j)_k, which T's column needs
            double acc = 0.0;
            if (k < w && k != j) {
#pragma unroll 4
                for (size_t i = (size_t)j + 1 + g; i < mp; i += kPanelGroups) acc += (double)col[i * lda] * (double)A[i * lda + k];
            }
            red[g * kNB + k] = acc;
            __syncthreads();
            if (tid < w && tid != j) {
                double total = (double)A[(size_t)j * lda + tid];   // v_j[j] = 1
                for (int q = 0; q < kPanelGroups; ++q) total += red[q * kNB + tid];
                z[tid] = (float)total;
            }
            __syncthreads();
            if (tid < j) {   // T[:j, j] = -tau_j T[:j, :j] (V^T v_j)
                float sum = 0.0f;
                for (int l = tid; l < j; ++l) sum += T[tid * kNB + l] * z[l];
                T[tid * kNB + j] = -tj * sum;
            }
            if (tid == j) T[j * kNB + j] = tj;
            if (k > j && k < w) {   // a_ik -= v_i (tau z_k)
                const float t = __fmul_rn(tj, z[k]);
                if (g == 0) A[(size_t)j * lda + k] = __fsub_rn(A[(size_t)j * lda + k], t);
#pragma unroll 4
                for (size_t i = (size_t)j + 1 + g; i < mp; i += kPanelGroups)
                    A[i * lda + k] = __fsub_rn(A[i * lda + k], __fmul_rn(col[i * lda], t));
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < kNB * kNB; e += kPanelThreads) {
        T_out[e] = T[e];
        T_out[kNB * kNB + (e & 63) * kNB + (e >> 6)] = T[e];
    }
}

// V (mp x w, row stride w) and Vt (w x mp, row stride ldv) := the unit lower trapezoid of the packed mp x w panel at A
__global__ __launch_bounds__(256) void qr_unpack_kernel(const float *A, size_t lda, size_t mp, int w, float *V, float *Vt, size_t ldv) {
    const int c = threadIdx.x & 63;
    if (c >= w) return;
    const size_t first = (size_t)blockIdx.x * kNB + (threadIdx.x >> 6);
#pragma unroll 4
    for (int t = 0; t < kNB / 4; ++t) {
        const size_t i = first + 4 * (size_t)t;
        if (i >= mp) break;
        const float v = i < (size_t)c ? 0.0f : (i == (size_t)c ? 1.0f : A[i * lda + c]);
        V[i * w + c] = v;
        Vt[(size_t)c * ldv + i] = v;
    }
}

// R (n x n, dense) := the upper triangle of the factored A (row stride lda), strict lower triangle +0.0f
__global__ __launch_bounds__(256) void qr_extract_r_kernel(const float *A, size_t lda, size_t n, float *R) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (size_t r = blockIdx.y; r < n; r += gridDim.y) R[r * n + c] = c >= r ? A[r * lda + c] : 0.0f;
}

// Q (m x n, dense) := I[:, :n]
__global__ __launch_bounds__(256) void qr_eye_kernel(float *Q, size_t m, size_t n) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (size_t r = blockIdx.y; r < m; r += gridDim.y) Q[r * n + c] = r == c ? 1.0f : 0.0f;
}

// *info := 1 + the first j with R_jj == 0, else 0 (R: the factored A, row stride lda)
__global__ __launch_bounds__(1024) void qr_diag_info_kernel(const float *A, size_t lda, size_t n, int *info) {
    __shared__ unsigned first;
    if (threadIdx.x == 0) first = 0xffffffffu;
    __syncthreads();
    for (size_t j = threadIdx.x; j < n; j += blockDim.x) {
        if (A[j * lda + j] == 0.0f) {
            atomicMin(&first, (unsigned)j);
            break;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *info = first == 0xffffffffu ? 0 : (int)first + 1;
}

// X[k0 .. k0 + nb) := R[k0 .., k0 ..]^-1 X[k0 .. k0 + nb): the nb x nb upper-triangular diagonal block of R (row stride ldr)
// against nb rows of the row-major X (row stride ldx, nrhs columns), a right-hand side per lane
__global__ __launch_bounds__(kNB) void qr_upper_block_kernel(const float *R, size_t ldr, size_t k0, int nb, float *X, size_t ldx, size_t nrhs) {
    __shared__ float Rs[kNB * kSolvePad];
    __shared__ float Xs[kNB * kSolvePad];
    const int lane = threadIdx.x;
    const size_t col = (size_t)blockIdx.x * kNB + lane;
    for (int r = 0; r < nb; ++r) {
        Rs[r * kSolvePad + lane] = lane < nb ? R[(k0 + r) * ldr + k0 + lane] : 0.0f;
        Xs[r * kSolvePad + lane] = col < nrhs ? X[(k0 + r) * ldx + col] : 0.0f;
    }
    __syncthreads();
    for (int i = nb - 1; i >= 0; --i) {
        float s = Xs[i * kSolvePad + lane];
        for (int q = i + 1; q < nb; ++q) s -= Rs[i * kSolvePad + q] * Xs[q * kSolvePad + lane];
        Xs[i * kSolvePad + lane] = __fdiv_rn(s, Rs[i * kSolvePad + i]);
    }
    if (col < nrhs)
        for (int r = 0; r < nb; ++r) X[(k0 + r) * ldx + col] = Xs[r * kSolvePad + lane];
}

// ---- host side ----

inline size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

// the pool scratch of one call: V, V^T, W, Z and the T store (every block's T and T^T)
struct QrWork {
    np::Scratch mem;
    float *V = nullptr, *Vt = nullptr, *W = nullptr, *T = nullptr;   // W: kNB x ldw, Z right behind it
    size_t ldv = 0, ldw = 0;
    int alloc(size_t m, size_t n, size_t widest) {   // widest: the most columns a block is ever applied to
        ldv = round4(m);
        ldw = round4(widest);
        const size_t blocks = (n + kNB - 1) / kNB;
        const size_t floats = round4(m * kNB) + (size_t)kNB * ldv + 2 * (size_t)kNB * ldw + blocks * kTPair;
        if (int rc = mem.alloc(floats * sizeof(float))) return rc;
        V = (float *)mem.ptr;
        Vt = V + round4(m * kNB);
        W = Vt + (size_t)kNB * ldv;
        T = W + 2 * (size_t)kNB * ldw;
        return NP_OK;
    }
};

int unpack(const float *panel, size_t lda, size_t mp, int w, QrWork &k) {
    qr_unpack_kernel<<<blocks_for(mp, kNB), 256, 0, np::stream()>>>(panel, lda, mp, w, k.V, k.Vt, k.ldv);
    NP_LAUNCH_CHECK("qr_unpack_kernel");
    return NP_OK;
}

// C (mp x nc, row stride ldc) -= V (Tm (V^T C)) for the block whose V / V^T sit in k; Tm: w x w with row stride kNB
int apply_block(float *C, size_t ldc, size_t mp, size_t nc, int w, const float *Tm, QrWork &k) {
    if (nc == 0) return NP_OK;
    float *W = k.W, *Z = k.W + (size_t)kNB * k.ldw;
    NP_HIP_CHECK(hipMemsetAsync(W, 0, 2 * (size_t)kNB * k.ldw * sizeof(float), np::stream()));
    if (int rc = np::sgemm_sub_ld((size_t)w, nc, mp, k.Vt, k.ldv, C, ldc, W, k.ldw)) return rc;      // W = -V^T C
    if (int rc = np::sgemm_sub_ld((size_t)w, nc, (size_t)w, Tm, kNB, W, k.ldw, Z, k.ldw)) return rc;  // Z = +Tm V^T C
    return np::sgemm_sub_ld(mp, nc, (size_t)w, k.V, (size_t)w, Z, k.ldw, C, ldc);                     // C -= V Z
}

// the blocked factorization of A (m x n, row stride lda) in place; k.T receives every block's T and T^T
int geqrf_blocked(float *A, size_t lda, size_t m, size_t n, float *tau, QrWork &k) {
    hipStream_t s = np::stream();
    for (size_t j0 = 0; j0 < n; j0 += kNB) {
        const int w = (int)(n - j0 < (size_t)kNB ? n - j0 : kNB);
        float *panel = A + j0 * lda + j0, *T = k.T + j0 / kNB * kTPair;
        qr_panel_kernel<<<1, kPanelThreads, 0, s>>>(panel, lda, m - j0, w, tau + j0, T);
        NP_LAUNCH_CHECK("qr_panel_kernel");
        if (j0 + w < n) {
            if (int rc = unpack(panel, lda, m - j0, w, k)) return rc;
            if (int rc = apply_block(panel + w, lda, m - j0, n - j0 - w, w, T + kNB * kNB, k)) return rc;
        }
    }
    return NP_OK;
}

int check_shape(const char *who, size_t m, size_t n) {
    if (m < n) return np::fail(NP_ERR_INVALID, "%s: m = %zu is smaller than n = %zu (only m >= n is factored)", who, m, n);
    if (m > kQrMaxM || n > kMaxBlockedN)
        return np::fail(NP_ERR_INVALID, "%s: %zu x %zu is larger than %zu x %zu", who, m, n, kQrMaxM, kMaxBlockedN);
    return NP_OK;
}

}  // namespace

extern "C" {

int np_geqrf(float *a, size_t m, size_t n, float *tau) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !tau) return np::fail(NP_ERR_INVALID, "np_geqrf: null pointer");
    if (int rc = check_shape("np_geqrf", m, n)) return rc;
    if (n == 0) return NP_OK;
    QrWork k;
    if (int rc = k.alloc(m, n, n)) return rc;
    return geqrf_blocked(a, n, m, n, tau, k);
}

int np_qr(const float *a, size_t m, size_t n, float *q, float *r) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !q || !r) return np::fail(NP_ERR_INVALID, "np_qr: null pointer");
    if (int rc = check_shape("np_qr", m, n)) return rc;
    if (n == 0) return NP_OK;
    hipStream_t s = np::stream();
    QrWork k;
    np::Scratch work;
    if (int rc = k.alloc(m, n, n)) return rc;
    if (int rc = work.alloc((m * n + n) * sizeof(float))) return rc;
    float *A = (float *)work.ptr, *tau = A + m * n;
    NP_HIP_CHECK(hipMemcpyAsync(A, a, m * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (int rc = geqrf_blocked(A, n, m, n, tau, k)) return rc;
    const unsigned gx = blocks_for(n, 256);
    qr_extract_r_kernel<<<dim3(gx, (unsigned)(n < 4096 ? n : 4096)), 256, 0, s>>>(A, n, n, r);
    NP_LAUNCH_CHECK("qr_extract_r_kernel");
    qr_eye_kernel<<<dim3(gx, (unsigned)(m < 4096 ? m : 4096)), 256, 0, s>>>(q, m, n);
    NP_LAUNCH_CHECK("qr_eye_kernel");
    for (size_t j0 = (n - 1) / kNB * kNB;; j0 -= kNB) {   // Q = H_0 ... H_{n-1} I[:, :n]: the last block first
        const int w = (int)(n - j0 < (size_t)kNB ? n - j0 : kNB);
        if (int rc = unpack(A + j0 * n + j0, n, m - j0, w, k)) return rc;
        if (int rc = apply_block(q + j0 * n + j0, n, m - j0, n - j0, w, k.T + j0 / kNB * kTPair, k)) return rc;
        if (j0 == 0) break;
    }
    return NP_OK;
}

int np_lstsq(const float *a, const float *b, size_t m, size_t n, size_t nrhs, float *x, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !b || !x || !info_host) return np::fail(NP_ERR_INVALID, "np_lstsq: null pointer");
    if (int rc = check_shape("np_lstsq", m, n)) return rc;
    if (nrhs > 0x7fffffffu) return np::fail(NP_ERR_INVALID, "np_lstsq: nrhs = %zu is too large", nrhs);
    *info_host = 0;
    if (n == 0 || nrhs == 0) return NP_OK;
    hipStream_t s = np::stream();
    QrWork k;
    np::Scratch work, info;
    if (int rc = k.alloc(m, n, n > nrhs ? n : nrhs)) return rc;
    if (int rc = work.alloc((round4(m * n) + round4(n) + m * nrhs) * sizeof(float))) return rc;
    if (int rc = info.alloc(sizeof(int))) return rc;
    float *A = (float *)work.ptr, *tau = A + round4(m * n), *C = tau + round4(n);
    NP_HIP_CHECK(hipMemcpyAsync(A, a, m * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (int rc = geqrf_blocked(A, n, m, n, tau, k)) return rc;
    qr_diag_info_kernel<<<1, 1024, 0, s>>>(A, n, n, (int *)info.ptr);
    NP_LAUNCH_CHECK("qr_diag_info_kernel");
    if (int rc = read_info((const int *)info.ptr, info_host)) return rc;
    if (*info_host != 0) return NP_OK;   // sgels' rule: x is not written
    NP_HIP_CHECK(hipMemcpyAsync(C, b, m * nrhs * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (size_t j0 = 0; j0 < n; j0 += kNB) {   // C := Q^T b = H_{n-1} ... H_0 b: the first block first
        const int w = (int)(n - j0 < (size_t)kNB ? n - j0 : kNB);
        if (int rc = unpack(A + j0 * n + j0, n, m - j0, w, k)) return rc;
        if (int rc = apply_block(C + j0 * nrhs, nrhs, m - j0, nrhs, w, k.T + j0 / kNB * kTPair + kNB * kNB, k)) return rc;
    }
    for (size_t k0 = (n - 1) / kNB * kNB;; k0 -= kNB) {   // R x = C[:n] from the bottom block upwards
        const int nb = (int)(n - k0 < (size_t)kNB ? n - k0 : kNB);
        qr_upper_block_kernel<<<blocks_for(nrhs, kNB), kNB, 0, s>>>(A, n, k0, nb, C, nrhs, nrhs);
        NP_LAUNCH_CHECK("qr_upper_block_kernel");
        if (k0 == 0) break;
        if (int rc = np::sgemm_sub_ld(k0, nrhs, (size_t)nb, A + k0, n, C + k0 * nrhs, nrhs, C, nrhs)) return rc;
    }
    NP_HIP_CHECK(hipMemcpyAsync(x, C, n * nrhs * sizeof(float), hipMemcpyDeviceToDevice, s));
    return NP_OK;
}

}  // extern "C"
