// Dense LU factorization with partial pivoting and what sits on it: det, inverse, solve, lu (DESIGN.md "LU").
//
// getrf works in place on a COLUMN-MAJOR n x n matrix with LAPACK's semantics (sgetrf): pivot = the first row with the
// largest |value| in the column (isamax), pivots 0-based int32 on the device, info = 1 + the first exactly-zero pivot
// (the factorization goes on past it and never divides by it, like sgetf2).  A row-major buffer handed to it is
// factored as its transpose, which is how the reference's LAPACK calls see it.
//
//   n <= kSmallN  one workgroup loads the whole matrix into LDS, factors it there and, for det / inverse / solve,
//                 finishes the job in the same launch (lu_small_kernel).
//   otherwise     blocked right-looking, panel width kNB.  Per panel: panel_kernel (one workgroup; the panel is
//                 factored in leaves of W columns held in registers), swap_trsm_kernel (the panel's row exchanges on
//                 every other column, U12 = L11^-1 A12 on the columns right of it) and the trailing update
//                 A22 -= L21 U12 on the MFMA GEMM (np::sgemm_sub_ld).  No grid-wide barrier, no float atomics: every
//                 sum has one fixed order, so the same call gives the same bits every time.
// getrs (A X = B with A = P^T L U): the pivots become one permutation, B is gathered through it, then blocked
// triangular solves — a kNB x kNB diagonal block per launch, the rest of the right-hand sides updated on the GEMM.
//
// The Cholesky factorization is np_cholesky.hip, the Jacobi SVD and symmetric eigensolver np_jacobi.hip; what they share with this
// file (kNB, the LDS budget of the one-workgroup paths, blocks_for, read_info) is np_linalg_common.h.
#include <limits.h>

#include "np_linalg_common.h"

namespace {

using namespace np::linalg;

constexpr int kSmallN = 128;             // n <= kSmallN: everything in one workgroup's LDS
constexpr size_t kPermLds = 16384;       // ipiv -> permutation in LDS up to this n (64 KiB), in global memory above

// ---- the isamax rule across a workgroup: larger |value| wins, the lower row wins a tie; NaN never wins ----
__device__ __forceinline__ void amax_combine(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// every thread gets the winning row (INT_MAX when no thread had a candidate that compares: all NaN).  sv / si hold one
// entry per wave; the caller keeps a barrier between two calls.
__device__ __forceinline__ int block_amax(float v, int i, float *sv, int *si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        amax_combine(v, i, ov, oi);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[wave] = v;
        si[wave] = i;
    }
    __syncthreads();
    float bv = sv[0];
    int bi = si[0];
    for (int w = 1; w < nw; ++w) amax_combine(bv, bi, sv[w], si[w]);
    return bi;
}

// ---- small n: the whole matrix in LDS ----
struct SmallArgs {
    const float *a;
    size_t ars, acs;          // the factored matrix M(r, c) = a[r * ars + c * acs]
    int n;
    float *lu;                // optional: M's factors, column-major
    int *ipiv;                // optional: pivots (0-based)
    int *info;                // optional
    float *det;               // optional: det(M), one float on the device
    const float *b;           // right-hand sides B(r, c) = b[r * brs + c * bcs]; null = the identity
    size_t brs, bcs;
    float *x;                 // optional: X(r, c) = x[r * xrs + c * xcs] with M X = B (skipped when info > 0)
    size_t xrs, xcs;
    int nrhs;
    int cw;                   // right-hand sides per pass through LDS
};

__global__ __launch_bounds__(1024) void lu_small_kernel(SmallArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int s_info;
    const int n = p.n, tid = threadIdx.x, nt = blockDim.x;
    float *S = lds;                         // n x n, column-major
    int *piv = (int *)(lds + (size_t)n * n);
    int *perm = piv + n;
    float *X = (float *)(perm + n);         // n x cw, column-major
    for (int e = tid; e < n * n; e += nt) {
        const int r = e % n, c = e / n;
        S[e] = p.a[(size_t)r * p.ars + (size_t)c * p.acs];
    }
    if (tid == 0) s_info = 0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        float best = -1.0f;
        int bi = INT_MAX;
        for (int r = j + tid; r < n; r += nt) {
            const float v = fabsf(S[j * n + r]);
            if (v > best) {
                best = v;
                bi = r;
            }
        }
        int pr = block_amax(best, bi, sv, si);
        if (pr == INT_MAX) pr = j;
        if (pr != j)
            for (int c = tid; c < n; c += nt) {
                const float t = S[c * n + j];
                S[c * n + j] = S[c * n + pr];
                S[c * n + pr] = t;
            }
        if (tid == 0) piv[j] = pr;
        __syncthreads();
        const float d = S[j * n + j];
        if (d != 0.0f) {
            for (int r = j + 1 + tid; r < n; r += nt) S[j * n + r] = S[j * n + r] / d;
        } else if (tid == 0 && s_info == 0) {
            s_info = j + 1;
        }
        __syncthreads();
        const int m = n - j - 1;
        for (int e = tid; e < m * m; e += nt) {
            const int r = j + 1 + e % m, c = j + 1 + e / m;
            S[c * n + r] -= S[j * n + r] * S[c * n + j];
        }
        __syncthreads();
    }
    const int info = s_info;
    if (p.lu)
        for (int e = tid; e < n * n; e += nt) p.lu[e] = S[e];
    if (p.ipiv)
        for (int j = tid; j < n; j += nt) p.ipiv[j] = piv[j];
    if (tid == 0) {
        if (p.info) *p.info = info;
        if (p.det) {
            // the reference's loop (linalg.c:286-297) on our U: the diagonal in index order, left to right in fp32
            float det = 1.0f;
            int swaps = 0;
            for (int j = 0; j < n; ++j) {
                det *= S[j * n + j];
                swaps += piv[j] != j;
            }
            if (swaps & 1) det = -det;
            *p.det = info > 0 ? 0.0f : det;
        }
        for (int r = 0; r < n; ++r) perm[r] = r;
        for (int j = 0; j < n; ++j) {
            const int t = perm[j];
            perm[j] = perm[piv[j]];
            perm[piv[j]] = t;
        }
    }
    if (!p.x || info > 0) return;
    __syncthreads();
    for (int c0 = 0; c0 < p.nrhs; c0 += p.cw) {
        const int w = min(p.cw, p.nrhs - c0);
        for (int e = tid; e < n * w; e += nt) {
            const int r = e % n, c = e / n, src = perm[r];
            X[e] = p.b ? p.b[(size_t)src * p.brs + (size_t)(c0 + c) * p.bcs] : (src == c0 + c ? 1.0f : 0.0f);
        }
        __syncthreads();
        for (int j = 0; j + 1 < n; ++j) {   // unit lower
            const int m = n - j - 1;
            for (int e = tid; e < m * w; e += nt) {
                const int r = j + 1 + e % m, c = e / m;
                X[c * n + r] -= S[j * n + r] * X[c * n + j];
            }
            __syncthreads();
        }
        for (int j = n - 1; j >= 0; --j) {   // upper
            for (int c = tid; c < w; c += nt) X[c * n + j] = X[c * n + j] / S[j * n + j];
            __syncthreads();
            for (int e = tid; e < j * w; e += nt) {
                const int r = e % j, c = e / j;
                X[c * n + r] -= S[j * n + r] * X[c * n + j];
            }
            __syncthreads();
        }
        for (int e = tid; e < n * w; e += nt) {
            const int r = e % n, c = e / n;
            p.x[(size_t)r * p.xrs + (size_t)(c0 + c) * p.xcs] = X[e];
        }
        __syncthreads();
    }
}

// ---- blocked factorization ----

// Factors columns [k0, k0 + nb) of the column-major A (rows k0 .. n-1) with ONE workgroup of 1024 threads: leaves of W
// columns, thread t holding rows t, t + 1024, ... (R of them) of the leaf in registers.  After each leaf, its exchanges
// are applied to the panel's other columns, U of the columns right of it is solved and those columns get the rank-W
// update.  ipiv[k0 .. k0+nb) = absolute pivot rows; *info is set if it was 0 and a zero pivot turned up.
template <int R, int W>
__global__ __launch_bounds__(1024) void panel_kernel(float *A, size_t n, size_t k0, int nb, int *ipiv, int *info) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float rowP[W], rowJ[W];
    __shared__ float Lkk[W * W];
    __shared__ float Ublk[W * kNB];
    __shared__ int s_piv[W];
    __shared__ int s_info;
    const int tid = threadIdx.x;
    if (tid == 0) s_info = 0;
    for (int kk = 0; kk < nb; kk += W) {
        const int w = min(W, nb - kk);
        const size_t rs = k0 + kk;            // first row and column of the leaf
        const size_t m = n - rs;              // rows of the leaf
        float v[R][W];
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const size_t r = (size_t)tid + (size_t)s * 1024;
#pragma unroll
            for (int j = 0; j < W; ++j) v[s][j] = (r < m && j < w) ? A[(rs + j) * n + rs + r] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (j < w) {
                float best = -1.0f;
                int bi = INT_MAX;
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    const size_t r = (size_t)tid + (size_t)s * 1024;
                    if (r >= (size_t)j && r < m) {
                        const float a = fabsf(v[s][j]);
                        if (a > best) {
                            best = a;
                            bi = (int)r;
                        }
                    }
                }
                int pr = block_amax(best, bi, sv, si);
                if (pr == INT_MAX) pr = j;
                const int pt = pr & 1023, ps = pr >> 10;
                if (tid == pt) {
#pragma unroll
                    for (int s = 0; s < R; ++s)
                        if (s == ps)
#pragma unroll
                            for (int jj = 0; jj < W; ++jj) rowP[jj] = v[s][jj];
                }
                if (tid == j) {
#pragma unroll
                    for (int jj = 0; jj < W; ++jj) rowJ[jj] = v[0][jj];
                }
                __syncthreads();
                if (pr != j) {
                    if (tid == j) {
#pragma unroll
                        for (int jj = 0; jj < W; ++jj) v[0][jj] = rowP[jj];
                    }
                    if (tid == pt) {
#pragma unroll
                        for (int s = 0; s < R; ++s)
                            if (s == ps)
#pragma unroll
                                for (int jj = 0; jj < W; ++jj) v[s][jj] = rowJ[jj];
                    }
                }
                if (tid == 0) s_piv[j] = pr;
                const float d = rowP[j];
                if (d == 0.0f && tid == 0 && s_info == 0) s_info = (int)(rs + j + 1);
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    const size_t r = (size_t)tid + (size_t)s * 1024;
                    if (r > (size_t)j && r < m) {
                        if (d != 0.0f) v[s][j] = v[s][j] / d;
#pragma unroll
                        for (int jj = j + 1; jj < W; ++jj) v[s][jj] -= v[s][j] * rowP[jj];
                    }
                }
                __syncthreads();   // rowP / rowJ / sv are written again for the next column
            }
        }
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const size_t r = (size_t)tid + (size_t)s * 1024;
            if (r < m)
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (j < w) A[(rs + j) * n + rs + r] = v[s][j];
        }
        if (tid < w) {
            ipiv[rs + tid] = (int)(rs + s_piv[tid]);
#pragma unroll
            for (int jj = 0; jj < W; ++jj) Lkk[tid * W + jj] = v[0][jj];
        }
        __syncthreads();
        // the leaf's exchanges on the panel's other columns: [k0, rs) and [rs + w, k0 + nb)
        if (tid < nb - w) {
            const size_t c = tid < kk ? k0 + tid : rs + w + (tid - kk);
            float *col = A + c * n;
            for (int j = 0; j < w; ++j) {
                const size_t pr = rs + s_piv[j];
                if (pr != rs + j) {
                    const float t = col[rs + j];
                    col[rs + j] = col[pr];
                    col[pr] = t;
                }
            }
        }
        __syncthreads();
        const int right = nb - kk - w;   // panel columns right of the leaf
        if (right > 0) {
            if (tid < right) {   // U of rows rs .. rs+w-1: forward substitution with the leaf's unit-lower block, in LDS
                float *col = A + (rs + w + tid) * n + rs;
                float *xs = Ublk + tid;
                for (int i = 0; i < w; ++i) xs[i * kNB] = col[i];
                for (int j = 0; j < w; ++j) {
                    const float xj = xs[j * kNB];
                    for (int i = j + 1; i < w; ++i) xs[i * kNB] -= Lkk[i * W + j] * xj;
                }
                for (int i = 0; i < w; ++i) col[i] = xs[i * kNB];
            }
            __syncthreads();
            for (int c = 0; c < right; ++c) {   // rank-w update of rows rs+w .. n-1
                float *col = A + (rs + w + c) * n + rs;
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    const size_t r = (size_t)tid + (size_t)s * 1024;
                    if (r >= (size_t)w && r < m) {
                        float acc = col[r];
#pragma unroll
                        for (int j = 0; j < W; ++j)
                            if (j < w) acc -= v[s][j] * Ublk[j * kNB + c];
                        col[r] = acc;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0 && s_info != 0 && *info == 0) *info = s_info;
}

// One column's rows k0 .. k0+nb-1, kept in LDS at xs[0], xs[stride], ... (a thread's own column: no barrier), := T^-1 x
// with T the nb x nb diagonal block in LDS (T[j * kNB + i] = element (i, j)): unit lower or non-unit upper.  (Held in
// registers with fully unrolled loops, the 64 x 64 solve had the compiler hoist T into 256 VGPRs and spill 6 KB per lane.)
__device__ __forceinline__ void tri_solve(float *xs, int stride, const float *T, int nb, bool upper) {
    if (!upper) {
        for (int j = 0; j < nb; ++j) {
            const float xj = xs[j * stride];
            for (int i = j + 1; i < nb; ++i) xs[i * stride] -= T[j * kNB + i] * xj;
        }
    } else {
        for (int j = nb - 1; j >= 0; --j) {
            const float xj = xs[j * stride] / T[j * kNB + j];
            xs[j * stride] = xj;
            for (int i = 0; i < j; ++i) xs[i * stride] -= T[j * kNB + i] * xj;
        }
    }
}

// T := the nb x nb block of the column-major LU at (k0, k0) (all threads call it)
__device__ __forceinline__ void load_diag_block(float *T, const float *LU, size_t n, size_t k0, int nb) {
    for (int e = threadIdx.x; e < kNB * kNB; e += blockDim.x) {
        const int i = e % kNB, j = e / kNB;
        T[e] = (i < nb && j < nb) ? LU[(k0 + j) * n + k0 + i] : 0.0f;
    }
}

constexpr int kTriThreads = 128;   // columns per workgroup of the two kernels below (T 16 KiB + the columns 32 KiB of LDS)

// After panel k0: the panel's exchanges on every column outside it, then U12 = L11^-1 A12 on the columns right of it.
// One thread per column.
__global__ __launch_bounds__(kTriThreads) void swap_trsm_kernel(float *A, size_t n, size_t k0, int nb, const int *ipiv) {
    __shared__ float T[kNB * kNB];
    __shared__ float Xs[kNB * kTriThreads];
    __shared__ int pv[kNB];
    load_diag_block(T, A, n, k0, nb);
    if (threadIdx.x < (unsigned)nb) pv[threadIdx.x] = ipiv[k0 + threadIdx.x];
    __syncthreads();
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n - nb) return;
    const size_t c = q < k0 ? q : q + nb;
    float *col = A + c * n;
    for (int i = 0; i < nb; ++i) {
        const size_t pr = (size_t)pv[i];
        if (pr != k0 + i) {
            const float t = col[k0 + i];
            col[k0 + i] = col[pr];
            col[pr] = t;
        }
    }
    if (c < k0) return;
    float *xs = Xs + threadIdx.x;
    for (int i = 0; i < nb; ++i) xs[i * kTriThreads] = col[k0 + i];
    tri_solve(xs, kTriThreads, T, nb, false);
    for (int i = 0; i < nb; ++i) col[k0 + i] = xs[i * kTriThreads];
}

// One diagonal block of a blocked triangular solve: rows k0 .. k0+nb-1 of every column of X (column-major, ldx).
__global__ __launch_bounds__(kTriThreads) void tri_block_kernel(const float *LU, size_t n, size_t k0, int nb, float *X,
                                                                size_t ldx, size_t nrhs, int upper) {
    __shared__ float T[kNB * kNB];
    __shared__ float Xs[kNB * kTriThreads];
    load_diag_block(T, LU, n, k0, nb);
    __syncthreads();
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nrhs) return;
    float *col = X + c * ldx + k0;
    float *xs = Xs + threadIdx.x;
    for (int i = 0; i < nb; ++i) xs[i * kTriThreads] = col[i];
    tri_solve(xs, kTriThreads, T, nb, upper != 0);
    for (int i = 0; i < nb; ++i) col[i] = xs[i * kTriThreads];
}

// perm[r] = the row of the original matrix that the pivots' exchanges bring to row r (LAPACK's laswp order)
__global__ __launch_bounds__(1024) void perm_kernel(const int *ipiv, size_t n, int *perm) {
    extern __shared__ int sp[];
    if (n <= kPermLds) {
        for (size_t r = threadIdx.x; r < n; r += blockDim.x) sp[r] = (int)r;
        __syncthreads();
        if (threadIdx.x == 0)
            for (size_t j = 0; j < n; ++j) {
                const int pj = ipiv[j], t = sp[j];
                sp[j] = sp[pj];
                sp[pj] = t;
            }
        __syncthreads();
        for (size_t r = threadIdx.x; r < n; r += blockDim.x) perm[r] = sp[r];
    } else {
        for (size_t r = threadIdx.x; r < n; r += blockDim.x) perm[r] = (int)r;
        __syncthreads();
        if (threadIdx.x == 0)
            for (size_t j = 0; j < n; ++j) {
                const int pj = ipiv[j], t = perm[j];
                perm[j] = perm[pj];
                perm[pj] = t;
            }
    }
}

// X(r, c) = B(perm[r], c), X column-major (ldx); B(r, c) = src[r * srs + c * scs], or the identity when src is null
__global__ __launch_bounds__(256) void gather_kernel(const float *src, size_t srs, size_t scs, const int *perm, size_t n,
                                                     size_t nrhs, float *X, size_t ldx) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t pr = (size_t)perm[r];
    for (size_t c = blockIdx.y; c < nrhs; c += gridDim.y)
        X[c * ldx + r] = src ? src[pr * srs + c * scs] : (pr == c ? 1.0f : 0.0f);
}

// det of the factored matrix: the diagonal in index order, left to right in fp32 (one lane), the pivot parity, 0 if info > 0
__global__ __launch_bounds__(1024) void det_kernel(const float *LU, size_t n, const int *ipiv, const int *info, float *out) {
    __shared__ float dg[1024];
    __shared__ int sw[1024];
    float det = 1.0f;
    int swaps = 0;
    for (size_t base = 0; base < n; base += 1024) {
        const size_t j = base + threadIdx.x;
        if (j < n) {
            dg[threadIdx.x] = LU[j * n + j];
            sw[threadIdx.x] = (size_t)ipiv[j] != j;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const size_t cnt = n - base < 1024 ? n - base : 1024;
            for (size_t k = 0; k < cnt; ++k) {
                det *= dg[k];
                swaps += sw[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (swaps & 1) det = -det;
        *out = *info > 0 ? 0.0f : det;
    }
}

// P, L, U (row-major n x n) from the column-major factors of M and perm: P M = L U
__global__ __launch_bounds__(256) void unpack_kernel(const float *LU, const int *perm, size_t n, float *P, float *L, float *U) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (size_t r = blockIdx.y; r < n; r += gridDim.y) {
        const float v = LU[c * n + r];
        const size_t e = r * n + c;
        L[e] = r > c ? v : (r == c ? 1.0f : 0.0f);
        U[e] = r <= c ? v : 0.0f;
        P[e] = (size_t)perm[r] == c ? 1.0f : 0.0f;
    }
}

// ---- host side ----

int launch_small(const SmallArgs &p0) {
    SmallArgs p = p0;
    const int n = p.n;
    const int fixed = n * n + 2 * n;
    p.cw = 0;
    if (p.x) {
        p.cw = (kSmallLdsFloats - fixed) / n;
        if (p.cw > p.nrhs) p.cw = p.nrhs;
        if (p.cw < 1) return np::fail(NP_ERR_INVALID, "lu: n = %d does not fit the LDS path", n);
    }
    const size_t lds = (size_t)(fixed + n * p.cw) * 4;
    if (lds > 64 * 1024)
        NP_HIP_CHECK(hipFuncSetAttribute((const void *)lu_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kSmallLdsBytes));
    lu_small_kernel<<<1, 1024, lds, np::stream()>>>(p);
    NP_LAUNCH_CHECK("lu_small_kernel");
    return NP_OK;
}

template <int R>
int launch_panel(float *A, size_t n, size_t k0, int nb, int *ipiv, int *info) {
    constexpr int W = R <= 4 ? 16 : 64 / R;
    panel_kernel<R, W><<<1, 1024, 0, np::stream()>>>(A, n, k0, nb, ipiv, info);
    NP_LAUNCH_CHECK("panel_kernel");
    return NP_OK;
}

int panel(float *A, size_t n, size_t k0, int nb, int *ipiv, int *info) {
    const size_t rows = (n - k0 + 1023) / 1024;
    if (rows <= 1) return launch_panel<1>(A, n, k0, nb, ipiv, info);
    if (rows <= 2) return launch_panel<2>(A, n, k0, nb, ipiv, info);
    if (rows <= 4) return launch_panel<4>(A, n, k0, nb, ipiv, info);
    if (rows <= 8) return launch_panel<8>(A, n, k0, nb, ipiv, info);
    if (rows <= 16) return launch_panel<16>(A, n, k0, nb, ipiv, info);
    if (rows <= 32) return launch_panel<32>(A, n, k0, nb, ipiv, info);
    return launch_panel<64>(A, n, k0, nb, ipiv, info);
}

// blocked getrf of the column-major A (n > kSmallN or a caller that wants the blocked path); info is zeroed first
int getrf_blocked(float *A, size_t n, int *ipiv, int *info) {
    if (n > kMaxBlockedN) return np::fail(NP_ERR_INVALID, "getrf: n = %zu is larger than %zu", n, kMaxBlockedN);
    hipStream_t s = np::stream();
    NP_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
    for (size_t k0 = 0; k0 < n; k0 += kNB) {
        const int nb = (int)(n - k0 < (size_t)kNB ? n - k0 : kNB);
        int rc = panel(A, n, k0, nb, ipiv, info);
        if (rc != NP_OK) return rc;
        if (n > (size_t)nb) {
            swap_trsm_kernel<<<blocks_for(n - nb, kTriThreads), kTriThreads, 0, s>>>(A, n, k0, nb, ipiv);
            NP_LAUNCH_CHECK("swap_trsm_kernel");
        }
        const size_t t = n - k0 - nb;   // trailing extent
        if (t > 0) {
            // column-major A22 -= L21 U12 is the row-major product C' -= U12' L21' on the same pointers, ld n
            rc = np::sgemm_sub_ld(t, t, (size_t)nb, A + k0 + (k0 + nb) * n, n, A + (k0 + nb) + k0 * n, n,
                                  A + (k0 + nb) + (k0 + nb) * n, n);
            if (rc != NP_OK) return rc;
        }
    }
    return NP_OK;
}

int getrf_any(float *A, size_t n, int *ipiv, int *info) {
    if (n <= (size_t)kSmallN) {
        SmallArgs p = {};
        p.a = A;
        p.ars = 1;
        p.acs = n;
        p.n = (int)n;
        p.lu = A;
        p.ipiv = ipiv;
        p.info = info;
        return launch_small(p);
    }
    return getrf_blocked(A, n, ipiv, info);
}

int make_perm(const int *ipiv, size_t n, int *perm) {
    const size_t lds = n <= kPermLds ? n * sizeof(int) : 0;
    perm_kernel<<<1, 1024, lds, np::stream()>>>(ipiv, n, perm);
    NP_LAUNCH_CHECK("perm_kernel");
    return NP_OK;
}

int gather(const float *src, size_t srs, size_t scs, const int *perm, size_t n, size_t nrhs, float *X, size_t ldx) {
    const dim3 grid(blocks_for(n, 256), (unsigned)(nrhs < 65535 ? nrhs : 65535));
    gather_kernel<<<grid, 256, 0, np::stream()>>>(src, srs, scs, perm, n, nrhs, X, ldx);
    NP_LAUNCH_CHECK("gather_kernel");
    return NP_OK;
}

// X := U^-1 L^-1 X for the already permuted right-hand sides X (column-major n x nrhs, ldx)
int solve_factored(const float *LU, size_t n, size_t nrhs, float *X, size_t ldx) {
    hipStream_t s = np::stream();
    const unsigned g = blocks_for(nrhs, kTriThreads);
    for (size_t k0 = 0; k0 < n; k0 += kNB) {
        const int nb = (int)(n - k0 < (size_t)kNB ? n - k0 : kNB);
        tri_block_kernel<<<g, kTriThreads, 0, s>>>(LU, n, k0, nb, X, ldx, nrhs, 0);
        NP_LAUNCH_CHECK("tri_block_kernel");
        if (k0 + nb < n) {
            const int rc = np::sgemm_sub_ld(nrhs, n - k0 - nb, (size_t)nb, X + k0, ldx, LU + k0 * n + k0 + nb, n, X + k0 + nb, ldx);
            if (rc != NP_OK) return rc;
        }
    }
    const size_t last = (n - 1) / kNB * kNB;
    for (size_t k0 = last;; k0 -= kNB) {
        const int nb = (int)(n - k0 < (size_t)kNB ? n - k0 : kNB);
        tri_block_kernel<<<g, kTriThreads, 0, s>>>(LU, n, k0, nb, X, ldx, nrhs, 1);
        NP_LAUNCH_CHECK("tri_block_kernel");
        if (k0 == 0) break;
        const int rc = np::sgemm_sub_ld(nrhs, k0, (size_t)nb, X + k0, ldx, LU + k0 * n, n, X, ldx);
        if (rc != NP_OK) return rc;
    }
    return NP_OK;
}

}  // namespace

extern "C" {

int np_getrf(float *a, size_t n, int *ipiv, int *info) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !ipiv || !info) return np::fail(NP_ERR_INVALID, "np_getrf: null pointer");
    if (n == 0) {
        NP_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), np::stream()));
        return NP_OK;
    }
    return getrf_any(a, n, ipiv, info);
}

int np_getrs(const float *lu, const int *ipiv, size_t n, size_t nrhs, float *b) {
    if (int rc = np::ensure_init()) return rc;
    if (!lu || !ipiv || !b) return np::fail(NP_ERR_INVALID, "np_getrs: null pointer");
    if (n == 0 || nrhs == 0) return NP_OK;
    np::Scratch perm, copy;
    if (int rc = perm.alloc(n * sizeof(int))) return rc;
    if (int rc = copy.alloc(n * nrhs * sizeof(float))) return rc;
    if (int rc = np::device_copy(copy.ptr, b, n * nrhs * sizeof(float))) return rc;
    if (int rc = make_perm(ipiv, n, (int *)perm.ptr)) return rc;
    if (int rc = gather((const float *)copy.ptr, 1, n, (const int *)perm.ptr, n, nrhs, b, n)) return rc;
    return solve_factored(lu, n, nrhs, b, n);
}

int np_det(const float *a, size_t n, float *out_dev) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !out_dev) return np::fail(NP_ERR_INVALID, "np_det: null pointer");
    if (n == 0) return np_fill(out_dev, 1.0f, 1);
    if (n <= (size_t)kSmallN) {   // det(a) = det(a^T): the buffer as LAPACK sees it
        SmallArgs p = {};
        p.a = a;
        p.ars = 1;
        p.acs = n;
        p.n = (int)n;
        p.det = out_dev;
        return launch_small(p);
    }
    np::Scratch lu, piv, info;
    if (int rc = lu.alloc(n * n * sizeof(float))) return rc;
    if (int rc = piv.alloc(n * sizeof(int))) return rc;
    if (int rc = info.alloc(sizeof(int))) return rc;
    if (int rc = np::device_copy(lu.ptr, a, n * n * sizeof(float))) return rc;
    if (int rc = getrf_blocked((float *)lu.ptr, n, (int *)piv.ptr, (int *)info.ptr)) return rc;
    det_kernel<<<1, 1024, 0, np::stream()>>>((const float *)lu.ptr, n, (const int *)piv.ptr, (const int *)info.ptr, out_dev);
    NP_LAUNCH_CHECK("det_kernel");
    return NP_OK;
}

int np_inverse(const float *a, size_t n, float *out, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !out || !info_host) return np::fail(NP_ERR_INVALID, "np_inverse: null pointer");
    *info_host = 0;
    if (n == 0) return NP_OK;
    np::Scratch info;
    if (int rc = info.alloc(sizeof(int))) return rc;
    if (n <= (size_t)kSmallN) {
        // the buffer as-is, column-major: M = a^T; M X = I gives (a^T)^-1 column-major = a^-1 row-major
        SmallArgs p = {};
        p.a = a;
        p.ars = 1;
        p.acs = n;
        p.n = (int)n;
        p.info = (int *)info.ptr;
        p.x = out;
        p.xrs = 1;
        p.xcs = n;
        p.nrhs = (int)n;
        if (int rc = launch_small(p)) return rc;
        return read_info((const int *)info.ptr, info_host);
    }
    np::Scratch lu, piv, perm;
    if (int rc = lu.alloc(n * n * sizeof(float))) return rc;
    if (int rc = piv.alloc(n * sizeof(int))) return rc;
    if (int rc = perm.alloc(n * sizeof(int))) return rc;
    if (int rc = np::device_copy(lu.ptr, a, n * n * sizeof(float))) return rc;
    if (int rc = getrf_blocked((float *)lu.ptr, n, (int *)piv.ptr, (int *)info.ptr)) return rc;
    if (int rc = read_info((const int *)info.ptr, info_host)) return rc;
    if (*info_host > 0) return NP_OK;
    if (int rc = make_perm((const int *)piv.ptr, n, (int *)perm.ptr)) return rc;
    if (int rc = gather(nullptr, 0, 0, (const int *)perm.ptr, n, n, out, n)) return rc;
    return solve_factored((const float *)lu.ptr, n, n, out, n);
}

int np_solve(const float *a, const float *b, size_t n, size_t nrhs, float *x, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !b || !x || !info_host) return np::fail(NP_ERR_INVALID, "np_solve: null pointer");
    *info_host = 0;
    if (n == 0 || nrhs == 0) return NP_OK;
    if (nrhs > 0x7fffffffu) return np::fail(NP_ERR_INVALID, "np_solve: too many right-hand sides");
    np::Scratch info;
    if (int rc = info.alloc(sizeof(int))) return rc;
    if (n <= (size_t)kSmallN) {   // M = a itself (row-major reads), B and X row-major n x nrhs
        SmallArgs p = {};
        p.a = a;
        p.ars = n;
        p.acs = 1;
        p.n = (int)n;
        p.info = (int *)info.ptr;
        p.b = b;
        p.brs = nrhs;
        p.bcs = 1;
        p.x = x;
        p.xrs = nrhs;
        p.xcs = 1;
        p.nrhs = (int)nrhs;
        if (int rc = launch_small(p)) return rc;
        return read_info((const int *)info.ptr, info_host);
    }
    np::Scratch lu, piv, perm, xs;
    if (int rc = lu.alloc(n * n * sizeof(float))) return rc;
    if (int rc = piv.alloc(n * sizeof(int))) return rc;
    if (int rc = perm.alloc(n * sizeof(int))) return rc;
    if (int rc = np_transpose2d(a, (float *)lu.ptr, 1, n, n)) return rc;   // column-major a
    if (int rc = getrf_blocked((float *)lu.ptr, n, (int *)piv.ptr, (int *)info.ptr)) return rc;
    if (int rc = read_info((const int *)info.ptr, info_host)) return rc;
    if (*info_host > 0) return NP_OK;
    if (int rc = make_perm((const int *)piv.ptr, n, (int *)perm.ptr)) return rc;
    float *X = x;   // one right-hand side: column-major is row-major
    if (nrhs > 1) {
        if (int rc = xs.alloc(n * nrhs * sizeof(float))) return rc;
        X = (float *)xs.ptr;
    }
    if (int rc = gather(b, nrhs, 1, (const int *)perm.ptr, n, nrhs, X, n)) return rc;
    if (int rc = solve_factored((const float *)lu.ptr, n, nrhs, X, n)) return rc;
    if (nrhs > 1) return np_transpose2d(X, x, 1, nrhs, n);
    return NP_OK;
}

int np_lu(const float *a, size_t n, float *p, float *l, float *u) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !p || !l || !u) return np::fail(NP_ERR_INVALID, "np_lu: null pointer");
    if (n == 0) return NP_OK;
    np::Scratch lu, piv, perm, info;
    if (int rc = lu.alloc(n * n * sizeof(float))) return rc;
    if (int rc = piv.alloc(n * sizeof(int))) return rc;
    if (int rc = perm.alloc(n * sizeof(int))) return rc;
    if (int rc = info.alloc(sizeof(int))) return rc;
    if (n <= (size_t)kSmallN) {   // M = a (row-major reads): partial pivoting on the rows of a
        SmallArgs sp = {};
        sp.a = a;
        sp.ars = n;
        sp.acs = 1;
        sp.n = (int)n;
        sp.lu = (float *)lu.ptr;
        sp.ipiv = (int *)piv.ptr;
        sp.info = (int *)info.ptr;
        if (int rc = launch_small(sp)) return rc;
    } else {
        if (int rc = np_transpose2d(a, (float *)lu.ptr, 1, n, n)) return rc;
        if (int rc = getrf_blocked((float *)lu.ptr, n, (int *)piv.ptr, (int *)info.ptr)) return rc;
    }
    if (int rc = make_perm((const int *)piv.ptr, n, (int *)perm.ptr)) return rc;
    const dim3 grid(blocks_for(n, 256), (unsigned)(n < 4096 ? n : 4096));
    unpack_kernel<<<grid, 256, 0, np::stream()>>>((const float *)lu.ptr, (const int *)perm.ptr, n, p, l, u);
    NP_LAUNCH_CHECK("unpack_kernel");
    return NP_OK;
}

}  // extern "C"
