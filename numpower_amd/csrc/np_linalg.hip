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
// Cholesky (potrf / cholesky; DESIGN.md "Cholesky") is further down: row-major, lower triangle, no pivoting, its own kernels.
// So is the SVD (svd / svdvals; DESIGN.md "SVD"): blocked one-sided Jacobi, its own kernels, nothing shared with the LU.
#include <limits.h>

#include "np_internal.h"

namespace {

constexpr int kNB = 64;                  // panel width of the blocked factorization and of the blocked solves
constexpr int kSmallN = 128;             // n <= kSmallN: everything in one workgroup's LDS
constexpr int kSmallLdsBytes = 156 * 1024;
constexpr int kSmallLdsFloats = kSmallLdsBytes / 4;
constexpr size_t kPermLds = 16384;       // ipiv -> permutation in LDS up to this n (64 KiB), in global memory above
constexpr size_t kMaxBlockedN = 65536;   // panel_kernel holds at most 64 rows per thread

inline unsigned blocks_for(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

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

// ---- Cholesky: a = L L^T on the ROW-MAJOR lower triangle ----
//
//   n <= kNB    one launch of chol_diag_kernel: the matrix is one diagonal block.
//   otherwise   right-looking with panel width kNB on a work matrix W whose strict upper triangle is scratch (np_potrf: a
//               pool copy of a's lower triangle, written back at the end; np_cholesky: the result array, whose upper
//               triangle is zeroed at the end).  Per panel: chol_diag_kernel (one wave: L11), chol_trsm_kernel
//               (L21 = A21 L11^-T, a row per lane, which also writes L21^T into pool scratch) and A22 -= L21 (L21^T) on
//               np::sgemm_sub_ld, one launch per strip of columns (at most four a panel) from the strip's diagonal
//               downwards.  The tiles that cross the diagonal leave garbage above it: in W, never in the caller's.
// No pivot search, no atomics; *info is written by one lane per panel and the stream orders the panels.

// Columns per trailing-update launch: a quarter of the trailing extent, at least kCholStripMin.  A 128 x 128 tile with k = 64
// is bound by its own memory latency, and a launch that does not fill the device still lasts as long as one tile: strips of a
// fixed 512 columns spent 29 of 38 ms at n = 8192 in half-empty launches.
constexpr size_t kCholStripMin = 1024;
constexpr int kCholPad = kNB + 1;    // row stride of a staged block: a lane per row and a lane per column both hit 64 banks

// One wave factors an nb x nb block.  Lane i holds row i in v (v[k] = a_ik for k <= i < nb, else 0) and ends with row i of
// L there; Lt (LDS, kNB * kNB) receives L^T: Lt[j * kNB + i] = l_ij.  Returns 1 + the first column whose pivot is not
// greater than zero (NaN included), else 0; the factorization goes on past it (what follows is unspecified, never a fault).
__device__ __forceinline__ int chol_block(float (&v)[kNB], int nb, float *Lt) {
    const int lane = threadIdx.x;
    int fail = 0;
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
        if (j < nb) {
            const float p = __shfl(v[j], j, 64);   // a_jj - sum_k l_jk^2
            if (!(p > 0.0f) && fail == 0) fail = j + 1;
            const float d = __fsqrt_rn(p);
            const float l = lane > j ? __fdiv_rn(v[j], d) : (lane == j ? d : 0.0f);
            v[j] = l;
            Lt[j * kNB + lane] = l;
            __syncthreads();
#pragma unroll
            for (int k = j + 1; k < kNB; ++k) v[k] -= l * Lt[j * kNB + k];
        }
    }
    return fail;
}

// The nb x nb diagonal block at (k0, k0): reads the lower triangle of src's block, writes L into the lower triangle of
// dst's (src == dst in the blocked path; both row-major with row stride ld).  zero_upper: the block's strict upper triangle
// of dst := +0.0f (the whole matrix is this block).  info_first: *info is this block's word; otherwise it is set only if it
// was still 0 (the first failing panel wins).  lt_out (optional, kNB * kNB floats): L^T for chol_trsm_kernel.
__global__ __launch_bounds__(kNB) void chol_diag_kernel(const float *src, float *dst, size_t ld, size_t k0, int nb,
                                                        int zero_upper, int *info, int info_first, float *lt_out) {
    __shared__ float St[kNB * kCholPad];
    __shared__ float Lt[kNB * kNB];
    const int lane = threadIdx.x;
    const float *in = src + k0 * ld + k0;
    // every load is issued, a masked-out lane reading the block's first element: no branch, 16 loads in flight
#pragma unroll 16
    for (int r = 0; r < kNB; ++r) {
        const bool low = r < nb && lane <= r;
        const float t = in[low ? (size_t)r * ld + lane : 0];
        St[r * kCholPad + lane] = low ? t : 0.0f;
    }
    __syncthreads();
    float v[kNB];
#pragma unroll
    for (int k = 0; k < kNB; ++k) v[k] = St[lane * kCholPad + k];
    const int fail = chol_block(v, nb, Lt);
#pragma unroll
    for (int k = 0; k < kNB; ++k) St[lane * kCholPad + k] = v[k];
    __syncthreads();
    if (lt_out && nb == kNB)
        for (int j = 0; j < kNB; ++j) lt_out[j * kNB + lane] = Lt[j * kNB + lane];
    float *out = dst + k0 * ld + k0;
    for (int r = 0; r < nb; ++r) {
        if (lane <= r)
            out[(size_t)r * ld + lane] = St[r * kCholPad + lane];
        else if (zero_upper && lane < nb)
            out[(size_t)r * ld + lane] = 0.0f;
    }
    if (lane == 0) {
        if (info_first)
            *info = fail;
        else if (fail != 0 && *info == 0)
            *info = (int)k0 + fail;
    }
}

// L21 = A21 L11^-T for the rows below the diagonal block at (k0, k0) (a full kNB-wide panel): row r of A21 is a row vector
// x with y L11^T = x, solved by substitution, a row per lane, against L11^T in LDS (Lt11: what chol_diag_kernel
// left, column j of L11 contiguous and read by every lane at once).  L21 overwrites A21 and its transpose goes to Lt21
// (kNB x (n - k0 - kNB), row stride ldt): the second operand of the trailing update, which reads none transposed.
__global__ __launch_bounds__(kNB) void chol_trsm_kernel(float *W, size_t n, size_t k0, const float *Lt11, float *Lt21, size_t ldt) {
    __shared__ float Tt[kNB * kNB];        // Tt[j * kNB + i] = l_ij of L11
    __shared__ float X[kNB * kCholPad];    // this workgroup's kNB rows of the panel
    const int lane = threadIdx.x;
#pragma unroll 16
    for (int r = 0; r < kNB; ++r) Tt[r * kNB + lane] = Lt11[r * kNB + lane];
    const size_t first = k0 + kNB + (size_t)blockIdx.x * kNB;   // first row of this workgroup
    float *rows = W + first * n + k0;
    const int cnt = (int)(n - first < (size_t)kNB ? n - first : kNB);
#pragma unroll 16
    for (int r = 0; r < kNB; ++r)   // rows past the matrix re-read its last one: their lanes compute and store nothing
        X[r * kCholPad + lane] = rows[(size_t)(r < cnt ? r : cnt - 1) * n + lane];
    __syncthreads();
    // The row stays in LDS (a lane's own row: no barrier) and the loops stay loops.  Held in registers with the loops
    // unrolled, the compiler put off the updates, kept what it had read of L11 instead and spilled 6 KB a lane.
    float *x = X + lane * kCholPad;
    for (int j = 0; j < kNB; ++j) {
        const float yj = __fdiv_rn(x[j], Tt[j * kNB + j]);
        x[j] = yj;
#pragma unroll 8
        for (int i = j + 1; i < kNB; ++i) x[i] -= yj * Tt[j * kNB + i];
    }
    if (lane < cnt) {
        float *lt = Lt21 + (first - k0 - kNB) + lane;
#pragma unroll 8
        for (int j = 0; j < kNB; ++j) lt[(size_t)j * ldt] = x[j];
    }
    __syncthreads();
    for (int r = 0; r < cnt; ++r) rows[(size_t)r * n + lane] = X[r * kCholPad + lane];
}

// The lower triangle (diagonal included) of dst := that of src (skipped when src == dst); zero_upper: the strict upper
// triangle of dst := +0.0f.  Both n x n row-major.
__global__ __launch_bounds__(256) void chol_tri_kernel(const float *src, float *dst, size_t n, int zero_upper) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (size_t r = blockIdx.y; r < n; r += gridDim.y) {
        if (c <= r) {
            if (src != dst) dst[r * n + c] = src[r * n + c];
        } else if (zero_upper) {
            dst[r * n + c] = 0.0f;
        }
    }
}

// ---- SVD: one-sided (Hestenes) Jacobi, blocked over pairs of 32-row blocks ----
//
// The work matrix W holds one "column of a" per row (W = a^T for m >= n, a itself for m < n: the transposed problem), padded
// with zero rows to a multiple of 64 and zero columns to a multiple of 32; Vt starts as I.  A sweep is a round-robin tournament
// over the 32-row blocks.  Per step and block pair (rows P, 64 x L):
//   svd_gram_kernel   G = P P^T on v_mfma_f32_32x32x2_f32, a wave per 32 x 32 quadrant, the row length cut into up to 16
//                     workgroups whose partial Grams are stored one by one
//   svd_eig_kernel    folds the partials in index order, counts the row pairs above the tolerance and, if there are any,
//                     diagonalises G by two-sided cyclic Jacobi in LDS — G, the rotations and their product M in fp64, M rounded
//                     to fp32 once at the end
//   svd_apply_kernel  P <- M P and the same for the 64 rows of Vt, on the MFMA, a wave per 32 columns, in place (a wave
//                     reads all 64 rows of its columns before it stores one); pairs without a rotation are skipped
// Up to 64 rows whose length fits LDS take svd_small_kernel instead: one launch, one workgroup (further down).
// A zero row never rotates, so the padding stays what it is.  The only cross-workgroup sums are integer counters and an integer
// max of float bit patterns: order-independent, so every call gives the same bits.
constexpr int kSvdB = 32;                // rows of a block
constexpr int kSvdP = 2 * kSvdB;         // rows of a block pair
constexpr int kSvdStr = kSvdP + 1;       // row stride of a 64 x 64 matrix in LDS
constexpr int kSvdMaxSplit = 16;         // partial Grams per pair at most
constexpr int kSvdSweepCap = 60;         // 26 sweeps at 4096 x 4096: the count grows with n
constexpr int kSvdInnerCap = 10;         // sweeps of the 64 x 64 eigenproblem at most (any orthogonal M is a valid step)
constexpr double kSvdTol = 4.0 * 1.1920928955078125e-7;
constexpr size_t kSvdMaxDim = 65536;
int g_svd_max_sweeps = 0;                // np_debug_svd_max_sweeps
int g_svd_last_sweeps = 0;               // np_debug_svd_last_sweeps
int g_svd_small_off = 0;                 // np_debug_svd_small_path(0): every shape takes the blocked path (A/B, tests)

typedef float svd_v16f __attribute__((ext_vector_type(16)));

struct SvdCtl {
    unsigned long long above;        // row pairs found above the tolerance by any workgroup of the sweep (0 = converged)
    unsigned long long above_once;   // the same with every row pair counted once (k (k - 1) / 2 at most: 2^31 at k = 65536)
    unsigned maxbits;                // bit pattern of the largest squared row norm at the start of the sweep
    int pad;
};

// block pair j of tournament step `step` over nblk (even) blocks: position 0 stays, the others go round
__device__ __forceinline__ void svd_pair(int nblk, int step, int j, int &p, int &q) {
    const int r = nblk - 1;
    const int a = j == 0 ? 0 : 1 + (j - 1 + step) % r;
    const int b = 1 + (nblk - 2 - j + step) % r;
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// global row of local row k (0 .. 63) of the block pair (p, q)
__device__ __forceinline__ size_t svd_row(int p, int q, int k) {
    return k < kSvdB ? (size_t)p * kSvdB + k : (size_t)q * kSvdB + (k - kSvdB);
}

// a, b squared norms, g the dot product; lim: both norms at or under it = a negligible pair
__device__ __forceinline__ bool svd_active(double a, double b, double g, double lim) {
    return a > 0.0 && b > 0.0 && !(a <= lim && b <= lim) && fabs(g) > kSvdTol * sqrt(a * b);
}

// squared norm of every row (a wave per row, one fixed order) and the largest of them into ctl->maxbits
__global__ __launch_bounds__(256) void svd_rownorm_kernel(const float *W, size_t ld, size_t nrows, float *normsq, SvdCtl *ctl) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= nrows) return;
    const float *w = W + row * ld;
    float acc = 0.0f;
    for (size_t c = lane; c < ld; c += 64) acc = fmaf(w[c], w[c], acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) {
        normsq[row] = acc;
        atomicMax(&ctl->maxbits, __float_as_uint(acc));   // non-negative floats order as their bits (a NaN ends on top)
    }
}

__global__ __launch_bounds__(256) void svd_gram_kernel(const float *W, size_t ld, int nblk, int step, int tiles_per_split,
                                                       int ntiles, int nsplit, float *Gpart) {
    __shared__ float T[kSvdP * 33];
    int p, q;
    svd_pair(nblk, step, blockIdx.x, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bi = wave >> 1, bj = wave & 1, i = lane & 31, kq = lane >> 5;
    svd_v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int t0 = blockIdx.y * tiles_per_split;
    const int t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
    const int col = tid & 31, r0 = tid >> 5;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = r0 + 8 * u;
            T[row * 33 + col] = W[svd_row(p, q, row) * ld + (size_t)t * 32 + col];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 32; kk += 2) {
            const float a = T[(bi * 32 + i) * 33 + kk + kq];
            const float b = T[(bj * 32 + i) * 33 + kk + kq];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float *out = Gpart + ((size_t)blockIdx.x * nsplit + blockIdx.y) * (kSvdP * kSvdP);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kq;
        out[row * kSvdP + bj * 32 + i] = acc[r];
    }
}

// dynamic LDS: G and M, kSvdP x kSvdStr doubles each
__global__ __launch_bounds__(256) void svd_eig_kernel(const float *Gpart, int nsplit, int step, float thr, SvdCtl *ctl,
                                                      float *Mbuf, int *flag) {
    extern __shared__ double svd_sm[];
    double *G = svd_sm, *M = svd_sm + kSvdP * kSvdStr;
    __shared__ double cs_c[32], cs_s[32];
    __shared__ int cs_p[32], cs_q[32];
    __shared__ int s_cnt[2];
    __shared__ int s_rot;
    const int tid = threadIdx.x, pair = blockIdx.x;
    const float *gp = Gpart + (size_t)pair * nsplit * (kSvdP * kSvdP);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) {
        float acc = gp[idx];   // (folding in fp64 instead was tried: no fewer sweeps)
        for (int s = 1; s < nsplit; ++s) acc += gp[(size_t)s * (kSvdP * kSvdP) + idx];
        const int r = idx >> 6, c = idx & 63;
        G[r * kSvdStr + c] = (double)acc;
        M[r * kSvdStr + c] = r == c ? 1.0 : 0.0;
    }
    if (tid < 2) s_cnt[tid] = 0;
    if (tid == 0) s_rot = 0;
    __syncthreads();
    const double maxsq = (double)__uint_as_float(ctl->maxbits);
    const double lim = (double)thr * (double)thr * maxsq;
    int all = 0, once = 0;
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < j && svd_active(G[i * kSvdStr + i], G[j * kSvdStr + j], G[i * kSvdStr + j], lim)) {
            ++all;
            if (step == 0 || ((i < kSvdB) != (j < kSvdB))) ++once;   // rows of one block meet again in every step
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        all += __shfl_down(all, off, 64);
        once += __shfl_down(once, off, 64);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt[0], all);
        atomicAdd(&s_cnt[1], once);
    }
    __syncthreads();
    if (s_cnt[0] == 0) {   // uniform: nothing to rotate, M = I, the apply kernel skips the pair
        if (tid == 0) flag[pair] = 0;
        return;
    }
    if (tid == 0) {
        atomicAdd(&ctl->above, (unsigned long long)s_cnt[0]);
        atomicAdd(&ctl->above_once, (unsigned long long)s_cnt[1]);
    }
    int p = 0, q = 0;
    bool mine = false;
    for (int isw = 0; isw < kSvdInnerCap; ++isw) {
        for (int st = 0; st < kSvdP - 1; ++st) {
            if (tid < 32) {
                svd_pair(kSvdP, st, tid, p, q);
                const double gpp = G[p * kSvdStr + p], gqq = G[q * kSvdStr + q], gpq = G[p * kSvdStr + q];
                double c = 1.0, s = 0.0;
                mine = svd_active(gpp, gqq, gpq, lim);
                if (mine) {
                    const double z = (gqq - gpp) / (2.0 * gpq);
                    const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = c * t;
                    s_rot = 1;
                }
                cs_c[tid] = c;
                cs_s[tid] = s;
                cs_p[tid] = p;
                cs_q[tid] = q;
            }
            __syncthreads();
            {   // rows p, q of G and of M
                const int col = tid & 63;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int pr = (tid >> 6) + 4 * u;
                    const double c = cs_c[pr], s = cs_s[pr];
                    if (s != 0.0) {
                        const int rp = cs_p[pr] * kSvdStr + col, rq = cs_q[pr] * kSvdStr + col;
                        const double gp_ = G[rp], gq_ = G[rq], mp_ = M[rp], mq_ = M[rq];
                        G[rp] = c * gp_ - s * gq_;
                        G[rq] = s * gp_ + c * gq_;
                        M[rp] = c * mp_ - s * mq_;
                        M[rq] = s * mp_ + c * mq_;
                    }
                }
            }
            __syncthreads();
            {   // columns p, q of G
                const int row = tid & 63;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int pr = (tid >> 6) + 4 * u;
                    const double c = cs_c[pr], s = cs_s[pr];
                    if (s != 0.0) {
                        const int cp = row * kSvdStr + cs_p[pr], cq = row * kSvdStr + cs_q[pr];
                        const double gp_ = G[cp], gq_ = G[cq];
                        G[cp] = c * gp_ - s * gq_;
                        G[cq] = s * gp_ + c * gq_;
                    }
                }
            }
            __syncthreads();
            if (tid < 32 && mine) {
                G[p * kSvdStr + q] = 0.0;
                G[q * kSvdStr + p] = 0.0;
            }
        }
        __syncthreads();
        const int rot = s_rot;
        __syncthreads();
        if (tid == 0) s_rot = 0;
        __syncthreads();
        if (!rot) break;
    }
    float *out = Mbuf + (size_t)pair * (kSvdP * kSvdP);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) out[idx] = (float)M[(idx >> 6) * kSvdStr + (idx & 63)];
    if (tid == 0) flag[pair] = 1;
}

// X <- M X for the block pair's 64 rows of W (chunks 0 .. wchunks - 1 of 128 columns) and of V (the chunks after them)
__global__ __launch_bounds__(256) void svd_apply_kernel(float *W, size_t ldw, int wchunks, float *V, size_t ldv, int nblk,
                                                        int step, const float *Mbuf, const int *flag) {
    __shared__ float Ms[kSvdP * kSvdStr];
    const int pair = blockIdx.x;
    if (!flag[pair]) return;
    int p, q;
    svd_pair(nblk, step, pair, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *Mg = Mbuf + (size_t)pair * (kSvdP * kSvdP);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) Ms[(idx >> 6) * kSvdStr + (idx & 63)] = Mg[idx];
    __syncthreads();
    const bool onw = (int)blockIdx.y < wchunks;
    float *X = onw ? W : V;
    const size_t ld = onw ? ldw : ldv;
    const size_t col0 = (size_t)(onw ? blockIdx.y : blockIdx.y - wchunks) * 128 + (size_t)wave * 32;
    if (col0 >= ld) return;   // ld is a multiple of 32: a wave's 32 columns are all there or none is
    const int i = lane & 31, kq = lane >> 5;
    float b[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) b[kk] = X[svd_row(p, q, 2 * kk + kq) * ld + col0 + i];
    svd_v16f acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ms[i * kSvdStr + 2 * kk + kq], b[kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ms[(32 + i) * kSvdStr + 2 * kk + kq], b[kk], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = (r & 3) + 8 * (r >> 2) + 4 * kq;
        X[((size_t)p * kSvdB + lr) * ld + col0 + i] = acc0[r];
        X[((size_t)q * kSvdB + lr) * ld + col0 + i] = acc1[r];
    }
}

// ---- small path: k <= 64 rows whose length fits LDS — the whole decomposition in ONE launch of one workgroup ----
// W (k rows of L floats, row stride Ls, odd) and Vt (k x k, row stride Vs, odd) live in LDS.  Unblocked one-sided Jacobi: a
// round-robin tournament over the rows (padded to an even count; the dummy never plays), k / 2 disjoint pairs per step, a
// half-wave per pair: three dot products in fp32 (lane-strided fmaf chains, then a butterfly: every lane holds the same bits), the
// rotation in fp64 from them, rounded once, applied to both rows of W and of Vt by the half-wave's lanes.  One barrier per step.  The
// tail — norms, stable descending ranks, __fsqrt_rn / __fdiv_rn, +0.0f for a zero norm — is the blocked path's, in the same launch.
struct SvdSmallArgs {
    const float *a;
    int k, L, Ls, Vs;    // rows (min(m, n)), their length (max(m, n)), LDS row strides of W and Vt
    int wide;            // m < n: the rows of a are the rows of W; else W = a^T
    int vectors;
    int cap;
    float thr;           // max(m, n) eps
    float *u, *s, *vt;
    int *out2;           // out2[0] = info, out2[1] = sweeps taken
};

__device__ __forceinline__ float svd_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the same within each half of the wave (the offsets stay below 32: no lane reads the other half, whatever that half is doing)
__device__ __forceinline__ float svd_half_sum(float v) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(1024) void svd_small_kernel(SvdSmallArgs p) {
    extern __shared__ float svd_small_sm[];
    const int k = p.k, L = p.L, Ls = p.Ls, Vs = p.Vs;
    float *W = svd_small_sm, *V = W + (size_t)k * Ls, *nsq = V + (size_t)k * Vs;
    int *rank = (int *)(nsq + k);
    __shared__ int s_cnt;
    __shared__ unsigned s_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int hl = lane & 31, half = lane >> 5;
    const int ke = k + (k & 1);
    for (int idx = tid; idx < k * L; idx += blockDim.x) {
        if (p.wide) {
            W[(idx / L) * Ls + idx % L] = p.a[idx];
        } else {   // a is L x k: element (r, i) goes to row i
            W[(idx % k) * Ls + idx / k] = p.a[idx];
        }
    }
    if (p.vectors)
        for (int idx = tid; idx < k * k; idx += blockDim.x) V[(idx / k) * Vs + idx % k] = idx / k == idx % k ? 1.0f : 0.0f;
    if (tid == 0) {
        s_cnt = 0;
        s_max = 0u;
    }
    __syncthreads();
    int sweeps = 0, above = 0;
    for (int sweep = 0; sweep < p.cap; ++sweep) {
        for (int i = wave; i < k; i += nw) {   // the largest squared norm at the start of the sweep: the negligible-pair rule
            const float *w = W + i * Ls;
            float acc = 0.0f;
            for (int c = lane; c < L; c += 64) acc = fmaf(w[c], w[c], acc);
            acc = svd_wave_sum(acc);
            if (lane == 0) atomicMax(&s_max, __float_as_uint(acc));
        }
        __syncthreads();
        const double lim = (double)p.thr * (double)p.thr * (double)__uint_as_float(s_max);
        for (int st = 0; st < ke - 1; ++st) {
            for (int pj = 2 * wave + half; pj < ke / 2; pj += 2 * nw) {   // a half-wave per pair: 32 pairs at once
                int rp, rq;
                svd_pair(ke, st, pj, rp, rq);
                if (rq >= k) continue;   // the dummy of an odd k
                float *wp = W + rp * Ls, *wq = W + rq * Ls;
                float sa = 0.0f, sb = 0.0f, sg = 0.0f;
                for (int c = hl; c < L; c += 32) {
                    const float x = wp[c], y = wq[c];
                    sa = fmaf(x, x, sa);
                    sb = fmaf(y, y, sb);
                    sg = fmaf(x, y, sg);
                }
                sa = svd_half_sum(sa);
                sb = svd_half_sum(sb);
                sg = svd_half_sum(sg);
                if (!svd_active((double)sa, (double)sb, (double)sg, lim)) continue;   // uniform in the half-wave
                const double z = ((double)sb - (double)sa) / (2.0 * (double)sg);
                const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
                const double cd = 1.0 / sqrt(1.0 + t * t);
                const float cf = (float)cd, sf = (float)(cd * t);
                if (hl == 0) atomicAdd(&s_cnt, 1);
                for (int c = hl; c < L; c += 32) {
                    const float x = wp[c], y = wq[c];
                    wp[c] = cf * x - sf * y;
                    wq[c] = sf * x + cf * y;
                }
                if (p.vectors) {
                    float *vp = V + rp * Vs, *vq = V + rq * Vs;
                    for (int c = hl; c < k; c += 32) {
                        const float x = vp[c], y = vq[c];
                        vp[c] = cf * x - sf * y;
                        vq[c] = sf * x + cf * y;
                    }
                }
            }
            __syncthreads();
        }
        above = s_cnt;
        sweeps = sweep + 1;
        __syncthreads();
        if (tid == 0) {
            s_cnt = 0;
            s_max = 0u;
        }
        __syncthreads();
        if (above == 0) break;   // uniform: every thread read the same count
    }
    for (int i = wave; i < k; i += nw) {
        const float *w = W + i * Ls;
        float acc = 0.0f;
        for (int c = lane; c < L; c += 64) acc = fmaf(w[c], w[c], acc);
        acc = svd_wave_sum(acc);
        if (lane == 0) nsq[i] = acc;
    }
    __syncthreads();
    if (tid < k) {   // the order of svd_rank_kernel
        const float vi = nsq[tid];
        const bool ni = vi != vi;
        int r = 0;
        for (int j = 0; j < k; ++j) {
            const float vj = nsq[j];
            const bool nj = vj != vj;
            const bool greater = (nj && !ni) || vj > vi, equal = (nj && ni) || vj == vi;
            r += (greater || (equal && j < tid)) ? 1 : 0;
        }
        rank[tid] = r;
        p.s[r] = __fsqrt_rn(vi);
    }
    if (tid == 0) {
        p.out2[0] = above;   // 0 when converged; at the cap: the pairs rotated in the last sweep, each met once
        p.out2[1] = sweeps;
    }
    if (!p.vectors) return;
    __syncthreads();
    for (int idx = tid; idx < k * L; idx += blockDim.x) {   // the normalised rows of W: vt (k x L) when wide, else u (L x k)
        const int i = p.wide ? idx / L : idx % k, c = p.wide ? idx % L : idx / k;
        const float sv = __fsqrt_rn(nsq[i]);
        const float v = sv == 0.0f ? 0.0f : __fdiv_rn(W[i * Ls + c], sv);
        if (p.wide) p.vt[(size_t)rank[i] * L + c] = v;
        else p.u[(size_t)c * k + rank[i]] = v;
    }
    for (int idx = tid; idx < k * k; idx += blockDim.x) {   // the rows of Vt: u (k x k) transposed when wide, else vt
        const int i = p.wide ? idx % k : idx / k, c = p.wide ? idx / k : idx % k;
        const float v = V[i * Vs + c];
        if (p.wide) p.u[(size_t)c * k + rank[i]] = v;
        else p.vt[(size_t)rank[i] * k + c] = v;
    }
}

// rank[i] = position of row i in descending order of its norm (stable: the lower row first among equals); s[rank[i]] = the norm
__global__ __launch_bounds__(256) void svd_rank_kernel(const float *normsq, size_t n, float *s, int *rank) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float vi = normsq[i];
    const bool ni = vi != vi;
    int r = 0;
    for (size_t j = 0; j < n; ++j) {   // a NaN counts as larger than every number and equal to a NaN: the ranks are a permutation
        const float vj = normsq[j];
        const bool nj = vj != vj;
        const bool greater = (nj && !ni) || vj > vi, equal = (nj && ni) || vj == vi;
        r += (greater || (equal && j < i)) ? 1 : 0;
    }
    rank[i] = r;
    s[r] = __fsqrt_rn(vi);
}

// dst[rank[i]][c] = src[i][c] for c < ncols, divided by the row's norm when normsq is given (+0.0f when that norm is 0)
__global__ __launch_bounds__(256) void svd_gather_kernel(const float *src, size_t ld, size_t ncols, size_t n, const int *rank,
                                                         const float *normsq, float *dst) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    for (size_t i = blockIdx.y; i < n; i += gridDim.y) {
        float v = src[i * ld + c];
        if (normsq) {
            const float sv = __fsqrt_rn(normsq[i]);
            v = sv == 0.0f ? 0.0f : __fdiv_rn(v, sv);
        }
        dst[(size_t)rank[i] * ncols + c] = v;
    }
}

// ---- symmetric eigensolver (np_eigh, np_eigvalsh) ----
// Two-sided (classical) Jacobi, blocked over pairs of 32-row blocks with the SVD's tournament.  W is the symmetric matrix built
// from the lower triangle of a, padded with zeros to a multiple of 64 (a zero row and column never rotates); Vt starts as I and
// holds the eigenvectors as ROWS while iterating, so one row operation serves W and Vt.  Per step and block pair (I, J):
//   eigh_eig_kernel       reads the 64 x 64 pivot block W[IJ, IJ] (its lower triangle) straight from W, counts the pairs above the
//                         tolerance and, if there are any, diagonalises it in LDS in fp64: M (fp32, rounded once) and the diagonal D
//   svd_apply_kernel      W[IJ, :] <- M W[IJ, :] and Vt[IJ, :] <- M Vt[IJ, :], all pairs (disjoint rows)
//   eigh_colapply_kernel  W[:, IJ] <- W[:, IJ] M^T, all pairs (disjoint columns), in a launch of its own: a row half and a column
//                         half of two pairs overlap.  The pivot block is written as diag(D) with exact zeros off it.
// A pair (p, q) rotates when |w_pq| > kEighTol * scale, scale = the largest |entry| of the lower triangle of a, fixed at the start
// of the call: diagonals may be zero or negative, so the SVD's sqrt(g_pp g_qq) has no meaning here.
// n <= 64 takes eigh_small_kernel: the same 64 x 64 LDS solve on the whole (padded) matrix, sort, signs and output in ONE launch.
constexpr int kEighSweepCap = 60;
constexpr double kEighTol = 1.1920928955078125e-7;   // eps: relative to the largest entry, not to the pair's diagonals
int g_eigh_max_sweeps = 0;                           // np_debug_eigh_max_sweeps
int g_eigh_last_sweeps = 0;                          // np_debug_eigh_last_sweeps
int g_eigh_small_off = 0;                            // np_debug_eigh_small_path(0)

struct EighCtl {
    unsigned long long above;        // pairs found above the tolerance by any workgroup of the sweep (0 = converged)
    unsigned long long above_once;   // the same with every pair counted once
    unsigned scalebits;              // bit pattern of the largest |entry| of the lower triangle (a NaN ends on top)
    int pad;
};

__device__ __forceinline__ bool eigh_active(double g, double lim) { return fabs(g) > lim; }

// W (npad x npad) from the lower triangle of a (n x n), zeros beyond n; the largest |entry| into ctl->scalebits
__global__ __launch_bounds__(256) void eigh_pack_kernel(const float *a, size_t n, float *W, size_t npad, EighCtl *ctl) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned top = 0u;
    if (c < npad) {
        for (size_t r = blockIdx.y; r < npad; r += gridDim.y) {
            float v = 0.0f;
            if (r < n && c < n) v = r >= c ? a[r * n + c] : a[c * n + r];
            W[r * npad + c] = v;
            const unsigned b = __float_as_uint(v) & 0x7fffffffu;
            top = b > top ? b : top;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_down((int)top, off, 64);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0 && top != 0u) atomicMax(&ctl->scalebits, top);   // an integer max: order-independent
}

// Cyclic two-sided Jacobi on the symmetric G (fp64, LDS, row stride kSvdStr, 64 x 64 of which the leading k x k is the problem and
// the rest zero) by 256 threads: the round-robin over its k rows (padded to an even count; the dummy never plays), up to 32 disjoint
// rotations per step, rotations accumulated as rows of M when M is given.  At most `cap` sweeps; a sweep without a rotation ends
// it.  Returns the sweeps taken (that last one included); *rot_last = the rotations of the last sweep.
__device__ int eigh_solve64(double *G, double *M, int k, double lim, int cap, int *rot_last) {
    __shared__ double cs_c[32], cs_s[32];
    __shared__ int cs_p[32], cs_q[32];
    __shared__ int s_rot;
    const int tid = threadIdx.x;
    if (tid == 0) s_rot = 0;
    __syncthreads();
    const int ke = k + (k & 1);
    int p = 0, q = 0, sweeps = 0, rot = 0;
    bool mine = false;
    for (int isw = 0; isw < cap; ++isw) {
        for (int st = 0; st < ke - 1; ++st) {
            if (tid < 32) {
                double c = 1.0, s = 0.0, gpp = 0.0, gqq = 0.0, gpq = 0.0;
                mine = false;
                p = q = 0;
                if (tid < ke / 2) {
                    svd_pair(ke, st, tid, p, q);
                    if (q < k) {   // else the dummy of an odd k
                        gpp = G[p * kSvdStr + p];
                        gqq = G[q * kSvdStr + q];
                        gpq = G[p * kSvdStr + q];
                        mine = eigh_active(gpq, lim);
                    }
                }
                if (mine) {
                    const double z = (gqq - gpp) / (2.0 * gpq);
                    const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = c * t;
                    atomicAdd(&s_rot, 1);
                }
                cs_c[tid] = c;
                cs_s[tid] = s;
                cs_p[tid] = p;
                cs_q[tid] = q;
            }
            __syncthreads();
            {   // rows p, q of G and of M
                const int col = tid & 63;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int pr = (tid >> 6) + 4 * u;
                    const double c = cs_c[pr], s = cs_s[pr];
                    if (s != 0.0) {
                        const int rp = cs_p[pr] * kSvdStr + col, rq = cs_q[pr] * kSvdStr + col;
                        const double gp_ = G[rp], gq_ = G[rq];
                        G[rp] = c * gp_ - s * gq_;
                        G[rq] = s * gp_ + c * gq_;
                        if (M) {
                            const double mp_ = M[rp], mq_ = M[rq];
                            M[rp] = c * mp_ - s * mq_;
                            M[rq] = s * mp_ + c * mq_;
                        }
                    }
                }
            }
            __syncthreads();
            {   // columns p, q of G
                const int row = tid & 63;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int pr = (tid >> 6) + 4 * u;
                    const double c = cs_c[pr], s = cs_s[pr];
                    if (s != 0.0) {
                        const int cp = row * kSvdStr + cs_p[pr], cq = row * kSvdStr + cs_q[pr];
                        const double gp_ = G[cp], gq_ = G[cq];
                        G[cp] = c * gp_ - s * gq_;
                        G[cq] = s * gp_ + c * gq_;
                    }
                }
            }
            __syncthreads();
            if (tid < 32 && mine) {
                G[p * kSvdStr + q] = 0.0;
                G[q * kSvdStr + p] = 0.0;
            }
        }
        __syncthreads();
        rot = s_rot;
        sweeps = isw + 1;
        __syncthreads();
        if (tid == 0) s_rot = 0;
        __syncthreads();
        if (rot == 0) break;   // uniform: every thread read the same count
    }
    *rot_last = rot;
    return sweeps;
}

// dynamic LDS: G and M, kSvdP x kSvdStr doubles each
__global__ __launch_bounds__(256) void eigh_eig_kernel(const float *W, size_t ld, int nblk, int step, EighCtl *ctl, float *Mbuf,
                                                       float *Dbuf, int *flag) {
    extern __shared__ double eigh_sm[];
    double *G = eigh_sm, *M = eigh_sm + kSvdP * kSvdStr;
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, pair = blockIdx.x;
    int p, q;
    svd_pair(nblk, step, pair, p, q);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) {
        const int r = idx >> 6, c = idx & 63;   // p < q: the block's lower triangle is a part of W's
        const int hi = r > c ? r : c, lo = r > c ? c : r;
        G[r * kSvdStr + c] = (double)W[svd_row(p, q, hi) * ld + svd_row(p, q, lo)];
        M[r * kSvdStr + c] = r == c ? 1.0 : 0.0;
    }
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const double lim = kEighTol * (double)__uint_as_float(ctl->scalebits);
    int all = 0, once = 0;
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < j && eigh_active(G[i * kSvdStr + j], lim)) {
            ++all;
            if (step == 0 || ((i < kSvdB) != (j < kSvdB))) ++once;   // rows of one block meet again in every step
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        all += __shfl_down(all, off, 64);
        once += __shfl_down(once, off, 64);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_cnt[0], all);
        atomicAdd(&s_cnt[1], once);
    }
    __syncthreads();
    if (s_cnt[0] == 0) {   // uniform: nothing to rotate, both apply kernels skip the pair
        if (tid == 0) flag[pair] = 0;
        return;
    }
    if (tid == 0) {
        atomicAdd(&ctl->above, (unsigned long long)s_cnt[0]);
        atomicAdd(&ctl->above_once, (unsigned long long)s_cnt[1]);
    }
    // the call's own cap: a solve that stopped while still rotating would have its remaining off-diagonal mass zeroed below
    // unseen.  Should it ever happen (it takes an input that does not converge at all), the sweep is reported as not converged.
    int rot_last;
    eigh_solve64(G, M, kSvdP, lim, kEighSweepCap, &rot_last);
    if (tid == 0 && rot_last != 0) {
        atomicAdd(&ctl->above, (unsigned long long)rot_last);
        atomicAdd(&ctl->above_once, (unsigned long long)rot_last);
    }
    float *out = Mbuf + (size_t)pair * (kSvdP * kSvdP);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) out[idx] = (float)M[(idx >> 6) * kSvdStr + (idx & 63)];
    if (tid < kSvdP) Dbuf[(size_t)pair * kSvdP + tid] = (float)G[tid * kSvdStr + tid];
    if (tid == 0) flag[pair] = 1;
}

// W[:, IJ] <- W[:, IJ] M^T for the block pair's 64 columns: a workgroup per pair and 128 rows, a wave per 32 rows.  The wave
// stages its 32 x 64 tile in LDS with row-contiguous loads (2 x 128 bytes per row), multiplies on the MFMA and stores rows again;
// the tile is read whole before anything is stored, and no other wave of the launch touches it.  The two waves whose rows are
// the pair's own write the pivot block instead: diag(D), exact zeros off it.
__global__ __launch_bounds__(256) void eigh_colapply_kernel(float *W, size_t ld, int nblk, int step, const float *Mbuf,
                                                            const float *Dbuf, const int *flag) {
    __shared__ float Ms[kSvdP * kSvdStr];
    __shared__ float Ts[4][kSvdB * kSvdStr];
    const int pair = blockIdx.x;
    if (!flag[pair]) return;
    int p, q;
    svd_pair(nblk, step, pair, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *Mg = Mbuf + (size_t)pair * (kSvdP * kSvdP);
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) Ms[(idx >> 6) * kSvdStr + (idx & 63)] = Mg[idx];
    const size_t row0 = (size_t)blockIdx.y * 128 + (size_t)wave * 32;
    const bool live = row0 < ld;   // ld is a multiple of 64: a wave's 32 rows are all there or none is
    const int rb = (int)(row0 / kSvdB);
    const bool pivot = rb == p || rb == q;
    const size_t col = lane < kSvdB ? (size_t)p * kSvdB + lane : (size_t)q * kSvdB + (lane - kSvdB);
    float *T = Ts[wave];
    if (live && !pivot) {
#pragma unroll 8
        for (int rr = 0; rr < kSvdB; ++rr) T[rr * kSvdStr + lane] = W[(row0 + rr) * ld + col];
    }
    __syncthreads();
    if (!live) return;
    if (pivot) {
        const int l0 = rb == p ? 0 : kSvdB;   // local index of the wave's first row
        const float d = Dbuf[(size_t)pair * kSvdP + lane];
        for (int rr = 0; rr < kSvdB; ++rr) W[(row0 + rr) * ld + col] = lane == l0 + rr ? d : 0.0f;
        return;
    }
    const int i = lane & 31, kq = lane >> 5;
    svd_v16f acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {   // out[r][j] = sum_k T[r][k] M[j][k]
        const float x = T[i * kSvdStr + 2 * kk + kq];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, Ms[i * kSvdStr + 2 * kk + kq], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, Ms[(32 + i) * kSvdStr + 2 * kk + kq], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = (r & 3) + 8 * (r >> 2) + 4 * kq;
        W[(row0 + lr) * ld + (size_t)p * kSvdB + i] = acc0[r];
        W[(row0 + lr) * ld + (size_t)q * kSvdB + i] = acc1[r];
    }
}

// diag[i] = W[i][i] for i < n, or NaN everywhere when the scale of the call is not finite (non-finite input)
__global__ __launch_bounds__(256) void eigh_diag_kernel(const float *W, size_t ld, size_t n, const EighCtl *ctl, float *diag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool finite = (ctl->scalebits & 0x7f800000u) != 0x7f800000u;
    diag[i] = finite ? W[i * ld + i] : __uint_as_float(0x7fc00000u);
}

// rank[i] = position of diag[i] in ascending order (stable: the lower index first among equals, -0.0f == +0.0f); w[rank[i]] = it
__device__ __forceinline__ int eigh_rank_of(const float *diag, size_t n, size_t i) {
    const float vi = diag[i];
    const bool ni = vi != vi;
    int r = 0;
    for (size_t j = 0; j < n; ++j) {   // a NaN counts as larger than every number and equal to a NaN: the ranks are a permutation
        const float vj = diag[j];
        const bool nj = vj != vj;
        const bool less = (ni && !nj) || vj < vi, equal = (nj && ni) || vj == vi;
        r += (less || (equal && j < i)) ? 1 : 0;
    }
    return r;
}

__global__ __launch_bounds__(256) void eigh_rank_kernel(const float *diag, size_t n, float *w, int *rank) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = eigh_rank_of(diag, n, i);
    rank[i] = r;
    w[r] = diag[i];
}

// the sign rule for `rows` rows of length n (stride ld), a wave per row: neg[row] = 1 when the component of largest magnitude,
// the first such in index order, is negative
__device__ __forceinline__ void eigh_row_sign(const float *v, int n, int lane, int *neg_out) {
    float best = -1.0f, val = 0.0f;   // the winner's magnitude and its signed value travel together: no lane reads another's
    int at = 0x7fffffff;
    for (int c = lane; c < n; c += 64) {
        const float x = v[c], m = fabsf(x);
        if (m > best) {   // strictly: the first index of a lane's own columns stays
            best = m;
            val = x;
            at = c;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64), ov = __shfl_xor(val, off, 64);
        const int oa = __shfl_xor(at, off, 64);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            val = ov;
            at = oa;
        }
    }
    if (lane == 0) *neg_out = val < 0.0f ? 1 : 0;
}

__global__ __launch_bounds__(256) void eigh_sign_kernel(const float *V, size_t ld, size_t n, int *neg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= n) return;
    eigh_row_sign(V + row * ld, (int)n, lane, neg + row);
}

// dst[rank[i]][c] = +-V[i][c] for c < n: the rows of Vt in ascending order of their eigenvalue, the sign rule applied
__global__ __launch_bounds__(256) void eigh_gather_kernel(const float *V, size_t ld, size_t n, const int *rank, const int *neg,
                                                          float *dst) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    for (size_t i = blockIdx.y; i < n; i += gridDim.y) {
        const float x = V[i * ld + c];
        dst[(size_t)rank[i] * n + c] = neg[i] ? -x : x;
    }
}

// any[0] = 1 when some i > j has a[i][j] != a[j][i] (two NaNs count as equal)
__global__ __launch_bounds__(256) void symmetry_kernel(const float *a, size_t n, int *any) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    bool bad = false;
    for (size_t r = (size_t)blockIdx.y; r < n; r += gridDim.y) {
        if (r <= c) continue;
        const float x = a[r * n + c], y = a[c * n + r];
        bad = bad || (x != y && !(x != x && y != y));
    }
    if (bad) atomicOr(any, 1);
}

// ---- small path: n <= 64 — the whole decomposition in ONE launch of one workgroup ----
// W (padded with zeros to 64 x 64) and Vt live in LDS as the G and M of eigh_solve64, in fp64; the sweeps, the ascending stable
// ranks, the sign rule and the transposed output follow in the same launch.
struct EighSmallArgs {
    const float *a;
    int n, vectors, cap;
    float *w, *v;
    int *out2;   // out2[0] = info, out2[1] = sweeps taken
};

__global__ __launch_bounds__(256) void eigh_small_kernel(EighSmallArgs p) {
    extern __shared__ double eigh_small_sm[];
    double *G = eigh_small_sm, *M = p.vectors ? eigh_small_sm + kSvdP * kSvdStr : nullptr;
    __shared__ float s_diag[kSvdP], s_vt[kSvdP * kSvdP];
    __shared__ int s_rank[kSvdP], s_neg[kSvdP];
    __shared__ unsigned s_scale;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = p.n;
    if (tid == 0) s_scale = 0u;
    __syncthreads();
    unsigned top = 0u;
    for (int idx = tid; idx < kSvdP * kSvdP; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        float v = 0.0f;
        if (r < n && c < n) v = r >= c ? p.a[r * n + c] : p.a[c * n + r];
        G[r * kSvdStr + c] = (double)v;
        if (M) M[r * kSvdStr + c] = r == c ? 1.0 : 0.0;
        const unsigned b = __float_as_uint(v) & 0x7fffffffu;
        top = b > top ? b : top;
    }
    atomicMax(&s_scale, top);
    __syncthreads();
    const bool finite = (s_scale & 0x7f800000u) != 0x7f800000u;
    const double lim = kEighTol * (double)__uint_as_float(s_scale);
    int rot_last = 0;
    const int sweeps = eigh_solve64(G, M, n, lim, p.cap, &rot_last);
    if (tid < n) s_diag[tid] = finite ? (float)G[tid * kSvdStr + tid] : __uint_as_float(0x7fc00000u);
    __syncthreads();
    if (tid < n) {
        const int r = eigh_rank_of(s_diag, (size_t)n, (size_t)tid);
        s_rank[tid] = r;
        p.w[r] = s_diag[tid];
    }
    if (tid == 0) {
        p.out2[0] = rot_last;   // 0 when converged; at the cap: the pairs rotated in the last sweep
        p.out2[1] = sweeps;
    }
    if (!p.vectors) return;
    for (int idx = tid; idx < n * kSvdP; idx += 256) s_vt[idx] = (float)M[(idx >> 6) * kSvdStr + (idx & 63)];   // rounded once
    __syncthreads();
    for (int i = wave; i < n; i += 4) eigh_row_sign(s_vt + i * kSvdP, n, lane, &s_neg[i]);   // a wave per row of Vt
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += 256) {
        const int i = idx / n, c = idx % n;
        const float x = s_vt[i * kSvdP + c];
        p.v[(size_t)c * n + s_rank[i]] = s_neg[i] ? -x : x;
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

int read_info(const int *dev_info, int *info_host) {
    int v = 0;
    const int rc = np_memcpy_d2h(&v, dev_info, sizeof(int));
    if (rc != NP_OK) return rc;
    *info_host = v;
    return NP_OK;
}

int chol_tri(const float *src, float *dst, size_t n, int zero_upper) {
    const dim3 grid(blocks_for(n, 256), (unsigned)(n < 4096 ? n : 4096));
    chol_tri_kernel<<<grid, 256, 0, np::stream()>>>(src, dst, n, zero_upper);
    NP_LAUNCH_CHECK("chol_tri_kernel");
    return NP_OK;
}

// blocked potrf of the row-major W (n > kNB): L into its lower triangle, garbage into its strict upper triangle
int potrf_blocked(float *W, size_t n, int *info) {
    hipStream_t s = np::stream();
    const size_t ldt = (n + 3) & ~(size_t)3;
    np::Scratch lt;
    if (int rc = lt.alloc(((size_t)kNB * kNB + (size_t)kNB * ldt) * sizeof(float))) return rc;
    float *Lt11 = (float *)lt.ptr, *Lt21 = Lt11 + kNB * kNB;   // L11^T of the current panel, then L21^T
    NP_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
    for (size_t k0 = 0; k0 < n; k0 += kNB) {
        const int nb = (int)(n - k0 < (size_t)kNB ? n - k0 : kNB);
        chol_diag_kernel<<<1, kNB, 0, s>>>(W, W, n, k0, nb, 0, info, 0, Lt11);
        NP_LAUNCH_CHECK("chol_diag_kernel");
        const size_t t = n - k0 - nb;   // trailing extent (nb == kNB whenever t > 0)
        if (t == 0) break;
        chol_trsm_kernel<<<blocks_for(t, kNB), kNB, 0, s>>>(W, n, k0, Lt11, Lt21, ldt);
        NP_LAUNCH_CHECK("chol_trsm_kernel");
        size_t strip = (t / 4 + 127) & ~(size_t)127;
        if (strip < kCholStripMin) strip = kCholStripMin;
        for (size_t c = 0; c < t; c += strip) {   // block column c of A22, from its diagonal downwards
            const size_t w = t - c < strip ? t - c : strip, c0 = k0 + nb + c;
            if (int rc = np::sgemm_sub_ld(t - c, w, (size_t)kNB, W + c0 * n + k0, n, Lt21 + c, ldt, W + c0 * n + c0, n)) return rc;
        }
    }
    return NP_OK;
}

int svd_gather(const float *src, size_t ld, size_t ncols, size_t n, const int *rank, const float *normsq, float *dst) {
    const dim3 grid(blocks_for(ncols, 256), (unsigned)(n < 4096 ? n : 4096));
    svd_gather_kernel<<<grid, 256, 0, np::stream()>>>(src, ld, ncols, n, rank, normsq, dst);
    NP_LAUNCH_CHECK("svd_gather_kernel");
    return NP_OK;
}

// LDS floats of the small path, or 0 when the shape does not take it.  The same answer for np_svd and np_svdvals (room for Vt is
// counted either way): both must take the same path to give the same s.
size_t svd_small_floats(size_t k, size_t L) {
    if (k > (size_t)kSvdP || g_svd_small_off) return 0;
    const size_t f = k * (L | 1) + k * (k | 1) + 2 * k;
    return f <= (size_t)kSmallLdsFloats ? f : 0;
}

int svd_small(const float *a, size_t k, size_t L, bool wide, float *u, float *s, float *vt, int *info_host) {
    np::Scratch out2;
    if (int rc = out2.alloc(2 * sizeof(int))) return rc;
    SvdSmallArgs p = {};
    p.a = a;
    p.k = (int)k;
    p.L = (int)L;
    p.Ls = (int)(L | 1);
    p.Vs = (int)(k | 1);
    p.wide = wide ? 1 : 0;
    p.vectors = u != nullptr ? 1 : 0;
    p.cap = g_svd_max_sweeps > 0 ? g_svd_max_sweeps : kSvdSweepCap;
    p.thr = (float)L * 1.1920928955078125e-7f;
    p.u = u;
    p.s = s;
    p.vt = vt;
    p.out2 = (int *)out2.ptr;
    const size_t lds = svd_small_floats(k, L) * sizeof(float);
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)svd_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmallLdsBytes));
    svd_small_kernel<<<1, 1024, lds, np::stream()>>>(p);
    NP_LAUNCH_CHECK("svd_small_kernel");
    int host2[2] = {0, 0};
    if (int rc = np_memcpy_d2h(host2, out2.ptr, sizeof(host2))) return rc;
    *info_host = host2[0];
    g_svd_last_sweeps = host2[1];
    return NP_OK;
}

// u, vt null: singular values only (no Vt, no normalisation; W goes through the same rotations, so s has the same bits)
int svd_impl(const char *who, const float *a, size_t m, size_t n, float *u, float *s, float *vt, int *info_host) {
    *info_host = 0;
    if (m == 0 || n == 0) return NP_OK;
    if (m > kSvdMaxDim || n > kSvdMaxDim) return np::fail(NP_ERR_INVALID, "%s: m, n = %zu, %zu: larger than %zu", who, m, n, kSvdMaxDim);
    hipStream_t st = np::stream();
    const bool vectors = u != nullptr;
    const bool wide = m < n;                       // the transposed problem: the rows of a are the "columns"
    const size_t k = wide ? m : n, L = wide ? n : m;
    if (svd_small_floats(k, L) > 0) return svd_small(a, k, L, wide, u, s, vt, info_host);
    const size_t npad = (k + kSvdP - 1) / kSvdP * kSvdP, ldw = (L + 31) & ~(size_t)31;
    const int nblk = (int)(npad / kSvdB), pairs = nblk / 2, steps = nblk - 1;
    const int ntiles = (int)(ldw / 32);
    int nsplit = (512 + pairs - 1) / pairs;
    if (nsplit > kSvdMaxSplit) nsplit = kSvdMaxSplit;
    if (nsplit > ntiles) nsplit = ntiles;
    const int tps = (ntiles + nsplit - 1) / nsplit;
    nsplit = (ntiles + tps - 1) / tps;
    np::Scratch w, v, tmp, gpart, mbuf, flag, ctl, normsq, rank;
    if (int rc = w.alloc(npad * ldw * sizeof(float))) return rc;
    if (vectors)
        if (int rc = v.alloc(npad * npad * sizeof(float))) return rc;
    if (!wide || vectors)   // a^T on its way into W and the factor that leaves through a transpose
        if (int rc = tmp.alloc(k * (wide ? k : L) * sizeof(float))) return rc;
    if (int rc = gpart.alloc((size_t)pairs * nsplit * kSvdP * kSvdP * sizeof(float))) return rc;
    if (int rc = mbuf.alloc((size_t)pairs * kSvdP * kSvdP * sizeof(float))) return rc;
    if (int rc = flag.alloc((size_t)pairs * sizeof(int))) return rc;
    if (int rc = ctl.alloc(sizeof(SvdCtl))) return rc;
    if (int rc = normsq.alloc(npad * sizeof(float))) return rc;
    if (int rc = rank.alloc(npad * sizeof(int))) return rc;
    float *W = (float *)w.ptr, *V = (float *)v.ptr, *T = (float *)tmp.ptr;
    if (int rc = np_memset0(W, npad * ldw * sizeof(float))) return rc;
    if (wide) {
        if (int rc = np_copy2d(W, ldw, a, n, n, m)) return rc;
    } else {
        if (int rc = np_transpose2d(a, T, 1, m, n)) return rc;
        if (int rc = np_copy2d(W, ldw, T, m, m, n)) return rc;
    }
    if (vectors)
        if (int rc = np_identity(V, npad)) return rc;
    constexpr size_t eig_lds = 2 * (size_t)kSvdP * kSvdStr * sizeof(double);
    // every call: the attribute belongs to the current device's copy of the kernel, and setting it costs nothing next to a sweep
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)svd_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)eig_lds));
    const float thr = (float)L * 1.1920928955078125e-7f;   // max(m, n) eps
    const int wchunks = (int)((ldw + 127) / 128), vchunks = vectors ? (int)((npad + 127) / 128) : 0;
    g_svd_last_sweeps = 0;
    const int cap = g_svd_max_sweeps > 0 ? g_svd_max_sweeps : kSvdSweepCap;
    bool converged = false;
    unsigned long long last[2] = {0, 0};
    for (int sweep = 0; sweep < cap && !converged; ++sweep) {
        NP_HIP_CHECK(hipMemsetAsync(ctl.ptr, 0, sizeof(SvdCtl), st));
        svd_rownorm_kernel<<<blocks_for(k, 4), 256, 0, st>>>(W, ldw, k, (float *)normsq.ptr, (SvdCtl *)ctl.ptr);
        NP_LAUNCH_CHECK("svd_rownorm_kernel");
        for (int step = 0; step < steps; ++step) {
            svd_gram_kernel<<<dim3(pairs, nsplit), 256, 0, st>>>(W, ldw, nblk, step, tps, ntiles, nsplit, (float *)gpart.ptr);
            NP_LAUNCH_CHECK("svd_gram_kernel");
            svd_eig_kernel<<<pairs, 256, eig_lds, st>>>((const float *)gpart.ptr, nsplit, step, thr, (SvdCtl *)ctl.ptr,
                                                        (float *)mbuf.ptr, (int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_eig_kernel");
            svd_apply_kernel<<<dim3(pairs, wchunks + vchunks), 256, 0, st>>>(W, ldw, wchunks, V, npad, nblk, step,
                                                                             (const float *)mbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_apply_kernel");
        }
        if (int rc = np_memcpy_d2h(last, ctl.ptr, sizeof(last))) return rc;   // the one host read of the sweep
        converged = last[0] == 0;
        g_svd_last_sweeps = sweep + 1;
    }
    if (!converged) *info_host = last[1] > (unsigned long long)INT_MAX ? INT_MAX : (last[1] > 0 ? (int)last[1] : 1);
    NP_HIP_CHECK(hipMemsetAsync(ctl.ptr, 0, sizeof(SvdCtl), st));
    svd_rownorm_kernel<<<blocks_for(k, 4), 256, 0, st>>>(W, ldw, k, (float *)normsq.ptr, (SvdCtl *)ctl.ptr);
    NP_LAUNCH_CHECK("svd_rownorm_kernel");
    svd_rank_kernel<<<blocks_for(k, 256), 256, 0, st>>>((const float *)normsq.ptr, k, s, (int *)rank.ptr);
    NP_LAUNCH_CHECK("svd_rank_kernel");
    if (vectors) {
        const int *rk = (const int *)rank.ptr;
        const float *nq = (const float *)normsq.ptr;
        if (wide) {   // a = V_B S U_B^T for B = a^T: vt = the normalised rows of W, u = the transposed rows of Vt
            if (int rc = svd_gather(W, ldw, L, k, rk, nq, vt)) return rc;
            if (int rc = svd_gather(V, npad, k, k, rk, nullptr, T)) return rc;
            if (int rc = np_transpose2d(T, u, 1, k, k)) return rc;
        } else {
            if (int rc = svd_gather(V, npad, k, k, rk, nullptr, vt)) return rc;
            if (int rc = svd_gather(W, ldw, L, k, rk, nq, T)) return rc;
            if (int rc = np_transpose2d(T, u, 1, k, L)) return rc;
        }
    }
    return np_sync();   // the scratch goes back to the pool; info is known
}

constexpr size_t kEighLds = 2 * (size_t)kSvdP * kSvdStr * sizeof(double);   // G and M

int eigh_small(const float *a, size_t n, float *w, float *v, int *info_host) {
    np::Scratch out2;
    if (int rc = out2.alloc(2 * sizeof(int))) return rc;
    EighSmallArgs p = {};
    p.a = a;
    p.n = (int)n;
    p.vectors = v != nullptr ? 1 : 0;
    p.cap = g_eigh_max_sweeps > 0 ? g_eigh_max_sweeps : kEighSweepCap;
    p.w = w;
    p.v = v;
    p.out2 = (int *)out2.ptr;
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)eigh_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEighLds));
    eigh_small_kernel<<<1, 256, kEighLds, np::stream()>>>(p);
    NP_LAUNCH_CHECK("eigh_small_kernel");
    int host2[2] = {0, 0};
    if (int rc = np_memcpy_d2h(host2, out2.ptr, sizeof(host2))) return rc;
    *info_host = host2[0];
    g_eigh_last_sweeps = host2[1];
    return NP_OK;
}

// v null: eigenvalues only (no Vt; W goes through the same rotations, so w has the same bits)
int eigh_impl(const char *who, const float *a, size_t n, float *w, float *v, int *info_host) {
    *info_host = 0;
    if (n == 0) return NP_OK;
    if (n > kSvdMaxDim) return np::fail(NP_ERR_INVALID, "%s: n = %zu: larger than %zu", who, n, kSvdMaxDim);
    if (n <= (size_t)kSvdP && !g_eigh_small_off) return eigh_small(a, n, w, v, info_host);
    hipStream_t st = np::stream();
    const bool vectors = v != nullptr;
    const size_t npad = (n + kSvdP - 1) / kSvdP * kSvdP;
    const int nblk = (int)(npad / kSvdB), pairs = nblk / 2, steps = nblk - 1;
    np::Scratch wm, vm, tmp, mbuf, dbuf, flag, ctl, diag, rank, neg;
    if (int rc = wm.alloc(npad * npad * sizeof(float))) return rc;
    if (vectors) {
        if (int rc = vm.alloc(npad * npad * sizeof(float))) return rc;
        if (int rc = tmp.alloc(n * n * sizeof(float))) return rc;   // the sorted rows of Vt on their way through a transpose
        if (int rc = neg.alloc(n * sizeof(int))) return rc;
    }
    if (int rc = mbuf.alloc((size_t)pairs * kSvdP * kSvdP * sizeof(float))) return rc;
    if (int rc = dbuf.alloc((size_t)pairs * kSvdP * sizeof(float))) return rc;
    if (int rc = flag.alloc((size_t)pairs * sizeof(int))) return rc;
    if (int rc = ctl.alloc(sizeof(EighCtl))) return rc;
    if (int rc = diag.alloc(n * sizeof(float))) return rc;
    if (int rc = rank.alloc(n * sizeof(int))) return rc;
    float *W = (float *)wm.ptr, *V = (float *)vm.ptr;
    EighCtl *C = (EighCtl *)ctl.ptr;
    NP_HIP_CHECK(hipMemsetAsync(C, 0, sizeof(EighCtl), st));
    const unsigned rows_y = (unsigned)(npad < 4096 ? npad : 4096);
    eigh_pack_kernel<<<dim3(blocks_for(npad, 256), rows_y), 256, 0, st>>>(a, n, W, npad, C);
    NP_LAUNCH_CHECK("eigh_pack_kernel");
    if (vectors)
        if (int rc = np_identity(V, npad)) return rc;
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)eigh_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEighLds));
    const int chunks = (int)((npad + 127) / 128);
    g_eigh_last_sweeps = 0;
    const int cap = g_eigh_max_sweeps > 0 ? g_eigh_max_sweeps : kEighSweepCap;
    bool converged = false;
    unsigned long long last[2] = {0, 0};
    for (int sweep = 0; sweep < cap && !converged; ++sweep) {
        NP_HIP_CHECK(hipMemsetAsync(C, 0, 2 * sizeof(unsigned long long), st));   // the counters; the scale stays
        for (int step = 0; step < steps; ++step) {
            eigh_eig_kernel<<<pairs, 256, kEighLds, st>>>(W, npad, nblk, step, C, (float *)mbuf.ptr, (float *)dbuf.ptr,
                                                          (int *)flag.ptr);
            NP_LAUNCH_CHECK("eigh_eig_kernel");
            svd_apply_kernel<<<dim3(pairs, chunks + (vectors ? chunks : 0)), 256, 0, st>>>(
                W, npad, chunks, V, npad, nblk, step, (const float *)mbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_apply_kernel");
            eigh_colapply_kernel<<<dim3(pairs, chunks), 256, 0, st>>>(W, npad, nblk, step, (const float *)mbuf.ptr,
                                                                      (const float *)dbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("eigh_colapply_kernel");
        }
        if (int rc = np_memcpy_d2h(last, C, sizeof(last))) return rc;   // the one host read of the sweep
        converged = last[0] == 0;
        g_eigh_last_sweeps = sweep + 1;
    }
    if (!converged) *info_host = last[1] > (unsigned long long)INT_MAX ? INT_MAX : (last[1] > 0 ? (int)last[1] : 1);
    eigh_diag_kernel<<<blocks_for(n, 256), 256, 0, st>>>(W, npad, n, C, (float *)diag.ptr);
    NP_LAUNCH_CHECK("eigh_diag_kernel");
    eigh_rank_kernel<<<blocks_for(n, 256), 256, 0, st>>>((const float *)diag.ptr, n, w, (int *)rank.ptr);
    NP_LAUNCH_CHECK("eigh_rank_kernel");
    if (vectors) {
        eigh_sign_kernel<<<blocks_for(n, 4), 256, 0, st>>>(V, npad, n, (int *)neg.ptr);
        NP_LAUNCH_CHECK("eigh_sign_kernel");
        const dim3 grid(blocks_for(n, 256), (unsigned)(n < 4096 ? n : 4096));
        eigh_gather_kernel<<<grid, 256, 0, st>>>(V, npad, n, (const int *)rank.ptr, (const int *)neg.ptr, (float *)tmp.ptr);
        NP_LAUNCH_CHECK("eigh_gather_kernel");
        if (int rc = np_transpose2d((const float *)tmp.ptr, v, 1, n, n)) return rc;
    }
    return np_sync();   // the scratch goes back to the pool; info is known
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

int np_potrf(float *a, size_t n, int *info) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !info) return np::fail(NP_ERR_INVALID, "np_potrf: null pointer");
    if (n == 0) {
        NP_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), np::stream()));
        return NP_OK;
    }
    if (n <= (size_t)kNB) {
        chol_diag_kernel<<<1, kNB, 0, np::stream()>>>(a, a, n, 0, (int)n, 0, info, 1, nullptr);
        NP_LAUNCH_CHECK("chol_diag_kernel");
        return NP_OK;
    }
    if (n > kMaxBlockedN) return np::fail(NP_ERR_INVALID, "np_potrf: n = %zu is larger than %zu", n, kMaxBlockedN);
    np::Scratch w;   // the trailing updates write above the diagonal: they run on a copy, the caller's upper triangle stays
    if (int rc = w.alloc(n * n * sizeof(float))) return rc;
    if (int rc = chol_tri(a, (float *)w.ptr, n, 0)) return rc;
    if (int rc = potrf_blocked((float *)w.ptr, n, info)) return rc;
    return chol_tri((const float *)w.ptr, a, n, 0);
}

int np_cholesky(const float *a, size_t n, float *out, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !out || !info_host) return np::fail(NP_ERR_INVALID, "np_cholesky: null pointer");
    *info_host = 0;
    if (n == 0) return NP_OK;
    if (n > kMaxBlockedN) return np::fail(NP_ERR_INVALID, "np_cholesky: n = %zu is larger than %zu", n, kMaxBlockedN);
    np::Scratch info;
    if (int rc = info.alloc(sizeof(int))) return rc;
    if (n <= (size_t)kNB) {
        chol_diag_kernel<<<1, kNB, 0, np::stream()>>>(a, out, n, 0, (int)n, 1, (int *)info.ptr, 1, nullptr);
        NP_LAUNCH_CHECK("chol_diag_kernel");
    } else {   // the result array is the work matrix: its upper triangle is scratch until the last launch zeroes it
        if (int rc = chol_tri(a, out, n, 0)) return rc;
        if (int rc = potrf_blocked(out, n, (int *)info.ptr)) return rc;
        if (int rc = chol_tri(out, out, n, 1)) return rc;
    }
    return read_info((const int *)info.ptr, info_host);
}

int np_svd(const float *a, size_t m, size_t n, float *u, float *s, float *vt, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !u || !s || !vt || !info_host) return np::fail(NP_ERR_INVALID, "np_svd: null pointer");
    return svd_impl("np_svd", a, m, n, u, s, vt, info_host);
}

int np_svdvals(const float *a, size_t m, size_t n, float *s, int *info_host) {
    if (int rc = np::ensure_init()) return rc;
    if (!a || !s || !info_host) return np::fail(NP_ERR_INVALID, "np_svdvals: null pointer");
    return svd_impl("np_svdvals", a, m, n, nullptr, s, nullptr, info_host);
}

int np_eigh(const float *a, size_t n, float *w, float *v, int *info_host) {
    if (!a || !w || !v || !info_host) return np::fail(NP_ERR_INVALID, "np_eigh: null pointer");   // before any device work
    if (int rc = np::ensure_init()) return rc;
    return eigh_impl("np_eigh", a, n, w, v, info_host);
}

int np_eigvalsh(const float *a, size_t n, float *w, int *info_host) {
    if (!a || !w || !info_host) return np::fail(NP_ERR_INVALID, "np_eigvalsh: null pointer");   // before any device work
    if (int rc = np::ensure_init()) return rc;
    return eigh_impl("np_eigvalsh", a, n, w, nullptr, info_host);
}

int np_symmetry_mismatch(const float *a, size_t n, int *host_any) {
    if (!a || !host_any) return np::fail(NP_ERR_INVALID, "np_symmetry_mismatch: null pointer");   // before any device work
    if (int rc = np::ensure_init()) return rc;
    *host_any = 0;
    if (n < 2) return NP_OK;
    np::Scratch any;
    if (int rc = any.alloc(sizeof(int))) return rc;
    NP_HIP_CHECK(hipMemsetAsync(any.ptr, 0, sizeof(int), np::stream()));
    const dim3 grid(blocks_for(n, 256), (unsigned)(n < 4096 ? n : 4096));
    symmetry_kernel<<<grid, 256, 0, np::stream()>>>(a, n, (int *)any.ptr);
    NP_LAUNCH_CHECK("symmetry_kernel");
    return read_info((const int *)any.ptr, host_any);
}

int np_debug_eigh_max_sweeps(int sweeps) {
    if (sweeps < 0) return np::fail(NP_ERR_INVALID, "np_debug_eigh_max_sweeps: %d", sweeps);
    g_eigh_max_sweeps = sweeps;
    return NP_OK;
}

int np_debug_eigh_small_path(int on) {
    g_eigh_small_off = on ? 0 : 1;
    return NP_OK;
}

int np_debug_eigh_last_sweeps(int *host_sweeps) {
    if (!host_sweeps) return np::fail(NP_ERR_INVALID, "np_debug_eigh_last_sweeps: null pointer");
    *host_sweeps = g_eigh_last_sweeps;
    return NP_OK;
}

int np_debug_svd_max_sweeps(int sweeps) {
    if (sweeps < 0) return np::fail(NP_ERR_INVALID, "np_debug_svd_max_sweeps: %d", sweeps);
    g_svd_max_sweeps = sweeps;
    return NP_OK;
}

int np_debug_svd_small_path(int on) {
    g_svd_small_off = on ? 0 : 1;
    return NP_OK;
}

int np_debug_svd_last_sweeps(int *host_sweeps) {
    if (!host_sweeps) return np::fail(NP_ERR_INVALID, "np_debug_svd_last_sweeps: null pointer");
    *host_sweeps = g_svd_last_sweeps;
    return NP_OK;
}

}  // extern "C"
