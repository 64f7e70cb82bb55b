// Cholesky factorization a = L L^T on the ROW-MAJOR lower triangle: np_potrf (in place, device info) and np_cholesky (out of
// place, host info).  No pivoting; its trailing update runs on the MFMA GEMM (np::sgemm_sub_ld), like the LU's
// (np_lu.hip), with which it shares only what np_linalg_common.h holds: the panel width kNB, the size limit, blocks_for, read_info.
//
//   n <= kNB    one launch of chol_diag_kernel: the matrix is one diagonal block.
//   otherwise   right-looking with panel width kNB on a work matrix W whose strict upper triangle is scratch (np_potrf: a
//               pool copy of a's lower triangle, written back at the end; np_cholesky: the result array, whose upper
//               triangle is zeroed at the end).  Per panel: chol_diag_kernel (one wave: L11), chol_trsm_kernel
//               (L21 = A21 L11^-T, a row per lane, which also writes L21^T into pool scratch) and A22 -= L21 (L21^T) on
//               np::sgemm_sub_ld, one launch per strip of columns (at most four a panel) from the strip's diagonal
//               downwards.  The tiles that cross the diagonal leave garbage above it: in W, never in the caller's.
// No pivot search, no atomics; *info is written by one lane per panel and the stream orders the panels.
#include "np_linalg_common.h"

namespace {

using namespace np::linalg;

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

// ---- host side ----

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

}  // namespace

extern "C" {

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

}  // extern "C"
