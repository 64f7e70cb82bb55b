// The two Jacobi solvers: the SVD (np_svd, np_svdvals) and the symmetric eigensolver (np_eigh, np_eigvalsh,
// np_symmetry_mismatch).  Both are blocked over pairs of 32-row blocks that meet in a round-robin tournament, both
// diagonalise a 64 x 64 symmetric matrix per block pair in LDS in fp64 and apply the product of its rotations on the MFMA, and
// both have a one-launch path for up to 64 rows.  They live in one file because they share kernels.
//
// Used by both solvers ("the Jacobi core", first in the file):
//   svd_apply_kernel      X <- M X for a block pair's 64 rows: W and Vt of the SVD, W and Vt of the eigensolver (the name is kept:
//                         DESIGN.md, docs/COVERAGE.md and the profiles refer to it).  It is the only __global__ both launch.
//   jacobi_pair / jacobi_row        the tournament and the rows of a block pair
//   jacobi_rotation                 c, s from (g_pp, g_qq, g_pq)
//   jacobi_rank_of                  the stable rank, descending (singular values) or ascending (eigenvalues)
//   jacobi_stage_m / jacobi_acc_row M into LDS and the row an MFMA 32x32 accumulator register holds
//   JacobiCtl, JacobiDebug, read_out2, end_sweep, sweep_info on the host side
// The SVD's alone keep svd_ in their name, the eigensolver's eigh_.
//
// Not shared, on purpose: what svd_eig_kernel and eigh_eig_kernel do between loading G and storing M.  Both count the pairs above
// their tolerance (the same dozen lines, with svd_active in one and eigh_active in the other) and then run the cyclic two-sided
// Jacobi on the 64 x 64 matrix in LDS.  eigh_solve64 is that solve for eigh_eig_kernel and eigh_small_kernel; svd_eig_kernel keeps
// its own loop, which differs in more than the rule (a flag set by a plain store where the eigensolver counts rotations with an
// atomic, M always there, 64 rows as a constant).  One template for both was built and measured: np_svd lost 4 % on every blocked
// size (profiles/linalg/split_ab.log).  svd_eig_kernel is nine tenths of a large SVD's time, so it is kept instruction for
// instruction what it was (profiles/linalg/split_resources.txt).
//
// The only cross-workgroup sums are integer counters and an integer max of float bit patterns: order-independent, so every call
// gives the same bits.
#include <limits.h>

#include "np_linalg_common.h"

namespace {

using namespace np::linalg;

// ---- the Jacobi core ----

constexpr int kJacB = 32;                // rows of a block
constexpr int kJacP = 2 * kJacB;         // rows of a block pair
constexpr int kJacStr = kJacP + 1;       // row stride of a 64 x 64 matrix in LDS
constexpr size_t kJacMaxDim = 65536;
constexpr size_t kJacSolveLds = 2 * (size_t)kJacP * kJacStr * sizeof(double);   // dynamic LDS of the 64 x 64 solves: G and M

typedef float jacobi_v16f __attribute__((ext_vector_type(16)));

struct JacobiCtl {
    unsigned long long above;        // (row) pairs found above the tolerance by any workgroup of the sweep (0 = converged)
    unsigned long long above_once;   // the same with every pair counted once (k (k - 1) / 2 at most: 2^31 at k = 65536)
    unsigned bits;                   // a float's bit pattern, an integer max: see svd_rownorm_kernel and eigh_pack_kernel
    int pad;
};

// the np_debug_* hooks of one solver
struct JacobiDebug {
    int max_sweeps;    // np_debug_*_max_sweeps: the sweep cap when > 0
    int last_sweeps;   // np_debug_*_last_sweeps
    int small_off;     // np_debug_*_small_path(0): every shape takes the blocked path (A/B, tests)
};
JacobiDebug g_svd_dbg = {0, 0, 0}, g_eigh_dbg = {0, 0, 0};

// block pair j of tournament step `step` over nblk (even) blocks: position 0 stays, the others go round
__device__ __forceinline__ void jacobi_pair(int nblk, int step, int j, int &p, int &q) {
    const int r = nblk - 1;
    const int a = j == 0 ? 0 : 1 + (j - 1 + step) % r;
    const int b = 1 + (nblk - 2 - j + step) % r;
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// global row of local row k (0 .. 63) of the block pair (p, q)
__device__ __forceinline__ size_t jacobi_row(int p, int q, int k) {
    return k < kJacB ? (size_t)p * kJacB + k : (size_t)q * kJacB + (k - kJacB);
}

// the row (0 .. 31) of the 32 x 32 tile that register r (0 .. 15) of a v_mfma_f32_32x32x2_f32 accumulator holds in a lane of
// half kq (lane >> 5); the column is lane & 31
__device__ __forceinline__ int jacobi_acc_row(int r, int kq) { return (r & 3) + 8 * (r >> 2) + 4 * kq; }

// Ms (LDS, kJacP x kJacStr) := block pair `pair`'s M of Mbuf, by 256 threads; the caller's barrier publishes it
__device__ __forceinline__ void jacobi_stage_m(float *Ms, const float *Mbuf, int pair) {
    const float *Mg = Mbuf + (size_t)pair * (kJacP * kJacP);
    for (int idx = threadIdx.x; idx < kJacP * kJacP; idx += 256) Ms[(idx >> 6) * kJacStr + (idx & 63)] = Mg[idx];
}

// the rotation that annihilates g_pq of the symmetric [[g_pp, g_pq], [g_pq, g_qq]] (g_pq != 0): the smaller root t, c, s = c t
__device__ __forceinline__ void jacobi_rotation(double gpp, double gqq, double gpq, double &c, double &s) {
    const double z = (gqq - gpp) / (2.0 * gpq);
    const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
    c = 1.0 / sqrt(1.0 + t * t);
    s = c * t;
}

// Position of v[i] among v[0 .. n): descending (a NaN first) or ascending (a NaN last), stable: the lower index first among equals,
// -0.0f == +0.0f.  A NaN counts as larger than every number and equal to a NaN: the ranks are a permutation.
template <bool Descending>
__device__ __forceinline__ int jacobi_rank_of(const float *v, size_t n, size_t i) {
    const float vi = v[i];
    const bool ni = vi != vi;
    int r = 0;
    for (size_t j = 0; j < n; ++j) {
        const float vj = v[j];
        const bool nj = vj != vj;
        const bool before = Descending ? ((nj && !ni) || vj > vi) : ((ni && !nj) || vj < vi);
        const bool equal = (nj && ni) || vj == vi;
        r += (before || (equal && j < i)) ? 1 : 0;
    }
    return r;
}

// Whether a pair rotates, from (g_pp, g_qq, g_pq).
// SVD: a, b squared norms, g the dot product; lim: both norms at or under it = a negligible pair
constexpr double kSvdTol = 4.0 * 1.1920928955078125e-7;
__device__ __forceinline__ bool svd_active(double a, double b, double g, double lim) {
    return a > 0.0 && b > 0.0 && !(a <= lim && b <= lim) && fabs(g) > kSvdTol * sqrt(a * b);
}
// eigensolver: |w_pq| against a limit fixed for the call.  Diagonals may be zero or negative, so sqrt(g_pp g_qq) has no meaning here.
__device__ __forceinline__ bool eigh_active(double g, double lim) { return fabs(g) > lim; }

// X <- M X for the block pair's 64 rows of W (chunks 0 .. wchunks - 1 of 128 columns) and of V (the chunks after them).
// Both solvers launch it: M comes from svd_eig_kernel or from eigh_eig_kernel.
__global__ __launch_bounds__(256) void svd_apply_kernel(float *W, size_t ldw, int wchunks, float *V, size_t ldv, int nblk,
                                                        int step, const float *Mbuf, const int *flag) {
    __shared__ float Ms[kJacP * kJacStr];
    const int pair = blockIdx.x;
    if (!flag[pair]) return;
    int p, q;
    jacobi_pair(nblk, step, pair, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    jacobi_stage_m(Ms, Mbuf, pair);
    __syncthreads();
    const bool onw = (int)blockIdx.y < wchunks;
    float *X = onw ? W : V;
    const size_t ld = onw ? ldw : ldv;
    const size_t col0 = (size_t)(onw ? blockIdx.y : blockIdx.y - wchunks) * 128 + (size_t)wave * 32;
    if (col0 >= ld) return;   // ld is a multiple of 32: a wave's 32 columns are all there or none is
    const int i = lane & 31, kq = lane >> 5;
    float b[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) b[kk] = X[jacobi_row(p, q, 2 * kk + kq) * ld + col0 + i];
    jacobi_v16f acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ms[i * kJacStr + 2 * kk + kq], b[kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ms[(32 + i) * kJacStr + 2 * kk + kq], b[kk], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = jacobi_acc_row(r, kq);
        X[((size_t)p * kJacB + lr) * ld + col0 + i] = acc0[r];
        X[((size_t)q * kJacB + lr) * ld + col0 + i] = acc1[r];
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
// A zero row never rotates, so the padding stays what it is.
constexpr int kSvdMaxSplit = 16;         // partial Grams per pair at most
constexpr int kSvdSweepCap = 60;         // 26 sweeps at 4096 x 4096: the count grows with n
constexpr int kSvdInnerCap = 10;         // sweeps of the 64 x 64 eigenproblem at most (any orthogonal M is a valid step)

// squared norm of every row (a wave per row, one fixed order) and the largest of them into ctl->bits: for the SVD the pattern
// is that of the largest squared row norm at the start of the sweep (the negligible-pair rule of svd_active)
__global__ __launch_bounds__(256) void svd_rownorm_kernel(const float *W, size_t ld, size_t nrows, float *normsq, JacobiCtl *ctl) {
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
        atomicMax(&ctl->bits, __float_as_uint(acc));   // non-negative floats order as their bits (a NaN ends on top)
    }
}

__global__ __launch_bounds__(256) void svd_gram_kernel(const float *W, size_t ld, int nblk, int step, int tiles_per_split,
                                                       int ntiles, int nsplit, float *Gpart) {
    __shared__ float T[kJacP * 33];
    int p, q;
    jacobi_pair(nblk, step, blockIdx.x, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bi = wave >> 1, bj = wave & 1, i = lane & 31, kq = lane >> 5;
    jacobi_v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int t0 = blockIdx.y * tiles_per_split;
    const int t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
    const int col = tid & 31, r0 = tid >> 5;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = r0 + 8 * u;
            T[row * 33 + col] = W[jacobi_row(p, q, row) * ld + (size_t)t * 32 + col];
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
    float *out = Gpart + ((size_t)blockIdx.x * nsplit + blockIdx.y) * (kJacP * kJacP);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = bi * 32 + jacobi_acc_row(r, kq);
        out[row * kJacP + bj * 32 + i] = acc[r];
    }
}

// dynamic LDS: G and M (kJacSolveLds).  The count and the 64 x 64 solve are written out here and not shared with the eigensolver:
// see the head of the file.
__global__ __launch_bounds__(256) void svd_eig_kernel(const float *Gpart, int nsplit, int step, float thr, JacobiCtl *ctl,
                                                      float *Mbuf, int *flag) {
    extern __shared__ double svd_sm[];
    double *G = svd_sm, *M = svd_sm + kJacP * kJacStr;
    __shared__ double cs_c[32], cs_s[32];
    __shared__ int cs_p[32], cs_q[32];
    __shared__ int s_cnt[2];
    __shared__ int s_rot;
    const int tid = threadIdx.x, pair = blockIdx.x;
    const float *gp = Gpart + (size_t)pair * nsplit * (kJacP * kJacP);
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) {
        float acc = gp[idx];   // (folding in fp64 instead was tried: no fewer sweeps)
        for (int s = 1; s < nsplit; ++s) acc += gp[(size_t)s * (kJacP * kJacP) + idx];
        const int r = idx >> 6, c = idx & 63;
        G[r * kJacStr + c] = (double)acc;
        M[r * kJacStr + c] = r == c ? 1.0 : 0.0;
    }
    if (tid < 2) s_cnt[tid] = 0;
    if (tid == 0) s_rot = 0;
    __syncthreads();
    const double maxsq = (double)__uint_as_float(ctl->bits);
    const double lim = (double)thr * (double)thr * maxsq;
    int all = 0, once = 0;
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < j && svd_active(G[i * kJacStr + i], G[j * kJacStr + j], G[i * kJacStr + j], lim)) {
            ++all;
            if (step == 0 || ((i < kJacB) != (j < kJacB))) ++once;   // rows of one block meet again in every step
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
        for (int st = 0; st < kJacP - 1; ++st) {
            if (tid < 32) {
                jacobi_pair(kJacP, st, tid, p, q);
                const double gpp = G[p * kJacStr + p], gqq = G[q * kJacStr + q], gpq = G[p * kJacStr + q];
                double c = 1.0, s = 0.0;
                mine = svd_active(gpp, gqq, gpq, lim);
                if (mine) {
                    jacobi_rotation(gpp, gqq, gpq, c, s);
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
                        const int rp = cs_p[pr] * kJacStr + col, rq = cs_q[pr] * kJacStr + col;
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
                        const int cp = row * kJacStr + cs_p[pr], cq = row * kJacStr + cs_q[pr];
                        const double gp_ = G[cp], gq_ = G[cq];
                        G[cp] = c * gp_ - s * gq_;
                        G[cq] = s * gp_ + c * gq_;
                    }
                }
            }
            __syncthreads();
            if (tid < 32 && mine) {
                G[p * kJacStr + q] = 0.0;
                G[q * kJacStr + p] = 0.0;
            }
        }
        __syncthreads();
        const int rot = s_rot;
        __syncthreads();
        if (tid == 0) s_rot = 0;
        __syncthreads();
        if (!rot) break;
    }
    float *out = Mbuf + (size_t)pair * (kJacP * kJacP);
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) out[idx] = (float)M[(idx >> 6) * kJacStr + (idx & 63)];
    if (tid == 0) flag[pair] = 1;
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
                jacobi_pair(ke, st, pj, rp, rq);
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
                double cd, sd;
                jacobi_rotation((double)sa, (double)sb, (double)sg, cd, sd);
                const float cf = (float)cd, sf = (float)sd;
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
    if (tid < k) {
        const int r = jacobi_rank_of<true>(nsq, (size_t)k, (size_t)tid);
        rank[tid] = r;
        p.s[r] = __fsqrt_rn(nsq[tid]);
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

// rank[i] = position of row i in descending order of its norm (jacobi_rank_of); s[rank[i]] = the norm
__global__ __launch_bounds__(256) void svd_rank_kernel(const float *normsq, size_t n, float *s, int *rank) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = jacobi_rank_of<true>(normsq, n, i);
    rank[i] = r;
    s[r] = __fsqrt_rn(normsq[i]);
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
// Two-sided (classical) Jacobi, blocked over pairs of 32-row blocks with the tournament above.  W is the symmetric matrix built
// from the lower triangle of a, padded with zeros to a multiple of 64 (a zero row and column never rotates); Vt starts as I and
// holds the eigenvectors as ROWS while iterating, so one row operation serves W and Vt.  Per step and block pair (I, J):
//   eigh_eig_kernel       reads the 64 x 64 pivot block W[IJ, IJ] (its lower triangle) straight from W, counts the pairs above the
//                         tolerance and, if there are any, diagonalises it in LDS in fp64: M (fp32, rounded once) and the diagonal D
//   svd_apply_kernel      W[IJ, :] <- M W[IJ, :] and Vt[IJ, :] <- M Vt[IJ, :], all pairs (disjoint rows)
//   eigh_colapply_kernel  W[:, IJ] <- W[:, IJ] M^T, all pairs (disjoint columns), in a launch of its own: a row half and a column
//                         half of two pairs overlap.  The pivot block is written as diag(D) with exact zeros off it.
// A pair (p, q) rotates when |w_pq| > kEighTol * scale, scale = the largest |entry| of the lower triangle of a, fixed at the start
// of the call (eigh_active).
// n <= 64 takes eigh_small_kernel: the same 64 x 64 LDS solve on the whole (padded) matrix, sort, signs and output in ONE launch.
constexpr int kEighSweepCap = 60;
constexpr double kEighTol = 1.1920928955078125e-7;   // eps: relative to the largest entry, not to the pair's diagonals

// W (npad x npad) from the lower triangle of a (n x n), zeros beyond n; the largest |entry| into ctl->bits: for the eigensolver
// the pattern is that of the largest |entry| of the lower triangle (a NaN ends on top), the scale of the whole call
__global__ __launch_bounds__(256) void eigh_pack_kernel(const float *a, size_t n, float *W, size_t npad, JacobiCtl *ctl) {
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
    if ((threadIdx.x & 63) == 0 && top != 0u) atomicMax(&ctl->bits, top);   // an integer max: order-independent
}

// Cyclic two-sided Jacobi on the symmetric G (fp64, LDS, row stride kJacStr, 64 x 64 of which the leading k x k is the problem and
// the rest zero) by 256 threads: the round-robin over its k rows (padded to an even count; the dummy never plays), up to 32 disjoint
// rotations per step, rotations accumulated as rows of M when M is given.  At most `cap` sweeps; a sweep without a rotation ends
// it.  Returns the sweeps taken (that last one included); *rot_last = the rotations of the last sweep.  eigh_eig_kernel and
// eigh_small_kernel call it; svd_eig_kernel has a solve of its own (see there).
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
                    jacobi_pair(ke, st, tid, p, q);
                    if (q < k) {   // else the dummy of an odd k
                        gpp = G[p * kJacStr + p];
                        gqq = G[q * kJacStr + q];
                        gpq = G[p * kJacStr + q];
                        mine = eigh_active(gpq, lim);
                    }
                }
                if (mine) {
                    jacobi_rotation(gpp, gqq, gpq, c, s);
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
                        const int rp = cs_p[pr] * kJacStr + col, rq = cs_q[pr] * kJacStr + col;
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
                        const int cp = row * kJacStr + cs_p[pr], cq = row * kJacStr + cs_q[pr];
                        const double gp_ = G[cp], gq_ = G[cq];
                        G[cp] = c * gp_ - s * gq_;
                        G[cq] = s * gp_ + c * gq_;
                    }
                }
            }
            __syncthreads();
            if (tid < 32 && mine) {
                G[p * kJacStr + q] = 0.0;
                G[q * kJacStr + p] = 0.0;
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

// dynamic LDS: G and M (kJacSolveLds)
__global__ __launch_bounds__(256) void eigh_eig_kernel(const float *W, size_t ld, int nblk, int step, JacobiCtl *ctl, float *Mbuf,
                                                       float *Dbuf, int *flag) {
    extern __shared__ double eigh_sm[];
    double *G = eigh_sm, *M = eigh_sm + kJacP * kJacStr;
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, pair = blockIdx.x;
    int p, q;
    jacobi_pair(nblk, step, pair, p, q);
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) {
        const int r = idx >> 6, c = idx & 63;   // p < q: the block's lower triangle is a part of W's
        const int hi = r > c ? r : c, lo = r > c ? c : r;
        G[r * kJacStr + c] = (double)W[jacobi_row(p, q, hi) * ld + jacobi_row(p, q, lo)];
        M[r * kJacStr + c] = r == c ? 1.0 : 0.0;
    }
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const double lim = kEighTol * (double)__uint_as_float(ctl->bits);
    int all = 0, once = 0;
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < j && eigh_active(G[i * kJacStr + j], lim)) {
            ++all;
            if (step == 0 || ((i < kJacB) != (j < kJacB))) ++once;   // rows of one block meet again in every step
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
    eigh_solve64(G, M, kJacP, lim, kEighSweepCap, &rot_last);
    if (tid == 0 && rot_last != 0) {
        atomicAdd(&ctl->above, (unsigned long long)rot_last);
        atomicAdd(&ctl->above_once, (unsigned long long)rot_last);
    }
    float *out = Mbuf + (size_t)pair * (kJacP * kJacP);
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) out[idx] = (float)M[(idx >> 6) * kJacStr + (idx & 63)];
    if (tid < kJacP) Dbuf[(size_t)pair * kJacP + tid] = (float)G[tid * kJacStr + tid];
    if (tid == 0) flag[pair] = 1;
}

// W[:, IJ] <- W[:, IJ] M^T for the block pair's 64 columns: a workgroup per pair and 128 rows, a wave per 32 rows.  The wave
// stages its 32 x 64 tile in LDS with row-contiguous loads (2 x 128 bytes per row), multiplies on the MFMA and stores rows again;
// the tile is read whole before anything is stored, and no other wave of the launch touches it.  The two waves whose rows are
// the pair's own write the pivot block instead: diag(D), exact zeros off it.
__global__ __launch_bounds__(256) void eigh_colapply_kernel(float *W, size_t ld, int nblk, int step, const float *Mbuf,
                                                            const float *Dbuf, const int *flag) {
    __shared__ float Ms[kJacP * kJacStr];
    __shared__ float Ts[4][kJacB * kJacStr];
    const int pair = blockIdx.x;
    if (!flag[pair]) return;
    int p, q;
    jacobi_pair(nblk, step, pair, p, q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    jacobi_stage_m(Ms, Mbuf, pair);
    const size_t row0 = (size_t)blockIdx.y * 128 + (size_t)wave * 32;
    const bool live = row0 < ld;   // ld is a multiple of 64: a wave's 32 rows are all there or none is
    const int rb = (int)(row0 / kJacB);
    const bool pivot = rb == p || rb == q;
    const size_t col = lane < kJacB ? (size_t)p * kJacB + lane : (size_t)q * kJacB + (lane - kJacB);
    float *T = Ts[wave];
    if (live && !pivot) {
#pragma unroll 8
        for (int rr = 0; rr < kJacB; ++rr) T[rr * kJacStr + lane] = W[(row0 + rr) * ld + col];
    }
    __syncthreads();
    if (!live) return;
    if (pivot) {
        const int l0 = rb == p ? 0 : kJacB;   // local index of the wave's first row
        const float d = Dbuf[(size_t)pair * kJacP + lane];
        for (int rr = 0; rr < kJacB; ++rr) W[(row0 + rr) * ld + col] = lane == l0 + rr ? d : 0.0f;
        return;
    }
    const int i = lane & 31, kq = lane >> 5;
    jacobi_v16f acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {   // out[r][j] = sum_k T[r][k] M[j][k]
        const float x = T[i * kJacStr + 2 * kk + kq];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, Ms[i * kJacStr + 2 * kk + kq], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, Ms[(32 + i) * kJacStr + 2 * kk + kq], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = jacobi_acc_row(r, kq);
        W[(row0 + lr) * ld + (size_t)p * kJacB + i] = acc0[r];
        W[(row0 + lr) * ld + (size_t)q * kJacB + i] = acc1[r];
    }
}

// diag[i] = W[i][i] for i < n, or NaN everywhere when the scale of the call is not finite (non-finite input)
__global__ __launch_bounds__(256) void eigh_diag_kernel(const float *W, size_t ld, size_t n, const JacobiCtl *ctl, float *diag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool finite = (ctl->bits & 0x7f800000u) != 0x7f800000u;
    diag[i] = finite ? W[i * ld + i] : __uint_as_float(0x7fc00000u);
}

// rank[i] = position of diag[i] in ascending order (jacobi_rank_of); w[rank[i]] = it
__global__ __launch_bounds__(256) void eigh_rank_kernel(const float *diag, size_t n, float *w, int *rank) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = jacobi_rank_of<false>(diag, n, i);
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
    double *G = eigh_small_sm, *M = p.vectors ? eigh_small_sm + kJacP * kJacStr : nullptr;
    __shared__ float s_diag[kJacP], s_vt[kJacP * kJacP];
    __shared__ int s_rank[kJacP], s_neg[kJacP];
    __shared__ unsigned s_scale;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = p.n;
    if (tid == 0) s_scale = 0u;
    __syncthreads();
    unsigned top = 0u;
    for (int idx = tid; idx < kJacP * kJacP; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        float v = 0.0f;
        if (r < n && c < n) v = r >= c ? p.a[r * n + c] : p.a[c * n + r];
        G[r * kJacStr + c] = (double)v;
        if (M) M[r * kJacStr + c] = r == c ? 1.0 : 0.0;
        const unsigned b = __float_as_uint(v) & 0x7fffffffu;
        top = b > top ? b : top;
    }
    atomicMax(&s_scale, top);
    __syncthreads();
    const bool finite = (s_scale & 0x7f800000u) != 0x7f800000u;
    const double lim = kEighTol * (double)__uint_as_float(s_scale);
    int rot_last = 0;
    const int sweeps = eigh_solve64(G, M, n, lim, p.cap, &rot_last);
    if (tid < n) s_diag[tid] = finite ? (float)G[tid * kJacStr + tid] : __uint_as_float(0x7fc00000u);
    __syncthreads();
    if (tid < n) {
        const int r = jacobi_rank_of<false>(s_diag, (size_t)n, (size_t)tid);
        s_rank[tid] = r;
        p.w[r] = s_diag[tid];
    }
    if (tid == 0) {
        p.out2[0] = rot_last;   // 0 when converged; at the cap: the pairs rotated in the last sweep
        p.out2[1] = sweeps;
    }
    if (!p.vectors) return;
    for (int idx = tid; idx < n * kJacP; idx += 256) s_vt[idx] = (float)M[(idx >> 6) * kJacStr + (idx & 63)];   // rounded once
    __syncthreads();
    for (int i = wave; i < n; i += 4) eigh_row_sign(s_vt + i * kJacP, n, lane, &s_neg[i]);   // a wave per row of Vt
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += 256) {
        const int i = idx / n, c = idx % n;
        const float x = s_vt[i * kJacP + c];
        p.v[(size_t)c * n + s_rank[i]] = s_neg[i] ? -x : x;
    }
}

// ---- host side ----

int sweep_cap(const JacobiDebug &dbg, int normal) { return dbg.max_sweeps > 0 ? dbg.max_sweeps : normal; }

// what a one-launch path left in out2: out2[0] = info, out2[1] = sweeps taken.  The host waits for the stream.
int read_out2(const np::Scratch &out2, int *info_host, JacobiDebug &dbg) {
    int host2[2] = {0, 0};
    if (int rc = np_memcpy_d2h(host2, out2.ptr, sizeof(host2))) return rc;
    *info_host = host2[0];
    dbg.last_sweeps = host2[1];
    return NP_OK;
}

// the blocked paths' sweep loop: it runs while !converged
struct SweepState {
    bool converged = false;
    unsigned long long last[2] = {0, 0};   // ctl's above, above_once after the latest sweep
};

// the end of sweep number `sweep`: the one host read of the sweep
int end_sweep(const JacobiCtl *ctl, int sweep, JacobiDebug &dbg, SweepState &st) {
    if (int rc = np_memcpy_d2h(st.last, ctl, sizeof(st.last))) return rc;
    st.converged = st.last[0] == 0;
    dbg.last_sweeps = sweep + 1;
    return NP_OK;
}

// info after the loop: 0 when converged, else the pairs still above the tolerance, each counted once, clipped to [1, INT_MAX]
int sweep_info(const SweepState &st) {
    if (st.converged) return 0;
    return st.last[1] > (unsigned long long)INT_MAX ? INT_MAX : (st.last[1] > 0 ? (int)st.last[1] : 1);
}

int debug_max_sweeps(JacobiDebug &dbg, const char *who, int sweeps) {
    if (sweeps < 0) return np::fail(NP_ERR_INVALID, "%s: %d", who, sweeps);
    dbg.max_sweeps = sweeps;
    return NP_OK;
}

int debug_last_sweeps(const JacobiDebug &dbg, const char *who, int *host_sweeps) {
    if (!host_sweeps) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    *host_sweeps = dbg.last_sweeps;
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
    if (k > (size_t)kJacP || g_svd_dbg.small_off) return 0;
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
    p.cap = sweep_cap(g_svd_dbg, kSvdSweepCap);
    p.thr = (float)L * 1.1920928955078125e-7f;
    p.u = u;
    p.s = s;
    p.vt = vt;
    p.out2 = (int *)out2.ptr;
    const size_t lds = svd_small_floats(k, L) * sizeof(float);
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)svd_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmallLdsBytes));
    svd_small_kernel<<<1, 1024, lds, np::stream()>>>(p);
    NP_LAUNCH_CHECK("svd_small_kernel");
    return read_out2(out2, info_host, g_svd_dbg);
}

// u, vt null: singular values only (no Vt, no normalisation; W goes through the same rotations, so s has the same bits)
int svd_impl(const char *who, const float *a, size_t m, size_t n, float *u, float *s, float *vt, int *info_host) {
    *info_host = 0;
    if (m == 0 || n == 0) return NP_OK;
    if (m > kJacMaxDim || n > kJacMaxDim) return np::fail(NP_ERR_INVALID, "%s: m, n = %zu, %zu: larger than %zu", who, m, n, kJacMaxDim);
    hipStream_t st = np::stream();
    const bool vectors = u != nullptr;
    const bool wide = m < n;                       // the transposed problem: the rows of a are the "columns"
    const size_t k = wide ? m : n, L = wide ? n : m;
    if (svd_small_floats(k, L) > 0) return svd_small(a, k, L, wide, u, s, vt, info_host);
    const size_t npad = (k + kJacP - 1) / kJacP * kJacP, ldw = (L + 31) & ~(size_t)31;
    const int nblk = (int)(npad / kJacB), pairs = nblk / 2, steps = nblk - 1;
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
    if (int rc = gpart.alloc((size_t)pairs * nsplit * kJacP * kJacP * sizeof(float))) return rc;
    if (int rc = mbuf.alloc((size_t)pairs * kJacP * kJacP * sizeof(float))) return rc;
    if (int rc = flag.alloc((size_t)pairs * sizeof(int))) return rc;
    if (int rc = ctl.alloc(sizeof(JacobiCtl))) return rc;
    if (int rc = normsq.alloc(npad * sizeof(float))) return rc;
    if (int rc = rank.alloc(npad * sizeof(int))) return rc;
    float *W = (float *)w.ptr, *V = (float *)v.ptr, *T = (float *)tmp.ptr;
    JacobiCtl *C = (JacobiCtl *)ctl.ptr;
    if (int rc = np_memset0(W, npad * ldw * sizeof(float))) return rc;
    if (wide) {
        if (int rc = np_copy2d(W, ldw, a, n, n, m)) return rc;
    } else {
        if (int rc = np_transpose2d(a, T, 1, m, n)) return rc;
        if (int rc = np_copy2d(W, ldw, T, m, m, n)) return rc;
    }
    if (vectors)
        if (int rc = np_identity(V, npad)) return rc;
    // every call: the attribute belongs to the current device's copy of the kernel, and setting it costs nothing next to a sweep
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)svd_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kJacSolveLds));
    const float thr = (float)L * 1.1920928955078125e-7f;   // max(m, n) eps
    const int wchunks = (int)((ldw + 127) / 128), vchunks = vectors ? (int)((npad + 127) / 128) : 0;
    g_svd_dbg.last_sweeps = 0;
    const int cap = sweep_cap(g_svd_dbg, kSvdSweepCap);
    SweepState state;
    for (int sweep = 0; sweep < cap && !state.converged; ++sweep) {
        NP_HIP_CHECK(hipMemsetAsync(C, 0, sizeof(JacobiCtl), st));
        svd_rownorm_kernel<<<blocks_for(k, 4), 256, 0, st>>>(W, ldw, k, (float *)normsq.ptr, C);
        NP_LAUNCH_CHECK("svd_rownorm_kernel");
        for (int step = 0; step < steps; ++step) {
            svd_gram_kernel<<<dim3(pairs, nsplit), 256, 0, st>>>(W, ldw, nblk, step, tps, ntiles, nsplit, (float *)gpart.ptr);
            NP_LAUNCH_CHECK("svd_gram_kernel");
            svd_eig_kernel<<<pairs, 256, kJacSolveLds, st>>>((const float *)gpart.ptr, nsplit, step, thr, C, (float *)mbuf.ptr,
                                                             (int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_eig_kernel");
            svd_apply_kernel<<<dim3(pairs, wchunks + vchunks), 256, 0, st>>>(W, ldw, wchunks, V, npad, nblk, step,
                                                                             (const float *)mbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_apply_kernel");
        }
        if (int rc = end_sweep(C, sweep, g_svd_dbg, state)) return rc;
    }
    *info_host = sweep_info(state);
    NP_HIP_CHECK(hipMemsetAsync(C, 0, sizeof(JacobiCtl), st));
    svd_rownorm_kernel<<<blocks_for(k, 4), 256, 0, st>>>(W, ldw, k, (float *)normsq.ptr, C);
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

int eigh_small(const float *a, size_t n, float *w, float *v, int *info_host) {
    np::Scratch out2;
    if (int rc = out2.alloc(2 * sizeof(int))) return rc;
    EighSmallArgs p = {};
    p.a = a;
    p.n = (int)n;
    p.vectors = v != nullptr ? 1 : 0;
    p.cap = sweep_cap(g_eigh_dbg, kEighSweepCap);
    p.w = w;
    p.v = v;
    p.out2 = (int *)out2.ptr;
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)eigh_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kJacSolveLds));
    eigh_small_kernel<<<1, 256, kJacSolveLds, np::stream()>>>(p);
    NP_LAUNCH_CHECK("eigh_small_kernel");
    return read_out2(out2, info_host, g_eigh_dbg);
}

// v null: eigenvalues only (no Vt; W goes through the same rotations, so w has the same bits)
int eigh_impl(const char *who, const float *a, size_t n, float *w, float *v, int *info_host) {
    *info_host = 0;
    if (n == 0) return NP_OK;
    if (n > kJacMaxDim) return np::fail(NP_ERR_INVALID, "%s: n = %zu: larger than %zu", who, n, kJacMaxDim);
    if (n <= (size_t)kJacP && !g_eigh_dbg.small_off) return eigh_small(a, n, w, v, info_host);
    hipStream_t st = np::stream();
    const bool vectors = v != nullptr;
    const size_t npad = (n + kJacP - 1) / kJacP * kJacP;
    const int nblk = (int)(npad / kJacB), pairs = nblk / 2, steps = nblk - 1;
    np::Scratch wm, vm, tmp, mbuf, dbuf, flag, ctl, diag, rank, neg;
    if (int rc = wm.alloc(npad * npad * sizeof(float))) return rc;
    if (vectors) {
        if (int rc = vm.alloc(npad * npad * sizeof(float))) return rc;
        if (int rc = tmp.alloc(n * n * sizeof(float))) return rc;   // the sorted rows of Vt on their way through a transpose
        if (int rc = neg.alloc(n * sizeof(int))) return rc;
    }
    if (int rc = mbuf.alloc((size_t)pairs * kJacP * kJacP * sizeof(float))) return rc;
    if (int rc = dbuf.alloc((size_t)pairs * kJacP * sizeof(float))) return rc;
    if (int rc = flag.alloc((size_t)pairs * sizeof(int))) return rc;
    if (int rc = ctl.alloc(sizeof(JacobiCtl))) return rc;
    if (int rc = diag.alloc(n * sizeof(float))) return rc;
    if (int rc = rank.alloc(n * sizeof(int))) return rc;
    float *W = (float *)wm.ptr, *V = (float *)vm.ptr;
    JacobiCtl *C = (JacobiCtl *)ctl.ptr;
    NP_HIP_CHECK(hipMemsetAsync(C, 0, sizeof(JacobiCtl), st));
    const unsigned rows_y = (unsigned)(npad < 4096 ? npad : 4096);
    eigh_pack_kernel<<<dim3(blocks_for(npad, 256), rows_y), 256, 0, st>>>(a, n, W, npad, C);
    NP_LAUNCH_CHECK("eigh_pack_kernel");
    if (vectors)
        if (int rc = np_identity(V, npad)) return rc;
    NP_HIP_CHECK(hipFuncSetAttribute((const void *)eigh_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kJacSolveLds));
    const int chunks = (int)((npad + 127) / 128);
    g_eigh_dbg.last_sweeps = 0;
    const int cap = sweep_cap(g_eigh_dbg, kEighSweepCap);
    SweepState state;
    for (int sweep = 0; sweep < cap && !state.converged; ++sweep) {
        NP_HIP_CHECK(hipMemsetAsync(C, 0, 2 * sizeof(unsigned long long), st));   // the counters; the scale stays
        for (int step = 0; step < steps; ++step) {
            eigh_eig_kernel<<<pairs, 256, kJacSolveLds, st>>>(W, npad, nblk, step, C, (float *)mbuf.ptr, (float *)dbuf.ptr,
                                                              (int *)flag.ptr);
            NP_LAUNCH_CHECK("eigh_eig_kernel");
            svd_apply_kernel<<<dim3(pairs, chunks + (vectors ? chunks : 0)), 256, 0, st>>>(
                W, npad, chunks, V, npad, nblk, step, (const float *)mbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("svd_apply_kernel");
            eigh_colapply_kernel<<<dim3(pairs, chunks), 256, 0, st>>>(W, npad, nblk, step, (const float *)mbuf.ptr,
                                                                      (const float *)dbuf.ptr, (const int *)flag.ptr);
            NP_LAUNCH_CHECK("eigh_colapply_kernel");
        }
        if (int rc = end_sweep(C, sweep, g_eigh_dbg, state)) return rc;
    }
    *info_host = sweep_info(state);
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

int np_debug_eigh_max_sweeps(int sweeps) { return debug_max_sweeps(g_eigh_dbg, "np_debug_eigh_max_sweeps", sweeps); }

int np_debug_eigh_small_path(int on) {
    g_eigh_dbg.small_off = on ? 0 : 1;
    return NP_OK;
}

int np_debug_eigh_last_sweeps(int *host_sweeps) { return debug_last_sweeps(g_eigh_dbg, "np_debug_eigh_last_sweeps", host_sweeps); }

int np_debug_svd_max_sweeps(int sweeps) { return debug_max_sweeps(g_svd_dbg, "np_debug_svd_max_sweeps", sweeps); }

int np_debug_svd_small_path(int on) {
    g_svd_dbg.small_off = on ? 0 : 1;
    return NP_OK;
}

int np_debug_svd_last_sweeps(int *host_sweeps) { return debug_last_sweeps(g_svd_dbg, "np_debug_svd_last_sweeps", host_sweeps); }

}  // extern "C"
