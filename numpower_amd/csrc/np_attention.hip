// Scaled dot-product attention for GPU arrays: np_attention_forward and np_attention_backward.
// The rules are in np_hip.h; this comment says how the kernels keep them.
//
// Operands are contiguous fp32: q (BH, Sq, D), k and v (BH, Sk, D), o (BH, Sq, D), the row statistics (BH, Sq).  The score matrix
// is never stored: every kernel forms one 32 x 32 block of it per wave in the MFMA accumulator and consumes it from there.
//
// All products run on v_mfma_f32_32x32x2_f32, an fp32 fmaf chain over the reduction index in ascending order.  With lane = (i, kq),
// i = lane & 31, kq = lane >> 5, the A operand of a step is A[i][kq], the B operand is B[kq][i], and register r of the accumulator
// is D[acc_row(r, kq)][i] (np_dnn.hip).  So a lane's 16 accumulator registers are 16 rows of ONE column i.
//
// Forward, attn_fwd_kernel<DP>: a workgroup of 4 waves owns kTQ = 128 query rows of one slice, a wave 32 of them.  The wave keeps
// its Q rows in registers as the B operand (lane (i, kq) holds q[i][2s + kq], s = 0 .. DP/2 - 1).  Key tiles of kTK = 32 keys are
// staged by the workgroup into LDS at the odd pitch DP + 1 (K and V, zero-filled past D and past Sk), the next tile's global loads
// being issued before the current tile's arithmetic.  Per tile the wave computes the TRANSPOSED block S^T = K . Q^T (A = K from
// LDS): lane (i, kq) then holds the scores of keys acc_row(r, kq) for query i, the other half-wave the other 16 keys of the SAME
// query.  Scale is one multiply of the finished chain; masked and tail keys become -Inf.  The tile maximum and the tile sum are
// folds over the 16 registers in r order plus one exchange with lane ^ 32 (half 0's value is always the left operand, so both
// halves hold the same bits).  The running pair (m, l) follows online_add of np_softmax.hip: a tile raises the maximum at most
// once, l and the accumulator are multiplied by ONE fast_exp of the step (ref(m) = m floored at -FLT_MAX), then the tile's
// e = fast_exp(s - ref(m)) are added.  The probabilities are already where the B operand of O^T += V^T . P^T needs them: step r
// pairs key acc_row(r, 0) of half 0 with key acc_row(r, 1) of half 1, A = V[key][d] from LDS.  The key order inside a tile is
// that fixed permutation.  O^T sits in DP/32 accumulators; the end divides each element by l (one IEEE division).  A row that
// ends with m = -Inf has seen nothing but -Inf: its l becomes NaN, which is what fast_exp(-Inf - m) gives, and so does its o.
// Under causal, a workgroup stops at the last key tile any of its rows sees, a wave skips the tiles wholly above its 32 rows, and
// the tiles that straddle the diagonal are masked per element.  Wave rows and key tiles are both 32 wide, so row i's tiles are
// exactly 0 .. i / 32 whatever Sq and Sk are.  The grid is then dealt heaviest workgroup first (the last query rows of every slice,
// then the rows before them), so that the short workgroups fill the gaps the long ones leave; the arithmetic of a row does not
// depend on which workgroup index computes it.
//
// Backward: attn_delta_kernel (a lane per row: delta = chain over d of do . o, multiply and add rounded separately),
// attn_dq_kernel<DP> (the forward's skeleton: S^T and dP^T = V . dO^T land in the same lanes, dS^T is the B operand of
// dQ^T += K^T . dS^T), and attn_dkdv_kernel<DP>: a workgroup owns 128 keys, a wave 32 of them with its K and V rows in registers as
// B operands, and walks the query tiles of 32 rows that see them in ascending order; Q, dO and the three row scalars are staged in
// LDS.  S = Q . K^T puts 16 queries of ONE key in a lane, so P and dS are again the B operands of dV^T += dO^T . P and
// dK^T += Q^T . dS.  The score chain multiplies the same pairs in the same order in all three kernels, so p has the forward's bits.
//
// A column of an accumulator never mixes with another column, so a NaN in a query row (forward, dq) or a key row (dkdv) stays in
// its lane; lanes of tail rows compute on zeros and are never stored.  No atomics; every order above is fixed by the extents
// and the tile constants.  Offsets are size_t; rows inside a slice are unsigned (Sq, Sk < 2^31); the grid is one-dimensional.
#include <float.h>

#include "np_elementwise_ops.h"

namespace {

typedef float attn_v16f __attribute__((ext_vector_type(16)));

constexpr int kTQ = 128;        // query rows per workgroup (forward, dq): 4 waves of kWaveRows
constexpr int kTK = 32;         // keys per staged tile (forward, dq); also the query tile of dkdv
constexpr int kWaveRows = 32;
constexpr int kKeysPerGroup = 128;   // keys per workgroup of attn_dkdv_kernel
constexpr int kMaxD = 128;
constexpr int kNumBounds = 7;
constexpr size_t kRowLim = (size_t)1 << 31;

int g_attn_d_class = 0;   // np_debug_attention_last_path
int g_attn_launches = 0;
size_t g_attn_key_tiles = 0;
size_t g_attn_skipped = 0;

struct AttnArgs {
    const float *q, *k, *v, *o, *dout, *smax_in, *ssum_in;
    float *out, *smax, *ssum;   // forward
    float *delta;               // backward scratch, [BH][Sq]
    float *dq, *dk, *dv;
    size_t rows;                // BH.Sq
    unsigned BH, Sq, Sk, D;
    unsigned nqt, nkt;          // query tiles of kTQ per slice; key tiles of kTK per slice
    unsigned nkg, nqt32;        // key groups of kKeysPerGroup per slice; query tiles of kTK per slice
    int causal;
    float scale;
};

__device__ __forceinline__ int acc_row(int r, int kq) { return (r & 3) + 8 * (r >> 2) + 4 * kq; }
__device__ __forceinline__ float row_max(float a, float b) { return np::dev::r_combine<NP_MAX>(a, b); }
__device__ __forceinline__ float floor_ref(float m) { return m > -FLT_MAX ? m : -FLT_MAX; }
// v of half 0 and of half 1, in that order, in both halves
__device__ __forceinline__ void halves(float v, int kq, float &h0, float &h1) {
    const float other = __shfl_xor(v, 32, 64);
    h0 = kq ? other : v, h1 = kq ? v : other;
}

// the workgroup's copy of a 32-row tile (rows row0 .. row0 + 31 of src, D floats each) in registers, zero past `rows` and D
template <int DP>
struct TileRegs {
    static constexpr int N = kTK * DP / 256;
    float x[N];
    __device__ __forceinline__ void load(const float *src, unsigned row0, unsigned rows, unsigned D, int tid) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int idx = tid + u * 256, row = idx / DP, d = idx % DP;
            const unsigned g = row0 + row;
            x[u] = (g < rows && (unsigned)d < D) ? src[(size_t)g * D + d] : 0.0f;
        }
    }
    __device__ __forceinline__ void store(float *lds, int tid) const {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const int idx = tid + u * 256, row = idx / DP, d = idx % DP;
            lds[row * (DP + 1) + d] = x[u];
        }
    }
};

// lane (i, kq)'s B operands of a chain over d: row[2s + kq], zero past D or when the row does not exist
template <int DP>
__device__ __forceinline__ void load_row_operand(float (&r)[DP / 2], const float *row, bool exists, unsigned D, int kq) {
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) {
        const unsigned d = 2 * s + kq;
        r[s] = (exists && d < D) ? row[d] : 0.0f;
    }
}

// acc = chain over d of tile[i][d] . b[d]: the 32 x 32 block (tile rows) x (this wave's columns)
template <int DP>
__device__ __forceinline__ attn_v16f chain_block(const float *tile, const float (&b)[DP / 2], int i, int kq) {
    attn_v16f acc = {};
#pragma unroll
    for (int s = 0; s < DP / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[i * (DP + 1) + 2 * s + kq], b[s], acc, 0, 0, 0);
    return acc;
}

// acc[nb] += tile^T . p: step r pairs tile row acc_row(r, 0) of half 0 with row acc_row(r, 1) of half 1
template <int DP>
__device__ __forceinline__ void accumulate_block(attn_v16f (&acc)[DP / 32], const float *tile, const float (&p)[16], int i, int kq) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float *row = tile + acc_row(r, kq) * (DP + 1) + i;
#pragma unroll
        for (int nb = 0; nb < DP / 32; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[nb * 32], p[r], acc[nb], 0, 0, 0);
    }
}

// the key tiles a query workgroup visits
__host__ __device__ __forceinline__ unsigned key_tiles_of(unsigned q0, unsigned Sq, unsigned nkt, int causal) {
    if (!causal) return nkt;
    const unsigned last = (q0 + kTQ < Sq ? q0 + kTQ : Sq) - 1, need = last / kTK + 1;
    return need < nkt ? need : nkt;
}

template <int DP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
    constexpr int PITCH = DP + 1, NB = DP / 32;
    __shared__ float Ks[kTK * PITCH], Vs[kTK * PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, kq = lane >> 5;
    // causal: the workgroups of the last query rows walk the most key tiles, so they are dealt first, slice by slice
    const unsigned qt = a.causal ? a.nqt - 1 - blockIdx.x / a.BH : blockIdx.x % a.nqt;
    const size_t b = a.causal ? blockIdx.x % a.BH : blockIdx.x / a.nqt;
    const unsigned q0 = qt * kTQ, w0 = q0 + wave * kWaveRows, qi = w0 + i;
    const float *kb = a.k + b * a.Sk * a.D, *vb = a.v + b * a.Sk * a.D;
    const bool wave_live = w0 < a.Sq, row_live = qi < a.Sq;

    float qr[DP / 2];
    load_row_operand<DP>(qr, a.q + (b * a.Sq + (row_live ? qi : 0)) * a.D, row_live, a.D, kq);
    attn_v16f oacc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) oacc[nb] = attn_v16f{};
    float m = -INFINITY, l = 0.0f;

    const unsigned kt_end = key_tiles_of(q0, a.Sq, a.nkt, a.causal);
    TileRegs<DP> pk, pv;
    pk.load(kb, 0, a.Sk, a.D, tid);
    pv.load(vb, 0, a.Sk, a.D, tid);
    for (unsigned kt = 0; kt < kt_end; ++kt) {
        const unsigned j0 = kt * kTK;
        __syncthreads();   // the tile before has been read
        pk.store(Ks, tid);
        pv.store(Vs, tid);
        __syncthreads();
        if (kt + 1 < kt_end) {
            pk.load(kb, j0 + kTK, a.Sk, a.D, tid);
            pv.load(vb, j0 + kTK, a.Sk, a.D, tid);
        }
        if (!wave_live || (a.causal && j0 > w0 + (kWaveRows - 1))) continue;   // wave-uniform: the tile is wholly above the wave's rows

        const attn_v16f s = chain_block<DP>(Ks, qr, i, kq);
        const bool mask = j0 + kTK > a.Sk || (a.causal && j0 + (kTK - 1) > w0);
        float x[16];
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned j = j0 + acc_row(r, kq);
            x[r] = s[r] * a.scale;
            if (mask && (j >= a.Sk || (a.causal && j > qi))) x[r] = -INFINITY;
            tm = row_max(tm, x[r]);
        }
        float h0, h1;
        halves(tm, kq, h0, h1);
        tm = row_max(h0, h1);
        const bool up = tm > m;
        const float f = up ? fast_exp(floor_ref(m) - floor_ref(tm)) : 1.0f;
        m = up ? tm : m;
        if (__any(up)) {   // a lane whose maximum stayed multiplies by exactly 1
            l = l * f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[nb][r] = oacc[nb][r] * f;
        }
        const float ref = floor_ref(m);
        float c = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            x[r] = fast_exp(x[r] - ref);
            c += x[r];
        }
        halves(c, kq, h0, h1);
        l += h0 + h1;
        accumulate_block<DP>(oacc, Vs, x, i, kq);
    }

    if (!row_live) return;
    if (m == -INFINITY) l = NAN;   // every visible score is -Inf: fast_exp(s - m) is fast_exp(-Inf + Inf) by the definition
    float *ob = a.out + (b * a.Sq + qi) * a.D;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned d = nb * 32 + acc_row(r, kq);
            if (d < a.D) ob[d] = __fdiv_rn(oacc[nb][r], l);
        }
    if (kq == 0) {
        if (a.smax) a.smax[b * a.Sq + qi] = m;
        if (a.ssum) a.ssum[b * a.Sq + qi] = l;
    }
}

// delta[row] = chain over d of dout . o, a lane per row
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnArgs a) {
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < a.rows; row += (size_t)gridDim.x * 256) {
        const float *po = a.o + row * a.D, *pd = a.dout + row * a.D;
        float t = 0.0f;
        for (unsigned d = 0; d < a.D; ++d) t += pd[d] * po[d];
        a.delta[row] = t;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void attn_dq_kernel(AttnArgs a) {
    constexpr int PITCH = DP + 1, NB = DP / 32;
    __shared__ float Ks[kTK * PITCH], Vs[kTK * PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, kq = lane >> 5;
    // causal: the workgroups of the last query rows walk the most key tiles, so they are dealt first, slice by slice
    const unsigned qt = a.causal ? a.nqt - 1 - blockIdx.x / a.BH : blockIdx.x % a.nqt;
    const size_t b = a.causal ? blockIdx.x % a.BH : blockIdx.x / a.nqt;
    const unsigned q0 = qt * kTQ, w0 = q0 + wave * kWaveRows, qi = w0 + i;
    const float *kb = a.k + b * a.Sk * a.D, *vb = a.v + b * a.Sk * a.D;
    const bool wave_live = w0 < a.Sq, row_live = qi < a.Sq;
    const size_t row = b * a.Sq + (row_live ? qi : 0);

    float qr[DP / 2], dor[DP / 2];
    load_row_operand<DP>(qr, a.q + row * a.D, row_live, a.D, kq);
    load_row_operand<DP>(dor, a.dout + row * a.D, row_live, a.D, kq);
    const float ref = floor_ref(row_live ? a.smax_in[row] : 0.0f), li = row_live ? a.ssum_in[row] : 1.0f;
    const float di = row_live ? a.delta[row] : 0.0f;
    attn_v16f acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = attn_v16f{};

    const unsigned kt_end = key_tiles_of(q0, a.Sq, a.nkt, a.causal);
    for (unsigned kt = 0; kt < kt_end; ++kt) {
        const unsigned j0 = kt * kTK;
        __syncthreads();
        {
            TileRegs<DP> t;
            t.load(kb, j0, a.Sk, a.D, tid);
            t.store(Ks, tid);
            t.load(vb, j0, a.Sk, a.D, tid);
            t.store(Vs, tid);
        }
        __syncthreads();
        if (!wave_live || (a.causal && j0 > w0 + (kWaveRows - 1))) continue;

        const attn_v16f s = chain_block<DP>(Ks, qr, i, kq);
        const attn_v16f dp = chain_block<DP>(Vs, dor, i, kq);
        const bool mask = j0 + kTK > a.Sk || (a.causal && j0 + (kTK - 1) > w0);
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned j = j0 + acc_row(r, kq);
            float x = s[r] * a.scale;
            if (mask && (j >= a.Sk || (a.causal && j > qi))) x = -INFINITY;
            const float p = __fdiv_rn(fast_exp(x - ref), li);
            ds[r] = p * (dp[r] - di);
        }
        accumulate_block<DP>(acc, Ks, ds, i, kq);
    }

    if (!row_live) return;
    float *ob = a.dq + row * a.D;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned d = nb * 32 + acc_row(r, kq);
            if (d < a.D) ob[d] = acc[nb][r] * a.scale;
        }
}

template <int DP>
__global__ __launch_bounds__(256) void attn_dkdv_kernel(AttnArgs a) {
    constexpr int PITCH = DP + 1, NB = DP / 32;
    __shared__ float Qs[kTK * PITCH], Os[kTK * PITCH], Rs[3 * kTK];   // Q, dO and (ref(m), l, delta) of the query tile
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, kq = lane >> 5;
    // causal: the workgroups of the first keys walk the most query tiles, so they are dealt first, slice by slice
    const unsigned kg = a.causal ? blockIdx.x / a.BH : blockIdx.x % a.nkg;
    const size_t b = a.causal ? blockIdx.x % a.BH : blockIdx.x / a.nkg;
    const unsigned k0 = kg * kKeysPerGroup, wk0 = k0 + wave * kWaveRows, kj = wk0 + i;
    const float *qb = a.q + b * a.Sq * a.D, *dob = a.dout + b * a.Sq * a.D;
    const bool wave_live = wk0 < a.Sk, key_live = kj < a.Sk;
    const size_t krow = b * a.Sk + (key_live ? kj : 0);
    const bool want_dk = a.dk != nullptr, want_dv = a.dv != nullptr;

    float kr[DP / 2], vr[DP / 2];
    load_row_operand<DP>(kr, a.k + krow * a.D, key_live, a.D, kq);
    load_row_operand<DP>(vr, a.v + krow * a.D, key_live, a.D, kq);
    attn_v16f dkacc[NB], dvacc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dkacc[nb] = attn_v16f{}, dvacc[nb] = attn_v16f{};

    // under causal the first query tile that sees key k0 is the one that holds row k0
    for (unsigned qt = a.causal ? k0 / kTK : 0; qt < a.nqt32; ++qt) {
        const unsigned i0 = qt * kTK;
        __syncthreads();
        {
            TileRegs<DP> t;
            t.load(qb, i0, a.Sq, a.D, tid);
            t.store(Qs, tid);
            t.load(dob, i0, a.Sq, a.D, tid);
            t.store(Os, tid);
        }
        if (tid < kTK) {
            const bool live = i0 + tid < a.Sq;
            const size_t row = b * a.Sq + (live ? i0 + tid : 0);
            Rs[tid] = floor_ref(live ? a.smax_in[row] : 0.0f);
            Rs[kTK + tid] = live ? a.ssum_in[row] : 1.0f;
            Rs[2 * kTK + tid] = live ? a.delta[row] : 0.0f;
        }
        __syncthreads();
        if (!wave_live || (a.causal && i0 + (kTK - 1) < wk0)) continue;   // wave-uniform: no row of the tile sees the wave's keys

        const attn_v16f s = chain_block<DP>(Qs, kr, i, kq);
        const attn_v16f dp = chain_block<DP>(Os, vr, i, kq);
        const bool mask = i0 + kTK > a.Sq || wk0 + kWaveRows > a.Sk || (a.causal && wk0 + (kWaveRows - 1) > i0);
        float p[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qrow = acc_row(r, kq);
            const unsigned qi = i0 + qrow;
            float x = s[r] * a.scale;
            if (mask && (qi >= a.Sq || !key_live || (a.causal && kj > qi))) x = -INFINITY;
            p[r] = __fdiv_rn(fast_exp(x - Rs[qrow]), Rs[kTK + qrow]);
            ds[r] = p[r] * (dp[r] - Rs[2 * kTK + qrow]);
        }
        if (want_dv) accumulate_block<DP>(dvacc, Os, p, i, kq);
        if (want_dk) accumulate_block<DP>(dkacc, Qs, ds, i, kq);
    }

    if (!key_live) return;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned d = nb * 32 + acc_row(r, kq);
            if (d < a.D) {
                if (want_dv) a.dv[krow * a.D + d] = dvacc[nb][r];
                if (want_dk) a.dk[krow * a.D + d] = dkacc[nb][r] * a.scale;
            }
        }
}

int d_class_of(size_t D) { return D <= 32 ? 32 : D <= 64 ? 64 : 128; }

// the extents and the scale of a call; no device is touched
int check_call(const char *who, size_t BH, size_t Sq, size_t Sk, size_t D, float scale) {
    if (BH < 1 || Sq < 1 || Sk < 1 || D < 1) return np::fail(NP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (D > (size_t)kMaxD) return np::fail(NP_ERR_INVALID, "%s: D = %zu is above %d", who, D, kMaxD);
    if (Sq >= kRowLim || Sk >= kRowLim) return np::fail(NP_ERR_INVALID, "%s: Sq or Sk is 2^31 or more", who);
    const size_t groups = (Sq + kTQ - 1) / kTQ > (Sk + kKeysPerGroup - 1) / kKeysPerGroup ? (Sq + kTQ - 1) / kTQ : (Sk + kKeysPerGroup - 1) / kKeysPerGroup;
    if (BH >= kRowLim || BH * groups >= kRowLim) return np::fail(NP_ERR_INVALID, "%s: BH times the tiles of a slice is 2^31 or more", who);
    const size_t S = Sq > Sk ? Sq : Sk, lim = SIZE_MAX / sizeof(float);
    if (S > lim / BH || BH * S > lim / D) return np::fail(NP_ERR_INVALID, "%s: BH.S.D does not fit a size_t", who);
    if (!(scale - scale == 0.0f)) return np::fail(NP_ERR_INVALID, "%s: scale must be finite", who);
    return NP_OK;
}

struct Range {
    const void *p;
    size_t count;   // floats; p == nullptr: absent
};

bool overlap(const Range &a, const Range &b) {
    if (!a.p || !b.p) return false;
    const uintptr_t p = (uintptr_t)a.p, q = (uintptr_t)b.p;
    return p < q + b.count * sizeof(float) && q < p + a.count * sizeof(float);
}

// true when an output overlaps an input or another output
bool any_overlap(const Range *out, int n_out, const Range *in, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (overlap(out[i], in[j])) return true;
        for (int j = i + 1; j < n_out; ++j)
            if (overlap(out[i], out[j])) return true;
    }
    return false;
}

void set_geometry(AttnArgs &a, size_t BH, size_t Sq, size_t Sk, size_t D, int causal, float scale) {
    a.rows = BH * Sq;
    a.BH = (unsigned)BH, a.Sq = (unsigned)Sq, a.Sk = (unsigned)Sk, a.D = (unsigned)D;
    a.nqt = (unsigned)((Sq + kTQ - 1) / kTQ), a.nkt = (unsigned)((Sk + kTK - 1) / kTK);
    a.nkg = (unsigned)((Sk + kKeysPerGroup - 1) / kKeysPerGroup), a.nqt32 = (unsigned)((Sq + kTK - 1) / kTK);
    a.causal = causal ? 1 : 0, a.scale = scale;
}

void record_path(const AttnArgs &a, int launches) {
    g_attn_d_class = d_class_of(a.D), g_attn_launches = launches;
    g_attn_key_tiles = key_tiles_of((a.nqt - 1) * kTQ, a.Sq, a.nkt, a.causal);
    size_t skipped = 0;
    for (unsigned qt = 0; qt < a.nqt; ++qt) skipped += a.nkt - key_tiles_of(qt * kTQ, a.Sq, a.nkt, a.causal);
    g_attn_skipped = skipped;
}

}  // namespace

extern "C" {

// The order is the pointers, the extents, the scale, the aliasing, ensure_init, then work: a refused call has touched no device.
int np_attention_forward(const float *q, const float *k, const float *v, size_t BH, size_t Sq, size_t Sk, size_t D, int causal, float scale,
                         float *o, float *save_max, float *save_sum) {
    const char *who = "np_attention_forward";
    if (!q || !k || !v || !o) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    if (int rc = check_call(who, BH, Sq, Sk, D, scale)) return rc;
    const size_t nq = BH * Sq * D, nk = BH * Sk * D, ns = BH * Sq;
    const Range in[] = {{q, nq}, {k, nk}, {v, nk}};
    const Range out[] = {{o, nq}, {save_max, ns}, {save_sum, ns}};
    if (any_overlap(out, 3, in, 3)) return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output", who);
    if (int rc = np::ensure_init()) return rc;
    AttnArgs a = {};
    a.q = q, a.k = k, a.v = v, a.out = o, a.smax = save_max, a.ssum = save_sum;
    set_geometry(a, BH, Sq, Sk, D, causal, scale);
    const unsigned grid = (unsigned)(BH * a.nqt);
    hipStream_t st = np::stream();
    switch (d_class_of(D)) {
        case 32: attn_fwd_kernel<32><<<grid, 256, 0, st>>>(a); break;
        case 64: attn_fwd_kernel<64><<<grid, 256, 0, st>>>(a); break;
        default: attn_fwd_kernel<128><<<grid, 256, 0, st>>>(a); break;
    }
    NP_LAUNCH_CHECK("attn_fwd_kernel");
    record_path(a, 1);
    return NP_OK;
}

int np_attention_backward(const float *q, const float *k, const float *v, const float *o, const float *dout, const float *save_max,
                          const float *save_sum, size_t BH, size_t Sq, size_t Sk, size_t D, int causal, float scale, float *dq, float *dk,
                          float *dv) {
    const char *who = "np_attention_backward";
    if (!q || !k || !v || !o || !dout || !save_max || !save_sum) return np::fail(NP_ERR_INVALID, "%s: null pointer", who);
    if (int rc = check_call(who, BH, Sq, Sk, D, scale)) return rc;
    const size_t nq = BH * Sq * D, nk = BH * Sk * D, ns = BH * Sq;
    const Range in[] = {{q, nq}, {k, nk}, {v, nk}, {o, nq}, {dout, nq}, {save_max, ns}, {save_sum, ns}};
    const Range out[] = {{dq, nq}, {dk, nk}, {dv, nk}};
    if (any_overlap(out, 3, in, 7)) return np::fail(NP_ERR_INVALID, "%s: an output overlaps an input or another output", who);
    AttnArgs a = {};
    a.q = q, a.k = k, a.v = v, a.o = o, a.dout = dout, a.smax_in = save_max, a.ssum_in = save_sum, a.dq = dq, a.dk = dk, a.dv = dv;
    set_geometry(a, BH, Sq, Sk, D, causal, scale);
    if (!dq && !dk && !dv) {   // nothing to produce: no launch, no scratch
        record_path(a, 0);
        return NP_OK;
    }
    if (int rc = np::ensure_init()) return rc;
    np::Scratch delta;   // released on every path below
    if (int rc = delta.alloc(ns * sizeof(float))) return rc;
    a.delta = (float *)delta.ptr;
    hipStream_t st = np::stream();
    int launches = 0;
    const size_t dgrid = (ns + 255) / 256;
    attn_delta_kernel<<<(unsigned)(dgrid < 65536 ? dgrid : 65536), 256, 0, st>>>(a);
    NP_LAUNCH_CHECK("attn_delta_kernel");
    launches += 1;
    const int dc = d_class_of(D);
    if (dk || dv) {
        const unsigned grid = (unsigned)(BH * a.nkg);
        switch (dc) {
            case 32: attn_dkdv_kernel<32><<<grid, 256, 0, st>>>(a); break;
            case 64: attn_dkdv_kernel<64><<<grid, 256, 0, st>>>(a); break;
            default: attn_dkdv_kernel<128><<<grid, 256, 0, st>>>(a); break;
        }
        NP_LAUNCH_CHECK("attn_dkdv_kernel");
        launches += 1;
    }
    if (dq) {
        const unsigned grid = (unsigned)(BH * a.nqt);
        switch (dc) {
            case 32: attn_dq_kernel<32><<<grid, 256, 0, st>>>(a); break;
            case 64: attn_dq_kernel<64><<<grid, 256, 0, st>>>(a); break;
            default: attn_dq_kernel<128><<<grid, 256, 0, st>>>(a); break;
        }
        NP_LAUNCH_CHECK("attn_dq_kernel");
        launches += 1;
    }
    record_path(a, launches);
    return NP_OK;
}

int np_debug_attention_last_path(int *d_class, int *q_tile, int *k_tile, int *launches, size_t *key_tiles, size_t *skipped) {
    if (!d_class || !q_tile || !k_tile || !launches || !key_tiles || !skipped)
        return np::fail(NP_ERR_INVALID, "np_debug_attention_last_path: null pointer");
    const bool any = g_attn_d_class != 0;
    *d_class = g_attn_d_class, *q_tile = any ? kTQ : 0, *k_tile = any ? kTK : 0, *launches = g_attn_launches;
    *key_tiles = g_attn_key_tiles, *skipped = g_attn_skipped;
    return NP_OK;
}

int np_debug_attention_bounds(size_t bounds[], int n) {
    if (!bounds) return np::fail(NP_ERR_INVALID, "np_debug_attention_bounds: null pointer");
    if (n < kNumBounds) return np::fail(NP_ERR_INVALID, "np_debug_attention_bounds: room for %d values is needed", kNumBounds);
    bounds[0] = kTQ, bounds[1] = kTK, bounds[2] = 32, bounds[3] = 64, bounds[4] = kMaxD, bounds[5] = kWaveRows, bounds[6] = kKeysPerGroup;
    return NP_OK;
}

}  // extern "C"
