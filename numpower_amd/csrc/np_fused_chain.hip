// Fused elementwise chains of libnp_hip.so: np_fused_chain and the np_fused_chain_reduce* family.
//
// acc = in[0]; for each op: acc = f(acc) | acc (op) in[k] | in[k] (op) acc; out = acc — ONE pass
// over HBM for a whole expression like exp(a) * b + 2 instead of one pass (and one temporary) per
// PHP-level op.  Every step goes through the same binary_apply / unary_apply bodies as the
// stand-alone kernels of np_elementwise.hip (np_elementwise_ops.h; contraction is off in both units),
// so a fused chain is bit-identical to the unfused sequence.  Inputs are full arrays of n elements,
// row / column vectors or scalars.
//
// This unit is the INTERPRETER: a kernel reads the chain's steps from its kernarg segment.  Four kernel
// families — flat (store, or a full reduction), last axis by lane group / workgroup, last axis staged
// through LDS, first axis — each with a launcher on the host side below; np_fused_static.hip holds the
// compiled straight-line kernels that the launchers hand a chain to when it is on their menu.
#include <math.h>

#include "np_internal.h"
#include "np_elementwise_ops.h"

// As in np_elementwise.hip: every multiply, add and divide is rounded on its own.
#pragma clang fp contract(off)

namespace {

constexpr size_t kColsWgPerCuDefault = 4;   // fused_chain_cols_kernel: 92.5 us vs 94-108 at 8 (profiles/r02/fused_cols_ab.log)

constexpr int FUSED_MAX_OPS = 12;
constexpr int FUSED_MAX_IN = 6;

// What the kernel interprets (built on the host from np_fused_op): operands are resolved to
// pointers / values up front so a step costs one uniform load of its descriptor.
enum { FUSED_SRC_SCALAR = 0, FUSED_SRC_STREAM = 1, FUSED_SRC_INPUT0 = 2 };
// how a streamed operand is indexed by the flat element index e of the rows x cols result
enum { FUSED_IDX_FULL = 0, FUSED_IDX_ROW = 1 /* e % cols */, FUSED_IDX_COL = 2 /* e / cols */, FUSED_IDX_ZERO = 3 };
struct FusedStep {
    int kind, op, swap, quirk;
    float p0, p1, scalar;
    int src_kind;
    const float *prefetch;   // array whose load is started when this step consumes its streamed operand
    size_t body_end;
    int prefetch_idx;        // FUSED_IDX_* of `prefetch`
    int pad;
};
struct FusedArgs {
    int n_ops;
    float scalar0;
    const float *in0;              // null -> scalar0
    const float *first_prefetch;   // first streamed operand of the chain (null: none)
    size_t cols;                   // row length of the result; 0 when no operand is broadcast
    int first_prefetch_idx;
    int sink;                      // -1: store the chain value; NP_SUM / NP_PROD / NP_MIN / NP_MAX: reduce it
    unsigned *ticket;              // full reduction on a small grid: the last workgroup folds the partials (np_internal.h) ...
    float *result;                 // ... into this device float; null ticket: np::fold_partials does, in a second launch
    unsigned div_m, div_s1, div_s2;   // e / cols for 32-bit e without a division (see fast_div)
    FusedStep ops[FUSED_MAX_OPS];
};
// The kernel indexes ops[] with a run-time k.  On a by-value kernel parameter that makes the compiler
// copy the whole struct to scratch (private memory) first; reading it through the kernarg segment
// pointer (constant address space) keeps every descriptor fetch a scalar load.
typedef const __attribute__((address_space(4))) FusedArgs *FusedArgsK;

constexpr bool binary_has_quirk(int op) {
    return op == NP_MULTIPLY || op == NP_MOD || op == NP_EQUAL || op == NP_NOT_EQUAL;
}

// One op applied to all N elements a thread holds: the op switch below runs once per op per
// thread-trip (uniform, scalar branch), not once per element.
template <int OP, int N>
__device__ __forceinline__ void unary_all(float (&acc)[N], float p0, float p1) {
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = unary_apply<OP>(acc[e], p0, p1);
}

// pow inside the chain interpreter goes through ONE out-of-line copy: inlined, its fp64 temporaries for 8
// elements took the full interpreter from 124 to 139 VGPRs (4 -> 3 waves per SIMD) for every chain
// that merely might contain a pow.
__device__ __attribute__((noinline)) float pow_outlined(float x, float y) { return fast_pow(x, y); }

template <int OP, int N>
__device__ __forceinline__ void binary_all(float (&acc)[N], const float (&oth)[N], bool swap, bool quirk,
                                           const bool (&body)[N]) {
    if constexpr (OP == NP_POW) {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = swap ? pow_outlined(oth[e], acc[e]) : pow_outlined(acc[e], oth[e]);
        return;
    }
    // `swap` and `quirk` are uniform: one branch each per step, not a select per element
    if (binary_has_quirk(OP) && quirk) {
        if (swap) {
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = binary_apply<OP, binary_has_quirk(OP)>(oth[e], acc[e], body[e]);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = binary_apply<OP, binary_has_quirk(OP)>(acc[e], oth[e], body[e]);
        }
    } else if (swap) {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = binary_apply<OP, false>(oth[e], acc[e], false);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = binary_apply<OP, false>(acc[e], oth[e], false);
    }
}

// Register allocation is static: a kernel that CAN run powf or tanf on 8 elements is allocated for
// them even when the chain is exp -> multiply -> add, and pays in occupancy.  So there are two
// interpreters: LIGHT knows only the ops whose bodies are a handful of instructions (the common
// arithmetic chains), the full one knows everything; np_fused_chain picks per chain.
constexpr bool fused_light_unary(int op) {
    switch (op) {
        case NP_ABS: case NP_SQRT: case NP_EXP: case NP_EXP2: case NP_LOG: case NP_LOG2: case NP_LOG10:
        case NP_DEGREES: case NP_RADIANS: case NP_RINT: case NP_FIX: case NP_FLOOR: case NP_CEIL:
        case NP_TRUNC: case NP_NEGATE: case NP_SIGN: case NP_CLIP: case NP_ROUND: case NP_RSQRT:
        case NP_POSITIVE: case NP_RECIPROCAL: case NP_UNARY_SQUARE:
            return true;
        default:
            return false;
    }
}
// (adding the hand-written log1p / hyperbolic ops here cost the exp -> multiply -> add chain 3-5 %,
// adding expm1 / tanh / arc* 10 %: the set stays minimal)
constexpr bool fused_light_binary(int op) { return op != NP_MOD && op != NP_POW && op != NP_ARCTAN2; }

template <int N, bool LIGHT>
__device__ __forceinline__ void unary_dispatch(int op, float (&acc)[N], float p0, float p1) {
#define NP_UD(OP_)                                                                     \
    case OP_:                                                                          \
        if constexpr (!LIGHT || fused_light_unary(OP_)) unary_all<OP_, N>(acc, p0, p1); \
        break
    switch (op) {
        NP_UD(NP_ABS); NP_UD(NP_SQRT); NP_UD(NP_EXP); NP_UD(NP_EXP2); NP_UD(NP_EXPM1); NP_UD(NP_LOG);
        NP_UD(NP_LOG2); NP_UD(NP_LOG10); NP_UD(NP_LOG1P); NP_UD(NP_LOGB); NP_UD(NP_SIN); NP_UD(NP_COS);
        NP_UD(NP_TAN); NP_UD(NP_ARCSIN); NP_UD(NP_ARCCOS); NP_UD(NP_ARCTAN); NP_UD(NP_DEGREES);
        NP_UD(NP_RADIANS); NP_UD(NP_SINH); NP_UD(NP_COSH); NP_UD(NP_TANH); NP_UD(NP_ARCSINH);
        NP_UD(NP_ARCCOSH); NP_UD(NP_ARCTANH); NP_UD(NP_RINT); NP_UD(NP_FIX); NP_UD(NP_FLOOR);
        NP_UD(NP_CEIL); NP_UD(NP_TRUNC); NP_UD(NP_SINC); NP_UD(NP_NEGATE); NP_UD(NP_SIGN); NP_UD(NP_CLIP);
        NP_UD(NP_ROUND); NP_UD(NP_RSQRT); NP_UD(NP_POSITIVE); NP_UD(NP_RECIPROCAL); NP_UD(NP_UNARY_SQUARE);
        default: break;
    }
#undef NP_UD
}

template <int N, bool LIGHT>
__device__ __forceinline__ void binary_dispatch(int op, float (&acc)[N], const float (&oth)[N], bool swap,
                                                bool quirk, const bool (&body)[N]) {
#define NP_BD(OP_)                                                                                        \
    case OP_:                                                                                             \
        if constexpr (!LIGHT || fused_light_binary(OP_)) binary_all<OP_, N>(acc, oth, swap, quirk, body); \
        break
    switch (op) {
        NP_BD(NP_ADD); NP_BD(NP_SUBTRACT); NP_BD(NP_MULTIPLY); NP_BD(NP_DIVIDE); NP_BD(NP_MOD); NP_BD(NP_POW);
        NP_BD(NP_ARCTAN2); NP_BD(NP_EQUAL); NP_BD(NP_NOT_EQUAL); NP_BD(NP_GREATER); NP_BD(NP_GREATER_EQUAL);
        NP_BD(NP_LESS); NP_BD(NP_LESS_EQUAL); NP_BD(NP_MAXIMUM); NP_BD(NP_MINIMUM);
        default: break;
    }
#undef NP_BD
}

// U slots of G contiguous elements per thread (G = 4: one float4 per slot), N = U*G values held in
// registers.  Slot v of a span starts at element elem0 + v*G.  Operand arrays are streamed: the
// load of the next array operand is issued as soon as the previous one has been consumed, so it is
// in flight while the steps in between compute; with input 0 that keeps two loads outstanding per
// thread without holding every input in registers (which cost occupancy: 6 inputs x 8 values).
// KEEP: the kernel variant for chains that name a full array MORE THAN ONCE (f(x) * y + x, (x - y) * y): full arrays are read with
// plain loads, so that the second read of a line finds it in the L2 — non-temporal loads do not leave it there and the array
// was streamed from HBM twice (10^8 elements: x * y + x 247 us = 16 B/elem -> 192 us; tools/sq_chain_probe.py).  A kernel of its
// own: the choice as a run-time branch in the common kernel cost the other chains 3-7 % (registers, occupancy 8 -> 7).
template <int U, int G, typename I, bool RAGGED = false, bool KEEP = false>
__device__ __forceinline__ void fused_fetch(float (&dst)[U * G], const float *p, int idx, const I (&first)[U],
                                            const I (&row)[U], const I (&col)[U], const bool (&live)[U],
                                            I ragged_cols = 0) {
    if (idx == FUSED_IDX_FULL) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (G == 4) {
                v4f t = v4f{0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (KEEP) {
                    if (live[u]) t = *(const v4f_u *)(p + (size_t)first[u]);
                } else {
                    if (live[u]) t = __builtin_nontemporal_load((const v4f_u *)(p + (size_t)first[u]));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[u * 4 + e] = t[e];
            } else {
                dst[u] = live[u] ? (KEEP ? p[(size_t)first[u]] : __builtin_nontemporal_load(p + (size_t)first[u])) : 0.0f;
            }
        }
    } else if (idx == FUSED_IDX_ROW) {
        // one row of `cols` floats, re-read by every result row: cache-resident, plain loads.  With cols % 4 != 0
        // (ragged_cols = cols, else 0) a slot may straddle two rows: those few slots walk the row with wrap-around.
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (G == 4) {
                v4f t = v4f{0.0f, 0.0f, 0.0f, 0.0f};
                if (live[u]) {
                    if (!RAGGED || col[u] + 3 < ragged_cols) {
                        t = *(const v4f_u *)(p + (size_t)col[u]);
                    } else {
                        I c = col[u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            t[e] = p[(size_t)c];
                            c = c + 1 == ragged_cols ? (I)0 : c + 1;
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[u * 4 + e] = t[e];
            } else {
                dst[u] = live[u] ? p[(size_t)col[u]] : 0.0f;
            }
        }
    } else {
        // one value per result row (column operand) or one value in all (0-d device scalar)
        if (RAGGED && G == 4 && idx == FUSED_IDX_COL) {   // uniform: a slot that runs into the next row takes that row's value for its tail
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool straddles = live[u] && col[u] + 3 >= ragged_cols;
                const float t0 = live[u] ? p[(size_t)row[u]] : 0.0f;
                const float t1 = straddles ? p[(size_t)row[u] + 1] : t0;
#pragma unroll
                for (int e = 0; e < G; ++e) dst[u * G + e] = (straddles && col[u] + e >= ragged_cols) ? t1 : t0;
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float t = live[u] ? p[idx == FUSED_IDX_COL ? (size_t)row[u] : (size_t)0] : 0.0f;
#pragma unroll
            for (int e = 0; e < G; ++e) dst[u * G + e] = t;
        }
    }
}

// VACC: the sink accumulates per register element (rv[u * G + e], for column reductions where every
// element of a slot belongs to a different result) instead of into the one scalar racc.
// [nan0_begin, nan0_end): the flat indices that are POSITION 0 of a reduced slice (element 0 of a full reduction, the first
// element of the row, row 0 of a column reduction).  NP_MIN / NP_MAX follow the reference's loop, which starts from that element
// (np_hip.h, np_reduce_op): a NaN chain value there becomes the accumulator, and stays — no later compare replaces a NaN.  It is
// always slot u = 0 of the first trip of the span's first thread (lane 0 / wave 0), the `a` side of every combine up to the
// writer, so it reaches the output (or partial 0 / chunk 0, where the folds look for it).
template <int U, int G, bool LIGHT, typename I, bool VACC, bool RAGGED = false, bool KEEP = false>
__device__ __forceinline__ void fused_span_impl(FusedArgsK f, float *__restrict__ out, I elem0, I nslots, I tid,
                                                I stride, float &racc, float (&rv)[U * G], I nan0_begin = 0, I nan0_end = 0) {
    constexpr int N = U * G;
    const int sink = f->sink;
    const int n_ops = f->n_ops;
    const float *in0 = f->in0, *first_prefetch = f->first_prefetch;
    const float scalar0 = f->scalar0;
    const int first_prefetch_idx = f->first_prefetch_idx;
    const I cols = (I)f->cols;
    const I ragged_cols = RAGGED ? cols : (I)0;   // float4 slots of a broadcast with cols % 4 != 0 may straddle rows (a kernel variant of its own:
                                                  // with the extra code in the common kernel, aligned exp(X) + col lost 9 %)
    const unsigned div_m = f->div_m, div_s1 = f->div_s1, div_s2 = f->div_s2;
    // does this thread's first slot (trip 0, u = 0) hold position 0 of a slice?  Decided once: the loop tests one flag
    bool own0 = sink >= NP_MIN && tid < nslots && elem0 + tid * G >= nan0_begin && elem0 + tid * G < nan0_end;
    for (I base = 0; base < nslots; base += stride * U) {
        I first[U], row[U], col[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const I v = base + (I)u * stride + tid;   // coalesced per u
            live[u] = v < nslots;
            first[u] = elem0 + v * G;
            row[u] = col[u] = 0;
            if (cols) {   // uniform: only chains with a broadcast operand need (row, col)
                if constexpr (sizeof(I) == 4)
                    row[u] = (I)fast_div((unsigned)first[u], div_m, div_s1, div_s2);
                else
                    row[u] = first[u] / cols;
                col[u] = first[u] - row[u] * cols;
            }
        }
        // the chain value starts as input 0 and lives in acc from the first load on: input 0 is not kept in a second
        // set of registers for the rare step that names it again (x * x ...) — that step re-reads it (an L2 hit in the KEEP
        // variant of the kernel, which such chains get), and every other chain saves N registers and N moves per trip
        float acc[N], nxt[N];
        if (in0) {
            fused_fetch<U, G, I, false, KEEP>(acc, in0, FUSED_IDX_FULL, first, row, col, live);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = scalar0;
        }
        if (first_prefetch) {
            fused_fetch<U, G, I, RAGGED, KEEP>(nxt, first_prefetch, first_prefetch_idx, first, row, col, live, ragged_cols);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) nxt[e] = 0.0f;
        }
        for (int k = 0; k < n_ops; ++k) {
            struct {
                int kind, op, swap, quirk, src_kind, prefetch_idx;
                float p0, p1, scalar;
                const float *prefetch;
                size_t body_end;
            } o = {f->ops[k].kind, f->ops[k].op, f->ops[k].swap, f->ops[k].quirk, f->ops[k].src_kind,
                   f->ops[k].prefetch_idx, f->ops[k].p0, f->ops[k].p1, f->ops[k].scalar, f->ops[k].prefetch,
                   f->ops[k].body_end};
            if (o.kind == NP_FUSED_UNARY) {
                unary_dispatch<N, LIGHT>(o.op, acc, o.p0, o.p1);
                continue;
            }
            float oth[N];
            bool body[N];
            // one uniform branch per step (written per element, the compiler emitted a branch ladder
            // for every one of the N selects)
            if (o.src_kind == FUSED_SRC_STREAM) {
#pragma unroll
                for (int e = 0; e < N; ++e) oth[e] = nxt[e];
            } else if (o.src_kind == FUSED_SRC_INPUT0) {
                if (in0) {
                    fused_fetch<U, G, I, false, KEEP>(oth, in0, FUSED_IDX_FULL, first, row, col, live);
                } else {
#pragma unroll
                    for (int e = 0; e < N; ++e) oth[e] = scalar0;
                }
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e) oth[e] = o.scalar;
            }
#pragma unroll
            for (int e = 0; e < N; ++e) {
                // body_end is a multiple of 8 and float4 slots start at multiples of 4: one flag per slot
                body[e] = (size_t)first[e / G] < o.body_end;
            }
            if (o.src_kind == FUSED_SRC_STREAM && o.prefetch)
                fused_fetch<U, G, I, RAGGED, KEEP>(nxt, o.prefetch, o.prefetch_idx, first, row, col, live, ragged_cols);
            binary_dispatch<N, LIGHT>(o.op, acc, oth, o.swap != 0, o.quirk != 0, body);
        }
        if constexpr (VACC) {
            if (sink == NP_SUM) {
#pragma unroll
                for (int e = 0; e < N; ++e) rv[e] += live[e / G] ? acc[e] : 0.0f;
            } else if (sink == NP_PROD) {
#pragma unroll
                for (int e = 0; e < N; ++e) rv[e] *= live[e / G] ? acc[e] : 1.0f;
            } else if (sink == NP_MIN) {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (live[e / G] && acc[e] < rv[e]) rv[e] = acc[e];
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (live[e / G] && acc[e] > rv[e]) rv[e] = acc[e];
            }
            if (own0) {   // (first trip, slot 0)
                own0 = false;
#pragma unroll
                for (int e = 0; e < G; ++e)
                    if (first[0] + (I)e < nan0_end && acc[e] != acc[e]) rv[e] = acc[e];
            }
            continue;
        }
        if (sink >= 0) {
            // reduction at the end of the chain: the value never goes to memory (uniform branch;
            // same combine rules as np_reduce_all: NaN never replaces in min / max, except the one in position 0 — below)
            if (sink == NP_SUM) {
#pragma unroll
                for (int e = 0; e < N; ++e) racc += live[e / G] ? acc[e] : 0.0f;
            } else if (sink == NP_PROD) {
#pragma unroll
                for (int e = 0; e < N; ++e) racc *= live[e / G] ? acc[e] : 1.0f;
            } else if (sink == NP_MIN) {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (live[e / G] && acc[e] < racc) racc = acc[e];
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (live[e / G] && acc[e] > racc) racc = acc[e];
            }
            if (own0) {   // (first trip, slot 0)
                own0 = false;
#pragma unroll
                for (int e = 0; e < G; ++e)
                    if (first[0] + (I)e < nan0_end && acc[e] != acc[e]) racc = acc[e];
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;
            if constexpr (G == 4)
                __builtin_nontemporal_store(v4f{acc[u * 4], acc[u * 4 + 1], acc[u * 4 + 2], acc[u * 4 + 3]},
                                            (v4f_u *)(out + (size_t)first[u]));
            else
                out[first[u]] = acc[u];
        }
    }
}

template <int U, int G, bool LIGHT, typename I, bool RAGGED = false, bool KEEP = false>
__device__ __forceinline__ void fused_span(FusedArgsK f, float *__restrict__ out, I elem0, I nslots, I tid,
                                           I stride, float &racc, I nan0_begin = 0, I nan0_end = 0) {
    float unused[U * G];
    fused_span_impl<U, G, LIGHT, I, false, RAGGED, KEEP>(f, out, elem0, nslots, tid, stride, racc, unused, nan0_begin, nan0_end);
}

__device__ __forceinline__ float sink_identity(int sink) {
    return sink == NP_SUM ? 0.0f : sink == NP_PROD ? 1.0f : sink == NP_MIN ? INFINITY : -INFINITY;
}
__device__ __forceinline__ float sink_combine(int sink, float a, float b) {   // np::dev::r_combine with a run-time op
    if (sink == NP_SUM) return a + b;
    if (sink == NP_PROD) return a * b;
    if (sink == NP_MIN) return (b < a) ? b : a;
    return (b > a) ? b : a;
}

// Chain ending in a reduction over the LAST axis: out[r] = reduce_c chain(r, c).  One wave per row
// (BLOCK = false; rows of up to a few thousand elements, no barrier anywhere) or one workgroup per
// row (BLOCK = true).  scale = 1 / cols for a mean (applied as a division, like NDArray::mean).
template <int G, bool LIGHT, bool BLOCK, typename I, int UU = 2>
__global__ __launch_bounds__(256) void fused_chain_rows_kernel(FusedArgs by_value, float *__restrict__ out, I rows, I cols,
                                                               unsigned L, I chunk_slots, float mean_div) {
    (void)by_value;
    FusedArgsK f = (FusedArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    const int sink = f->sink;
    // wave mode: groups of L lanes (a power of two <= 64) own a row each, so short rows still fill the wave
    const I lane = BLOCK ? threadIdx.x : (threadIdx.x & (L - 1));
    const I width = BLOCK ? 256 : L;
    const I groups = 64 / L;
    const I first_row = BLOCK ? (I)blockIdx.x : ((I)blockIdx.x * 4 + (threadIdx.x >> 6)) * groups + (threadIdx.x & 63) / L;
    const I row_stride = BLOCK ? (I)gridDim.x : (I)gridDim.x * 4 * groups;
    __shared__ float lds4[4];
    // workgroup mode may cut a row into gridDim.y chunks of chunk_slots slots (a handful of very long rows):
    // out then holds [row][chunk] partials for np_reduce_axis to fold
    const I slot0 = BLOCK ? (I)blockIdx.y * chunk_slots : 0;
    const I nslots = BLOCK ? (slot0 + chunk_slots < cols / G ? chunk_slots : cols / G - slot0) : cols / G;
    const I out_stride = BLOCK ? (I)gridDim.y : 1, out_off = BLOCK ? (I)blockIdx.y : 0;
    for (I r = first_row; r < rows; r += row_stride) {
        float racc = sink_identity(sink);
        fused_span<UU, G, LIGHT, I>(f, out, r * cols + slot0 * G, nslots, lane, width, racc, r * cols, r * cols + 1);
        if constexpr (G == 4) {   // a row of cols % 4 != 0 floats: its last 1-3 elements, one per lane, behind the float4 slots
            const I tail = cols - (cols / 4) * 4;
            if (tail != 0 && (!BLOCK || blockIdx.y == gridDim.y - 1))
                fused_span<1, 1, LIGHT, I>(f, out, r * cols + (cols / 4) * 4, tail, lane, width, racc, r * cols, r * cols + 1);
        }
        if constexpr (BLOCK) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) racc = sink_combine(sink, racc, __shfl_down(racc, off, 64));
        } else {
            for (unsigned off = L >> 1; off > 0; off >>= 1) racc = sink_combine(sink, racc, __shfl_xor(racc, (int)off, 64));
        }
        if constexpr (BLOCK) {
            if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = racc;
            __syncthreads();
            if (threadIdx.x == 0) {
                float v = lds4[0];
                for (int w = 1; w < 4; ++w) v = sink_combine(sink, v, lds4[w]);
                out[(size_t)r * out_stride + out_off] = mean_div != 0.0f ? v / mean_div : v;
            }
            __syncthreads();
        } else if (lane == 0) {
            out[r] = mean_div != 0.0f ? racc / mean_div : racc;
        }
    }
}

// Chain ending in a reduction over the FIRST axis of a rows x cols result: out[c] = reduce_r chain(r, c).
// A workgroup owns 64 slots of G columns; its four waves take every fourth row of the block's row chunk
// (blockIdx.y), each lane accumulating its own G columns (VACC), and are combined through LDS.  With
// more than one row chunk the partials [chunk][cols] are folded by np_reduce_axis.
template <int G, bool LIGHT, typename I, int CU = 2>
__global__ __launch_bounds__(256) void fused_chain_cols_kernel(FusedArgs by_value, float *__restrict__ out, I rows, I cols,
                                                               I rows_per_chunk, float mean_div) {
    (void)by_value;
    FusedArgsK f = (FusedArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    const int sink = f->sink;
    const I lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const I slots_per_row = cols / G;             // cols % G == 0
    const I r0 = (I)blockIdx.y * rows_per_chunk;
    const I r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    float rv[CU * G], racc = 0.0f;   // CU rows in flight per lane, one accumulator set per row slot
#pragma unroll
    for (int e = 0; e < CU * G; ++e) rv[e] = sink_identity(sink);
    // (256-slot column blocks, the whole workgroup walking down the chunk row by row with nothing to combine across waves,
    // were tried with no gain: docs/HISTORY.md round 2 item 7)
    const I slot = (I)blockIdx.x * 64 + lane;
    // slot index v of the span <-> (row r0 + v / slots_per_row, slot v % slots_per_row): this thread's
    // slots are v = (wave + 4 i) * slots_per_row + slot
    if (slot < slots_per_row)
        fused_span_impl<CU, G, LIGHT, I, true>(f, out, r0 * cols, (r1 - r0) * slots_per_row, wave * slots_per_row + slot,
                                              4 * slots_per_row, racc, rv, (I)0, cols);
    // cross-wave combine through LDS, lane fastest: a wave's 64 stores / loads of one element land on 64 different banks
    // (lane-major [lane][e] put lanes l and l + 16 on one bank: 74 % of this kernel's LDS cycles were conflicts)
    __shared__ float part[4][G][64];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        float v = rv[e];
        for (int u = 1; u < CU; ++u) v = sink_combine(sink, v, rv[u * G + e]);
        part[wave][e][lane] = v;
    }
    __syncthreads();
    float v[G];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        v[e] = part[0][e][lane];
        for (int w = 1; w < 4; ++w) v[e] = sink_combine(sink, v[e], part[w][e][lane]);
    }
    // One row of results per chunk of rows; with several chunks np_reduce_axis folds them in a second launch.  (Round 3
    // folded them here, in the last workgroup of each column block to finish — memory-side partials, a ticket per block,
    // profiles/r03/fused_cols_ab.log: 96 us against 75 + the ~9 us second launch.  The 64 partial rows arrive one
    // memory round trip after the other at the end of a kernel that has nothing left to hide them behind.)
    if (wave == 0 && slot < slots_per_row) {
#pragma unroll
        for (int e = 0; e < G; ++e) out[(size_t)blockIdx.y * cols + (size_t)slot * G + e] = mean_div != 0.0f ? v[e] / mean_div : v[e];
    }
}

template <bool VEC, int U, bool LIGHT, typename I, bool RAGGED = false, bool KEEP = false>
__global__ __launch_bounds__(256) void fused_chain_kernel(FusedArgs by_value, float *__restrict__ out, I n) {
    (void)by_value;   // first kernel argument: lives at offset 0 of the kernarg segment
    FusedArgsK f = (FusedArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    const I stride = (I)gridDim.x * blockDim.x;
    const I tid = (I)blockIdx.x * blockDim.x + threadIdx.x;
    const int sink = f->sink;
    float racc = sink == NP_SUM ? 0.0f : sink == NP_PROD ? 1.0f : sink == NP_MIN ? INFINITY : -INFINITY;
    if constexpr (VEC) {
        const I nvec = n / 4;
        fused_span<U, 4, LIGHT, I, RAGGED, KEEP>(f, out, (I)0, nvec, tid, stride, racc, (I)0, (I)1);
        fused_span<1, 1, LIGHT, I>(f, out, nvec * 4, n - nvec * 4, tid, stride, racc, (I)0, (I)1);   // ragged tail (< 4 elements)
    } else {
        fused_span<U, 1, LIGHT, I>(f, out, (I)0, n, tid, stride, racc, (I)0, (I)1);   // 4-byte aligned views
    }
    if (sink >= 0) {   // one partial per workgroup, folded in a fixed order (deterministic) by the last workgroup or a second launch
        __shared__ float lds4[4];
        unsigned *ticket = f->ticket;
        float *result = f->result;
#define NP_FOLD(OP_) np::dev::fold_in_last_workgroup<OP_>(np::dev::block_reduce<OP_>(racc, lds4), out, ticket, result, 1.0f, lds4)
        if (sink == NP_SUM) NP_FOLD(NP_SUM);
        else if (sink == NP_PROD) NP_FOLD(NP_PROD);
        else if (sink == NP_MIN) NP_FOLD(NP_MIN);
        else NP_FOLD(NP_MAX);
#undef NP_FOLD
    }
}

}  // namespace


// Chain ending in a reduction over the LAST axis of a matrix with very many SHORT rows (sum(exp(X), 1) over 10 classes):
// the row kernels above give a lane group to each row and load 4 bytes per lane at the row stride.  Here — as in
// reduce_rows_staged (np_reduce.hip), whose fold order this repeats, so that the fused result stays bit-identical to the
// op-by-op one — a workgroup walks a contiguous slab of R rows as the flat float4 stream it is, runs the chain on each
// float4 (every operand kind can be fetched there: the element's row and column are known), parks the chain values in
// LDS (row pitch len | 1 words) and then every thread folds its rows.  R is a multiple of 256, so slabs start on 16 bytes.
struct StagedCtx {
    FusedArgsK f;
    float *slab;          // LDS
    size_t base, row0;    // flat index / row index of the slab's first element
    unsigned len, pitch, magic;
};

// N values (one float4 or one element) of the slab through the chain; e = slab-relative flat index of the first.
// (Out of line — one copy of the interpreter, called once per float4 with all eight loads of a thread issued first —
// it cost 2.3x: register save / restore around every call, 0.129 -> 0.29 ms on 10^7 x 10.)
template <int N, bool LIGHT>
__device__ __forceinline__ void staged_run(const StagedCtx &cx, unsigned e, v4f x) {
    FusedArgsK f = cx.f;
    const float *in0 = f->in0;
    const unsigned len = cx.len;
    float acc[N];
    unsigned r[N], c[N];
    r[0] = __umulhi(e, cx.magic);                // e / len (magic = ceil(2^32 / len), exact for e < 2^16)
    c[0] = e - r[0] * len;
#pragma unroll
    for (int j = 1; j < N; ++j) {
        const bool wrap = c[j - 1] + 1 == len;
        c[j] = wrap ? 0u : c[j - 1] + 1;
        r[j] = r[j - 1] + (wrap ? 1u : 0u);
    }
    const size_t ge = cx.base + e;
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = x[j];
    auto fetch = [&](const float *p, int idx, float (&dst)[N]) {
        if (idx == FUSED_IDX_FULL) {
            if constexpr (N == 4) {
                const v4f t = *(const v4f_u *)(p + ge);
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[j] = t[j];
            } else {
                dst[0] = p[ge];
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                dst[j] = p[idx == FUSED_IDX_ROW ? (size_t)c[j] : idx == FUSED_IDX_COL ? cx.row0 + r[j] : (size_t)0];
        }
    };
    const float *stream = f->first_prefetch;
    int stream_idx = f->first_prefetch_idx;
    const int n_ops = f->n_ops;
    for (int k = 0; k < n_ops; ++k) {
        const int kind = f->ops[k].kind, op = f->ops[k].op;
        if (kind == NP_FUSED_UNARY) {
            unary_dispatch<N, LIGHT>(op, acc, f->ops[k].p0, f->ops[k].p1);
            continue;
        }
        float oth[N];
        bool body[N];
        const int src = f->ops[k].src_kind;
        if (src == FUSED_SRC_STREAM) {
            fetch(stream, stream_idx, oth);
            stream = f->ops[k].prefetch;
            stream_idx = f->ops[k].prefetch_idx;
        } else if (src == FUSED_SRC_INPUT0) {
            fetch(in0, FUSED_IDX_FULL, oth);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) oth[j] = f->ops[k].scalar;
        }
        const size_t body_end = f->ops[k].body_end;
#pragma unroll
        for (int j = 0; j < N; ++j) body[j] = ge + j < body_end;
        binary_dispatch<N, LIGHT>(op, acc, oth, f->ops[k].swap != 0, f->ops[k].quirk != 0, body);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) cx.slab[r[j] * cx.pitch + c[j]] = acc[j];
}

template <int SINK, bool LIGHT>
__global__ __launch_bounds__(256) void fused_chain_rows_staged_kernel(FusedArgs by_value, float *__restrict__ out,
                                                                      size_t rows_total, unsigned len, unsigned R,
                                                                      unsigned magic, float mean_div, unsigned T) {
    (void)by_value;
    extern __shared__ __attribute__((aligned(16))) float slab[];
    StagedCtx cx;
    cx.f = (FusedArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    cx.slab = slab;
    cx.len = len;
    cx.pitch = len | 1u;
    cx.magic = magic;
    cx.row0 = (size_t)blockIdx.x * R;
    cx.base = cx.row0 * len;
    const unsigned pitch = cx.pitch;
    const size_t row0 = cx.row0;
    const unsigned rows = (unsigned)(rows_total - row0 < R ? rows_total - row0 : R);
    const unsigned total = rows * len;
    const float *in0 = cx.f->in0;
    // two float4s of input 0 in flight per trip (the chain is a long stretch of code the compiler does not move loads
    // across): sum(exp(X), 1) on 10^7 x 10 0.129 ms with one, 0.109 with two, 0.123 with four (four inlined copies of the
    // interpreter)
    const unsigned nvec = total / 4;
    for (unsigned v = threadIdx.x; v < nvec; v += 512) {
        const bool two = v + 256 < nvec;
        const v4f x0 = __builtin_nontemporal_load((const v4f *)(in0 + cx.base + (size_t)v * 4));
        const v4f x1 = two ? __builtin_nontemporal_load((const v4f *)(in0 + cx.base + (size_t)(v + 256) * 4)) : v4f{0, 0, 0, 0};
        staged_run<4, LIGHT>(cx, v * 4, x0);
        if (two) staged_run<4, LIGHT>(cx, (v + 256) * 4, x1);
    }
    for (unsigned e = nvec * 4 + threadIdx.x; e < total; e += 256) staged_run<1, LIGHT>(cx, e, v4f{in0[cx.base + e], 0, 0, 0});
    __syncthreads();
    if (T > 1) {
        // rows of 49 ... 1024 floats: only a few rows fit a slab, so a group of T lanes (a power of two <= 64) folds each
        // row — lane t takes elements t, t + T, ... (consecutive lanes, consecutive LDS words), then an xor-shuffle tree
        const unsigned g = threadIdx.x / T, t = threadIdx.x & (T - 1), per_pass = 256u / T;
        for (unsigned r = g; r < rows; r += per_pass) {
            const float *p = slab + r * pitch;
            float a = np::dev::r_identity<SINK>();
            for (unsigned c = t; c < len; c += T) a = np::dev::r_combine<SINK>(a, p[c]);
            for (unsigned off = T >> 1; off > 0; off >>= 1) a = np::dev::r_combine<SINK>(a, __shfl_xor(a, (int)off, 64));
            if (t == 0) out[row0 + r] = np::dev::r_first_nan<SINK>(mean_div != 0.0f ? __fdiv_rn(a, mean_div) : a, p);   // (p[0]: the chain value in position 0)
        }
        return;
    }
    for (unsigned r = threadIdx.x; r < rows; r += 256) {
        const float *p = slab + r * pitch;
        float a0 = np::dev::r_identity<SINK>(), a1 = a0;
        unsigned c = 0;
        for (; c + 1 < len; c += 2) {
            a0 = np::dev::r_combine<SINK>(a0, p[c]);
            a1 = np::dev::r_combine<SINK>(a1, p[c + 1]);
        }
        if (c < len) a0 = np::dev::r_combine<SINK>(a0, p[c]);
        float v = np::dev::r_combine<SINK>(a0, a1);
        if (mean_div != 0.0f) v = __fdiv_rn(v, mean_div);
        out[row0 + r] = np::dev::r_first_nan<SINK>(v, p);   // (p[0]: the chain value in position 0)
    }
}

// very many short rows: the staged kernel (the same window as reduce_rows_staged in np_reduce.hip, which the op-by-op
// path takes for these shapes — the two must agree for the fused result to stay bit-identical)
static bool fused_rows_staged_shape(size_t rows, size_t cols) {
    return cols > 4 && cols <= 48 && rows * cols >= (size_t(8) << 20);
}
// Rows of 49 ... 512 floats of a large array that the lane-group kernel packs badly take the same staged kernel, a lane
// group folding each row of the slab: rows whose length is not a multiple of 4 (the lane-group kernel walks their last
// 1-3 elements in a pass of their own) and rows whose float4 slots do not fill the lane groups (100 floats = 25 slots on
// 16 lanes).  Measured, same box (profiles/r03/fused_mid_rows_ab.log): 2e6 x 50 2.5 -> 4.3 TB/s, 400000 x 250 2.9 -> 3.8,
// 800000 x 127 3.0 -> 3.9, 1e6 x 100 3.2 -> 3.6; well-packed rows stay where they are (64 / 256 / 1000 / 1024 floats:
// 3.8-4.8 TB/s there against 3.3-3.8 staged).
constexpr size_t kStagedMidMax = 512;
static bool fused_rows_staged_mid_shape(size_t rows, size_t cols) {
    if (cols <= 48 || cols > kStagedMidMax || rows < 4096 || rows * cols < (size_t(8) << 20)) return false;
    if (cols % 4 != 0) return true;
    const size_t slots = cols / 4;
    size_t L = 64;                                   // the lane-group kernel's choice (launch_rows)
    while (L > 4 && L >= slots) L >>= 1;
    const size_t trips = (slots + 2 * L - 1) / (2 * L);
    return (double)slots / (double)(trips * 2 * L) < 0.9;
}

// np_debug_chain_reduce_last_path: the NP_CHAIN_PATH_* bits of what the last np_fused_chain_reduce(_dev / _axis) call launched.
// A plain process global, cleared at the top of those entry points.
static unsigned g_chain_last_path = 0;

static bool fused_axis_shape_ok(size_t rows, size_t cols, int axis) {
    if (rows * cols >= (size_t(1) << 32)) return false;
    if (axis == 1 && (fused_rows_staged_shape(rows, cols) || fused_rows_staged_mid_shape(rows, cols))) return true;
    if (axis == 1) return cols >= 16 && (rows >= 128 || rows * cols >= (size_t(1) << 20));   // a lane group / wave / workgroup (or several) per row
    return rows >= 32 && cols / (cols % 4 == 0 ? 4 : 1) >= 32;   // first axis: a lane per column slot, waves interleaved over rows
}

// ------------------------------------------------------------------------------------------
// host side: one plan per chain, one launcher per kernel family
// ------------------------------------------------------------------------------------------

// What plan_chain makes of a caller's chain: the interpreter's descriptors, the same chain as np_fused_static.hip wants it, and
// what the launchers choose their kernels by.
struct ChainPlan {
    FusedArgs f;
    np::FusedStaticDesc sd;
    bool vec;           // float4 slots (dword-aligned accesses: pointers may start anywhere)
    bool broadcast;     // some operand is a row or a column vector
    bool light;         // every op is on the LIGHT interpreter's menu
    bool names_twice;   // a full array is named more than once: the KEEP variant (see fused_fetch)
    bool compiled;      // sd is filled in and may be on the menu of the compiled kernels (np::fused_static_covers decides)
};

// Checks the caller's arguments and fills the plan.  An empty result (rows * cols == 0) is NP_OK with the plan left alone,
// once the counts and pointers have been checked: the caller returns before it looks at the plan.
static int plan_chain(ChainPlan &p, const float *const *inputs, const int *input_kinds, int n_inputs, const np_fused_op *ops,
                      int n_ops, const float *out, size_t rows, size_t cols, int sink, int axis_mode) {
    const size_t n = rows * cols;
    if (n_inputs < 1 || n_inputs > FUSED_MAX_IN)
        return np::fail(NP_ERR_INVALID, "np_fused_chain: 1..%d inputs supported", FUSED_MAX_IN);
    if (n_ops < 0 || n_ops > FUSED_MAX_OPS)
        return np::fail(NP_ERR_INVALID, "np_fused_chain: at most %d ops per chain", FUSED_MAX_OPS);
    if (!inputs || !input_kinds || (n_ops > 0 && !ops) || !out)
        return np::fail(NP_ERR_INVALID, "np_fused_chain: null pointer");
    if (n == 0) return NP_OK;
    if (int rc = np::ensure_init()) return rc;
    const int variant = np::g_ew_variant;
    FusedArgs &f = p.f;
    f.n_ops = n_ops;
    p.vec = true;
    p.broadcast = false;
    for (int i = 0; i < n_inputs; ++i) {
        if (!inputs[i]) return np::fail(NP_ERR_INVALID, "np_fused_chain: null input %d", i);
        switch (input_kinds[i]) {
            case NP_FULL: break;
            // (float4 slots also when cols % 4 != 0, from 4 columns up: a slot then straddles at most two rows — fused_fetch)
            case NP_ROW:
            case NP_COL: p.vec = p.vec && (cols % 4 == 0 || (cols >= 4 && axis_mode < 0)); p.broadcast = true; break;
            case NP_SCALAR:
            case NP_HOST_SCALAR: break;
            default: return np::fail(NP_ERR_INVALID, "np_fused_chain: unknown operand kind %d", input_kinds[i]);
        }
    }
    if (input_kinds[0] != NP_FULL && input_kinds[0] != NP_HOST_SCALAR)
        return np::fail(NP_ERR_INVALID, "np_fused_chain: input 0 must be NP_FULL or NP_HOST_SCALAR");
    f.in0 = input_kinds[0] == NP_FULL ? inputs[0] : nullptr;
    f.scalar0 = input_kinds[0] == NP_FULL ? 0.0f : *inputs[0];
    f.first_prefetch = nullptr;
    f.first_prefetch_idx = FUSED_IDX_FULL;
    // does the chain name a full array more than once (as the operand of several steps, or input 0 again)?  Such a chain runs
    // on the interpreter's KEEP variant (see fused_fetch); np_elementwise_set_variant(7002): as every other chain (A/B)
    p.names_twice = false;
    if (variant != 7002) {
        for (int i = 0; i < n_inputs && !p.names_twice; ++i) {
            if (input_kinds[i] != NP_FULL) continue;
            int uses = (i == 0) ? 1 : 0;                       // input 0 is the chain's first value
            for (int k = 0; k < n_ops; ++k)
                if (ops[k].kind == NP_FUSED_BINARY && ops[k].operand >= 0 && ops[k].operand < n_inputs &&
                    input_kinds[ops[k].operand] == NP_FULL && inputs[ops[k].operand] == inputs[i])
                    ++uses;
            p.names_twice = uses >= 2;
        }
    }
    f.cols = p.broadcast ? cols : 0;
    f.sink = sink;
    f.ticket = nullptr;   // (launch_flat sets the two for a full reduction on a small grid)
    f.result = nullptr;
    f.div_m = f.div_s1 = f.div_s2 = 0;   // cols == 1: q = n
    if (p.broadcast && cols > 1 && cols <= 0xffffffffull) fast_div_magic(cols, f.div_m, f.div_s1, f.div_s2);
    FusedStep *last_stream = nullptr;
    p.light = true;
    // the same chain as np_fused_static.hip wants it, while it still may be one of the compiled ones: 1-3 steps on a full
    // input 0, float4-divisible rows under a broadcast, 32-bit indices, no AVX-body quirk other than multiply's (variant 7000: interpreter only)
    np::FusedStaticDesc &sd = p.sd;
    sd = np::FusedStaticDesc{};
    p.compiled = n_ops >= 1 && n_ops <= 3 && f.in0 && p.vec && (!p.broadcast || cols % 4 == 0) && n < (size_t(1) << 31) &&
                 variant != 7000 && (!p.names_twice || variant == 7001);   // (the compiled kernels stream every array: 7001 = A/B)
    sd.n_ops = n_ops;
    sd.in0 = f.in0;
    sd.bcast_cols = p.broadcast ? (unsigned)cols : 0u;
    sd.div_m = f.div_m;
    sd.div_s1 = f.div_s1;
    sd.div_s2 = f.div_s2;
    for (int k = 0; k < n_ops; ++k) {
        const np_fused_op &o = ops[k];
        FusedStep &d = f.ops[k];
        d = FusedStep{};
        d.kind = o.kind;
        d.op = o.op;
        d.p0 = o.p0;
        d.p1 = o.p1;
        if (o.kind == NP_FUSED_UNARY) {
            if (o.op < 0 || o.op >= NP_UNARY_OP_COUNT) return np::fail(NP_ERR_INVALID, "np_fused_chain: unknown unary op %d", o.op);
            if (o.op == NP_ROUND) d.p0 = powf(10.0f, o.p0);   // as np_unary
            p.light = p.light && fused_light_unary(o.op);
        } else if (o.kind == NP_FUSED_BINARY) {
            if (o.op < 0 || o.op >= NP_BINARY_OP_COUNT) return np::fail(NP_ERR_INVALID, "np_fused_chain: unknown binary op %d", o.op);
            if (o.operand < 0 || o.operand >= n_inputs) return np::fail(NP_ERR_INVALID, "np_fused_chain: operand index out of range");
            if (o.op == NP_POW && !o.swap && input_kinds[o.operand] == NP_HOST_SCALAR && *inputs[o.operand] == 2.0f) {
                // value ** 2 with a PHP number: np_binary computes it as x * x (its case NP_POW), so the chain does
                d.kind = NP_FUSED_UNARY;
                d.op = NP_UNARY_SQUARE;
                if (p.compiled) {
                    sd.kind[k] = d.kind;
                    sd.op[k] = d.op;           // not on the menu of np_fused_static.hip: the interpreter runs this chain
                }
                continue;
            }
            p.light = p.light && fused_light_binary(o.op);
            d.swap = o.swap;
            d.quirk = (o.flags & NP_QUIRK_AVX_BODY) ? 1 : 0;
            d.body_end = o.body_end;
            if (input_kinds[o.operand] == NP_HOST_SCALAR) {
                d.src_kind = FUSED_SRC_SCALAR;
                d.scalar = *inputs[o.operand];
            } else if (inputs[o.operand] == inputs[0] && input_kinds[o.operand] == NP_FULL && f.in0) {
                d.src_kind = FUSED_SRC_INPUT0;   // already in registers
            } else {
                d.src_kind = FUSED_SRC_STREAM;
                const int kind = input_kinds[o.operand];
                const int idx = kind == NP_FULL ? FUSED_IDX_FULL : kind == NP_ROW ? FUSED_IDX_ROW
                              : kind == NP_COL ? FUSED_IDX_COL : FUSED_IDX_ZERO;
                if (last_stream) {
                    last_stream->prefetch = inputs[o.operand];
                    last_stream->prefetch_idx = idx;
                } else {
                    f.first_prefetch = inputs[o.operand];
                    f.first_prefetch_idx = idx;
                }
                last_stream = &d;
            }
        } else {
            return np::fail(NP_ERR_INVALID, "np_fused_chain: unknown op kind %d", o.kind);
        }
        if (p.compiled) {
            sd.kind[k] = d.kind;
            sd.op[k] = d.op;
            sd.swap[k] = d.swap;
            sd.p0[k] = d.p0;
            sd.p1[k] = d.p1;
            sd.scalar[k] = d.scalar;
            sd.quirk[k] = 0;
            sd.body_end[k] = 0;
            if (d.kind == NP_FUSED_BINARY) {
                // the AVX-body quirk: the compiled kernels know multiply's (what the binding's chains carry); mod / equal are not on their menu
                if (d.quirk && binary_has_quirk(d.op)) {
                    if (d.op == NP_MULTIPLY) {
                        sd.quirk[k] = 1;
                        sd.body_end[k] = (unsigned)(d.body_end < n ? d.body_end : n);
                    } else {
                        p.compiled = false;
                    }
                }
                const int kind = input_kinds[o.operand];
                sd.operand[k] = d.src_kind == FUSED_SRC_SCALAR ? nullptr : d.src_kind == FUSED_SRC_INPUT0 ? f.in0 : inputs[o.operand];
                sd.idx[k] = d.src_kind != FUSED_SRC_STREAM ? 0 : kind == NP_FULL ? 0 : kind == NP_ROW ? 1 : kind == NP_COL ? 2 : 3;
            }
        }
    }
    return NP_OK;
}

// The tail of an axis reduction that was cut into chunks: `partial` holds outer x chunks x inner values, out receives the
// outer x inner results — divided by mean_div (!= 0) for a mean, which the chunked kernel could not do.
static int fold_axis_chunks(int sink, const float *partial, size_t outer, size_t chunks, size_t inner, float *out, float mean_div) {
    if (int rc = np_reduce_axis(sink, partial, outer, chunks, inner, out, 0)) return rc;
    if (mean_div != 0.0f) return np_binary(NP_DIVIDE, out, NP_FULL, &mean_div, NP_HOST_SCALAR, out, 1, outer * inner, 0, 0);
    return NP_OK;
}

// Last axis, staged (fused_chain_rows_staged_kernel): input 0 is a 16-byte aligned full array (fused_chain_impl has checked).
static int launch_rows_staged(const ChainPlan &p, float *out, size_t rows, size_t cols, float mean_div, bool staged_mid) {
    const unsigned pitch = (unsigned)cols | 1u;
    unsigned R = (8192u / pitch) / 256u * 256u, T = 1;
    if (R < 256) R = 256;
    if (staged_mid) {
        // ~32 KB of LDS per workgroup (4-5 resident per CU keep the streaming phase's loads in flight); R % 4 == 0 keeps
        // every slab's first element 16-byte aligned; T lanes per row, the largest power of two that R rows leave
        R = (8192u / pitch) / 4u * 4u;
        if (R < 4) R = 4;
        T = 64;
        while (T > 1 && T * R > 256u) T >>= 1;
    }
    const size_t blocks = (rows + R - 1) / R;
    if (blocks > 0x7fffffffu) return np::fail(NP_ERR_INVALID, "np_fused_chain_reduce_axis: too many rows");
    const size_t lds = (size_t)R * pitch * sizeof(float);
    const unsigned magic = (unsigned)((0x100000000ull + cols - 1) / cols);
    hipStream_t s = np::stream();
    // (the LIGHT interpreter — only ops whose bodies are a handful of instructions — where the chain allows: fewer
    // registers, more waves, more loads in flight; profiles/r03/fused_mid_rows_light_ab.log has the A/B against the full one)
#define NP_FRS(SINK_)                                                                                                                          \
    do {                                                                                                                                       \
        if (p.light)                                                                                                                           \
            fused_chain_rows_staged_kernel<SINK_, true><<<(unsigned)blocks, 256, lds, s>>>(p.f, out, rows, (unsigned)cols, R, magic, mean_div, T);  \
        else                                                                                                                                   \
            fused_chain_rows_staged_kernel<SINK_, false><<<(unsigned)blocks, 256, lds, s>>>(p.f, out, rows, (unsigned)cols, R, magic, mean_div, T); \
    } while (0)
    const int sink = p.f.sink;
    if (sink == NP_SUM) NP_FRS(NP_SUM);
    else if (sink == NP_PROD) NP_FRS(NP_PROD);
    else if (sink == NP_MIN) NP_FRS(NP_MIN);
    else NP_FRS(NP_MAX);
#undef NP_FRS
    NP_LAUNCH_CHECK("fused_chain_rows_staged_kernel");
    g_chain_last_path |= NP_CHAIN_PATH_ROWS_STAGED;
    return NP_OK;
}

// Last axis (fused_chain_rows_kernel, or np::fused_static_rows in the same lane-group geometry): a wave per row while rows
// are plentiful and short enough to leave a wave busy, else a workgroup.
static int launch_rows(const ChainPlan &p, float *out, size_t rows, size_t cols, float mean_div) {
    const int sink = p.f.sink;
    const bool block = cols >= 16384 || rows < (size_t)np::num_cus() * 16;
    // float4 slots also for rows of cols % 4 != 0 floats (dword-aligned accesses; the kernel takes the 1-3 leftover
    // elements of each row one per lane): such rows used to run one ELEMENT per slot
    const size_t slots = cols / 4;
    // The lane-group (wave) mode is bound by instruction issue, not by HBM (profiles/r03/rows_pmc.txt: SALU + VALU
    // activity scales with the time; rows of 64 floats issue 50 % more instructions per element than rows of 4000).
    // For LIGHT chains over rows of 128 ... 512 floats the interpreter's per-trip dispatch is amortised over 4 float4
    // slots per lane instead of 2, the lane group sized to ~4 slots per lane: 128 / 256 / 500 / 512 floats +7-12 %
    // (192, 384: neutral); shorter and longer rows lose 3-18 % to the extra registers and keep 2
    // (profiles/r03/fused_rows_u4_ab.log).
    const bool four = p.light && !block && cols >= 128 && cols <= 512;
    unsigned L = 64;                                   // ~2 (or ~4) slots per lane per trip
    while (L > 4 && (size_t)L * (four ? 2 : 1) >= slots) L >>= 1;
    size_t grid = block ? rows : (rows + 4 * (64 / L) - 1) / (4 * (64 / L));
    const size_t cap = (size_t)np::num_cus() * 16;
    if (grid > cap) grid = cap;
    // a handful of very long rows: several workgroups per row (>= 1024 slots each), partials folded afterwards
    size_t chunks = 1;
    if (block && rows < (size_t)np::num_cus() * 4) {
        chunks = ((size_t)np::num_cus() * 8 + rows - 1) / rows;
        const size_t max_chunks = slots / 1024 ? slots / 1024 : 1;
        if (chunks > max_chunks) chunks = max_chunks;
        if (chunks > 65535) chunks = 65535;
    }
    const size_t chunk_slots = (slots + chunks - 1) / chunks;
    chunks = (slots + chunk_slots - 1) / chunk_slots;
    np::Scratch partial;
    float *dst = out;
    if (chunks > 1) {
        if (int rc = partial.alloc(rows * chunks * sizeof(float))) return rc;
        dst = (float *)partial.ptr;
    }
    const float div = chunks > 1 ? 0.0f : mean_div;
    if (p.compiled && !block && chunks == 1 && cols % 4 == 0 && np::fused_static_covers(p.sd, sink, 1)) {
        // a compiled chain (np_fused_static.hip) in the same wave-per-row geometry: ~2 slots per lane per trip
        unsigned Lc = 64;
        while (Lc > 4 && (size_t)Lc >= slots) Lc >>= 1;
        size_t gridc = (rows + 4 * (64 / Lc) - 1) / (4 * (64 / Lc));
        if (gridc > cap) gridc = cap;
        g_chain_last_path |= NP_CHAIN_PATH_STATIC_ROWS;
        return np::fused_static_rows(p.sd, dst, rows, cols, Lc, div, (unsigned)gridc);
    }
    const dim3 grid2((unsigned)grid, (unsigned)chunks);
    hipStream_t s = np::stream();
#define NP_FR(LIGHT_, BLOCK_, UU_) \
    fused_chain_rows_kernel<4, LIGHT_, BLOCK_, uint32_t, UU_><<<grid2, 256, 0, s>>>(p.f, dst, (uint32_t)rows, (uint32_t)cols, L, (uint32_t)chunk_slots, div)
    if (four) NP_FR(true, false, 4);
    else if (p.light) { if (block) NP_FR(true, true, 2); else NP_FR(true, false, 2); }
    else { if (block) NP_FR(false, true, 2); else NP_FR(false, false, 2); }
#undef NP_FR
    NP_LAUNCH_CHECK("fused_chain_rows_kernel");
    g_chain_last_path |= NP_CHAIN_PATH_ROWS | (chunks > 1 ? NP_CHAIN_PATH_SPLIT : 0u);
    return chunks > 1 ? fold_axis_chunks(sink, dst, rows, chunks, 1, out, mean_div) : NP_OK;
}

// First axis (fused_chain_cols_kernel, or np::fused_static_cols in the same geometry): 64-slot column blocks, the rows cut
// into chunks so that every CU gets its workgroups.
static int launch_cols(const ChainPlan &p, float *out, size_t rows, size_t cols, float mean_div) {
    const int sink = p.f.sink, variant = np::g_ew_variant;
    const size_t g = cols % 4 == 0 ? 4 : 1;
    // np_elementwise_set_variant(12000 + k / 14000 + k): k workgroups per CU, compiled chains with 2 / 4 rows in flight
    // (7004: 4 rows at the default; A/B, tools/fused_static_ab.py)
    const bool wg_override = (variant / 1000 == 12 || variant / 1000 == 14) && variant % 1000;
    const size_t wg_per_cu = wg_override ? (size_t)(variant % 1000) : kColsWgPerCuDefault;
    const size_t col_blocks = (cols / g + 63) / 64;
    size_t chunks = ((size_t)np::num_cus() * wg_per_cu + col_blocks - 1) / col_blocks;
    const size_t max_chunks = rows / 32 ? rows / 32 : 1;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks > 65535) chunks = 65535;
    const size_t rows_per_chunk = (rows + chunks - 1) / chunks;
    chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
    np::Scratch partial;
    float *dst = out;
    if (chunks > 1) {
        if (int rc = partial.alloc(chunks * cols * sizeof(float))) return rc;
        dst = (float *)partial.ptr;
    }
    const float div = chunks > 1 ? 0.0f : mean_div;
    if (p.compiled && g == 4 && np::fused_static_covers(p.sd, sink, 0)) {
        // a compiled chain (np_fused_static.hip): the same geometry, straight-line code
        if (int rc = np::fused_static_cols(p.sd, dst, rows, cols, rows_per_chunk, div, (unsigned)col_blocks, (unsigned)chunks,
                                           variant == 7004 || variant / 1000 == 14 ? 4 : 2))
            return rc;
        g_chain_last_path |= NP_CHAIN_PATH_STATIC_COLS;
    } else {
        const dim3 grid((unsigned)col_blocks, (unsigned)chunks);
        hipStream_t s = np::stream();
#define NP_FCOL(G_, LIGHT_) fused_chain_cols_kernel<G_, LIGHT_, uint32_t><<<grid, 256, 0, s>>>(p.f, dst, (uint32_t)rows, (uint32_t)cols, (uint32_t)rows_per_chunk, div)
        // (two rows in flight per lane: 1, 3 and 4 were measured with tools/fused_cols_ab.py, profiles/r02/fused_cols_ab.log)
        if (g == 4) { if (p.light) NP_FCOL(4, true); else NP_FCOL(4, false); }
        else { if (p.light) NP_FCOL(1, true); else NP_FCOL(1, false); }
#undef NP_FCOL
        NP_LAUNCH_CHECK("fused_chain_cols_kernel");
        g_chain_last_path |= NP_CHAIN_PATH_COLS;
    }
    if (chunks > 1) g_chain_last_path |= NP_CHAIN_PATH_SPLIT;
    return chunks > 1 ? fold_axis_chunks(sink, dst, 1, chunks, cols, out, mean_div) : NP_OK;
}

// Flat (fused_chain_kernel, or np::fused_static_flat): out receives the n chain values, or — a sink — the full reduction.
static int launch_flat(ChainPlan &p, float *out, size_t n, size_t cols) {
    const int sink = p.f.sink;
    np::Scratch partials;
    float *result = out;
    unsigned reduce_blocks = 0;
    if (sink >= 0) {
        // grid-stride loop over a capped grid of few, long-lived workgroups (16 per CU), one workgroup-reduce + partial each
        const size_t want = (n / 4 + 255) / 256 + 1, cap = (size_t)np::num_cus() * 16;
        reduce_blocks = (unsigned)np::capped_grid(want, cap);
        if (int rc = partials.alloc(reduce_blocks * sizeof(float))) return rc;
        out = (float *)partials.ptr;
        if (reduce_blocks <= np::kFoldInKernelMaxBlocks) {
            p.f.ticket = np::next_ticket();
            p.f.result = result;
        }
    }
    // two float4 slots per lane for both interpreters: with the 8-instruction exp a wave's fixed cost (launch, kernarg
    // and descriptor loads, one scalar branch per step) weighs more than its registers — exp(X) + row 0.161 -> 0.139-0.143
    // ms, exp(a)*b+2 0.204-0.213 -> 0.197-0.203 (round 1, with the 14-instruction expf, one slot was ahead for the
    // light interpreter; profiles/r01/fused_ab.log, profiles/r02/fused_u_ab.log)
    const unsigned grid = reduce_blocks ? reduce_blocks : np::grid_for(p.vec ? n / 4 + 1 : n, 2, 0);
    if (p.compiled && np::fused_static_covers(p.sd, sink, -1)) {
        if (int rc = np::fused_static_flat(p.sd, out, n, sink, grid, p.f.ticket, p.f.result)) return rc;
        if (sink >= 0) g_chain_last_path |= NP_CHAIN_PATH_STATIC_FLAT;
    } else {
        const bool small = n < (size_t(1) << 31);
        hipStream_t s = np::stream();
#define NP_FC_I(VEC_, I_, RAGGED_, KEEP_)                                                                             \
    do {                                                                                                              \
        if (p.light) fused_chain_kernel<VEC_, 2, true, I_, RAGGED_, KEEP_><<<grid, 256, 0, s>>>(p.f, out, (I_)n);     \
        else fused_chain_kernel<VEC_, 2, false, I_, RAGGED_, KEEP_><<<grid, 256, 0, s>>>(p.f, out, (I_)n);            \
    } while (0)
#define NP_FC(VEC_, RAGGED_)                                   \
    do {                                                       \
        if (small) NP_FC_I(VEC_, uint32_t, RAGGED_, false);    \
        else NP_FC_I(VEC_, uint64_t, RAGGED_, false);          \
    } while (0)
        if (p.vec && p.broadcast && cols % 4 != 0) NP_FC(true, true);   // float4 slots that may straddle rows: the RAGGED variant
        else if (!p.vec) NP_FC(false, false);
        else if (p.names_twice && small && np::g_ew_variant != 7001) NP_FC_I(true, uint32_t, false, true);   // KEEP
        else NP_FC(true, false);
#undef NP_FC
#undef NP_FC_I
        NP_LAUNCH_CHECK("fused_chain_kernel");
        if (sink >= 0) g_chain_last_path |= NP_CHAIN_PATH_FLAT;
    }
    if (sink >= 0 && !p.f.ticket) return np::fold_partials(sink, (const float *)partials.ptr, reduce_blocks, result);
    return NP_OK;
}

// sink < 0: out receives rows*cols values; else out is a device float receiving the reduction — or,
// with axis_mode 1 / 0, rows / cols floats: the reduction over the last / first axis (mean_div != 0:
// divide the result by it)
static int fused_chain_impl(const float *const *inputs, const int *input_kinds, int n_inputs,
                            const np_fused_op *ops, int n_ops, float *out, size_t rows, size_t cols, int sink,
                            int axis_mode = -1, float mean_div = 0.0f) {
    ChainPlan p;
    if (int rc = plan_chain(p, inputs, input_kinds, n_inputs, ops, n_ops, out, rows, cols, sink, axis_mode)) return rc;
    const size_t n = rows * cols;
    if (n == 0) return NP_OK;
    if (axis_mode == 0) return launch_cols(p, out, rows, cols, mean_div);
    if (axis_mode != 1) return launch_flat(p, out, n, cols);
    // very many short rows, or mid-length rows that the lane groups pack badly: the staged kernel, which needs input 0 as a
    // 16-byte aligned full array
    const bool in0_aligned = p.f.in0 && ((uintptr_t)p.f.in0 & 15u) == 0;
    const bool staged_mid = fused_rows_staged_mid_shape(rows, cols) && in0_aligned;
    if (!fused_rows_staged_shape(rows, cols) && !staged_mid) return launch_rows(p, out, rows, cols, mean_div);
    if (in0_aligned) return launch_rows_staged(p, out, rows, cols, mean_div, staged_mid);
    // (anything else — a chain that starts from a scalar, a view at an odd offset — is materialised and handed to
    // np_reduce_axis like the shapes fused_axis_shape_ok turns away)
    np::Scratch tmp;
    if (int rc = tmp.alloc(n * sizeof(float))) return rc;
    if (int rc = fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, (float *)tmp.ptr, rows, cols, -1)) return rc;
    g_chain_last_path |= NP_CHAIN_PATH_TEMPORARY;
    return np_reduce_axis(mean_div != 0.0f ? NP_MEAN : sink, (const float *)tmp.ptr, rows, cols, 1, out, 0);
}

// What the three np_fused_chain_reduce* entry points check before anything else (`who`: the entry point's name; axis: 0 for the
// two full reductions), and the reset of np_debug_chain_reduce_last_path's record.
static int begin_chain_reduce(const char *who, const void *out, int reduce_op, size_t rows, size_t cols, int axis) {
    if (!out) return np::fail(NP_ERR_INVALID, "%s: null output", who);
    if (axis != 0 && axis != 1) return np::fail(NP_ERR_INVALID, "%s: axis %d of a rows x cols chain", who, axis);
    if (reduce_op != NP_SUM && reduce_op != NP_PROD && reduce_op != NP_MIN && reduce_op != NP_MAX && reduce_op != NP_MEAN)
        return np::fail(NP_ERR_INVALID, "%s: unknown reduction %d", who, reduce_op);
    if (rows * cols == 0) return np::fail(NP_ERR_INVALID, "%s: empty input", who);
    if (int rc = np::ensure_init()) return rc;
    g_chain_last_path = 0;
    return NP_OK;
}

extern "C" {

int np_fused_chain(const float *const *inputs, const int *input_kinds, int n_inputs,
                   const np_fused_op *ops, int n_ops, float *out, size_t rows, size_t cols) {
    return fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, out, rows, cols, -1);
}

int np_fused_chain_reduce(const float *const *inputs, const int *input_kinds, int n_inputs,
                          const np_fused_op *ops, int n_ops, int reduce_op, size_t rows, size_t cols,
                          float *host_out) {
    if (int rc = begin_chain_reduce("np_fused_chain_reduce", host_out, reduce_op, rows, cols, 0)) return rc;
    np::ResultCall call;
    float *slot = call.slot;
    if (!slot) return NP_ERR_ALLOC;
    const int sink = reduce_op == NP_MEAN ? NP_SUM : reduce_op;
    if (int rc = fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, slot, rows, cols, sink))
        return rc;
    if (int rc = call.wait()) return rc;
    const float v = slot[0];
    *host_out = reduce_op == NP_MEAN ? v / (float)(rows * cols) : v;
    return NP_OK;
}

// Same, the result left on the device (1 float): nothing waits, the call can be issued back to back like any kernel.
int np_fused_chain_reduce_dev(const float *const *inputs, const int *input_kinds, int n_inputs, const np_fused_op *ops, int n_ops,
                              int reduce_op, size_t rows, size_t cols, float *dev_out) {
    if (int rc = begin_chain_reduce("np_fused_chain_reduce_dev", dev_out, reduce_op, rows, cols, 0)) return rc;
    const int sink = reduce_op == NP_MEAN ? NP_SUM : reduce_op;
    if (int rc = fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, dev_out, rows, cols, sink)) return rc;
    if (reduce_op == NP_MEAN) {
        const float count = (float)(rows * cols);
        return np_binary(NP_DIVIDE, dev_out, NP_FULL, &count, NP_HOST_SCALAR, dev_out, 1, 1, 0, 0);
    }
    return NP_OK;
}

int np_fused_chain_reduce_axis(const float *const *inputs, const int *input_kinds, int n_inputs,
                               const np_fused_op *ops, int n_ops, int reduce_op, size_t rows, size_t cols, int axis,
                               float *out) {
    if (int rc = begin_chain_reduce("np_fused_chain_reduce_axis", out, reduce_op, rows, cols, axis)) return rc;
    const int sink = reduce_op == NP_MEAN ? NP_SUM : reduce_op;
    const float mean_div = reduce_op == NP_MEAN ? (float)(axis == 1 ? cols : rows) : 0.0f;
    if (fused_axis_shape_ok(rows, cols, axis))
        return fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, out, rows, cols, sink, axis, mean_div);
    // shapes the sink kernels would run mostly idle on: one fused pass into a temporary, then the
    // stand-alone axis reduction
    np::Scratch tmp;
    if (int rc = tmp.alloc(rows * cols * sizeof(float))) return rc;
    if (int rc = fused_chain_impl(inputs, input_kinds, n_inputs, ops, n_ops, (float *)tmp.ptr, rows, cols, -1)) return rc;
    g_chain_last_path |= NP_CHAIN_PATH_TEMPORARY;
    return axis == 1 ? np_reduce_axis(reduce_op, (const float *)tmp.ptr, rows, cols, 1, out, 0)
                     : np_reduce_axis(reduce_op, (const float *)tmp.ptr, 1, rows, cols, out, 0);
}

int np_debug_chain_reduce_last_path(unsigned *host_mask) {
    if (!host_mask) return np::fail(NP_ERR_INVALID, "np_debug_chain_reduce_last_path: null pointer");
    *host_mask = g_chain_last_path;
    return NP_OK;
}

}  // extern "C"
