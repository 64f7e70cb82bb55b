/*
 * np_hip.h — C ABI of the MI355X (gfx950) device back end for NumPower's fp32 hot path.
 *
 * This is the drop-in boundary: plain C, raw device pointers, size_t counts, int status.
 * It replaces the reference's inner (C <-> device back end) interface, i.e.
 *   - src/gpu_alloc.h:8-15            (vmalloc / vfree / vmemcpy* / vmemcheck / NDArray_VFLOAT)
 *   - src/ndmath/cuda/cuda_math.h:14-79 (cuda_*_float, cuda_float_*, cuda_sum/prod/min/max_float,
 *                                        cuda_fill_float, cuda_float_multiply_matrix_vector)
 *   - the cublasSgemm call in src/ndmath/linalg.c:55-71
 * Every entry point cites the reference symbol it stands in for.  All paths are relative to
 * the reference tree (NumPower/numpower @ 2024_08_07).
 *
 * Conventions
 *   - every function returns NP_OK (0) or a negative np_status; np_last_error() returns the
 *     message of the last failure on the calling thread.
 *   - pointers are DEVICE pointers unless the parameter name starts with `host`.
 *   - all arrays are contiguous C-order fp32 (the reference's only dtype on this path,
 *     src/types.h:5); the ops never look at strides (same contract as arithmetics.c).
 *   - work is enqueued on the library stream (np_get_stream/np_set_stream) and is asynchronous;
 *     np_sync(), np_memcpy_d2h() and the host_out reductions are the only blocking calls.
 *     (The reference synchronises after every launch, cuda_math.cu:1104-1109; results are
 *     identical, only the blocking point moves to the read-back.)
 *   - no torch / PHP / Zend types anywhere in this file.
 *   - threads: the library is one device + one stream per process, like the reference (PHP NTS, one
 *     request = one thread).  Calls may come from several host threads: the pool and the host-result
 *     entry points (np_reduce_all, np_all, np_count_mismatch, np_moments, np_weighted_sums,
 *     np_order_stat, np_fused_chain_reduce) serialise internally, np_last_error() is per thread.
 *     Every np_* call leaves the CALLING THREAD's current HIP device set to the library's device
 *     (np_init / np_set_device) — the effect cudaSetDevice has in the reference (numpower.c:633);
 *     a host that keeps another device current for its own work must re-select it afterwards.
 */
#ifndef NUMPOWER_AMD_NP_HIP_H
#define NUMPOWER_AMD_NP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum np_status {
    NP_OK = 0,
    NP_ERR_INVALID = -1,   /* bad argument (null pointer, unknown op, bad shape)          */
    NP_ERR_ALLOC = -2,     /* "device memory allocation failed" (gpu_alloc.c:15)          */
    NP_ERR_DEVICE = -3,    /* HIP runtime error (message in np_last_error)                */
    NP_ERR_NODEVICE = -4   /* "No GPU device available" (numpower.c:525)                  */
} np_status;

/* ---- runtime ------------------------------------------------------------------------ */

/* Select the device and create the library stream.  Replaces the implicit CUDA context
 * creation of the reference; np_set_device mirrors NDArray::setDevice -> cudaSetDevice
 * (numpower.c:615-635): it changes where NEW buffers and NEW work go and tears nothing down — the
 * device used before keeps its stream (work in flight completes), its cached blocks and its live
 * buffers, which can be freed at any time and used again after switching back. */
int np_init(int device);
int np_set_device(int device);
int np_device_count(int *host_count);
int np_sync(void);
/* Device errors.  A kernel whose device-side wait gives up (see "Device-side waits" below) raises a bit in the error word of
 * THE DEVICE IT RUNS ON.  From then on np_sync, np_memcpy_d2h, every host-result call and every np_comm_* call on that device
 * return NP_ERR_DEVICE — every time, whichever thread asks, so nobody's sync "eats" the error of the launch's owner — and the
 * same calls on another device (np_set_device) are not affected.  np_clear_device_error() is the acknowledgement: it waits
 * for everything the current device was given (all streams), puts the library's device-side bookkeeping back in order,
 * clears the word and hands back the bits that were up (1 = a stream-ordering wait of np_comm, 2 = a GEMM workgroup waiting
 * for its siblings' partial tiles; 0 = there was nothing to acknowledge).  Results produced between the failed launch and
 * the acknowledgement must be discarded.  While the device's communicator still has a transfer in flight that waits for a peer
 * (after 10 s of grace, or np_comm_set_wait_limit's seconds if fewer) it returns NP_ERR_DEVICE and clears nothing — the collective library's kernel does not end by itself
 * when a rank has died, and waiting for the whole device would never return: np_comm_destroy() first (it aborts the
 * communicator), then acknowledge.  (The reference ignores device errors altogether: cuda_math.cu never checks a launch.) */
int np_clear_device_error(unsigned *host_bits /* may be NULL */);
const char *np_last_error(void);
/* Library version string, e.g. "numpower_amd 0.1 gfx950". */
const char *np_version(void);

/* Stream plumbing: the library launches on one stream.  By default it owns a non-blocking
 * stream; a caller that already has one (e.g. torch's current stream, passed as the raw
 * hipStream_t) can hand it in.  Pass NULL to go back to the library-owned stream.
 * np_get_stream() returns a handle that is ordered behind every library call made BEFORE it.  While the library owns the stream,
 * large np_sgemm calls may run on a side stream of the library's (np_sgemm_overlap_stats below), and the handle is ordered behind
 * those only as of the moment it was fetched: a caller that enqueues its own work on it behind LATER library calls fetches it
 * again after those calls (or installs its own stream with np_set_stream, which turns the side stream off). */
int np_set_stream(void *hip_stream);
void *np_get_stream(void);

/* Event timing on the library stream (used by bench.py; hipEvent based). */
int np_timer_create(void **timer);
int np_timer_start(void *timer);
int np_timer_stop(void *timer);
int np_timer_elapsed_ms(void *timer, float *host_ms);   /* blocks until stop event done */
int np_timer_destroy(void *timer);

/* Launch-bound sequences as HIP graphs: capture what the library enqueues between begin and end,
 * replay it with one launch.  The reference synchronises after every kernel (cuda_math.cu:1104-1109),
 * so a chain of small ops costs a launch + sync each; a captured chain costs one graph launch.
 * Inside the captured region: no host-result calls (np_reduce_all, np_read_float, np_memcpy_*2h/h2d
 * ...), and warm the sequence up once first so the pool does not have to hipMalloc. */
int np_graph_begin(void);
int np_graph_end(void **graph_exec);
int np_graph_launch(void *graph_exec);
int np_graph_destroy(void *graph_exec);

/* ---- device-buffer layer (replaces src/gpu_alloc.c) ---------------------------------- */

/* vmalloc (gpu_alloc.c:11-17).  size_t instead of the reference's `unsigned int` (4 GiB cap).
 * Served from a caching sub-allocator (freed blocks are kept per size class and reused, so the
 * per-op result allocation of arithmetics.c:211-231 does not reach hipMalloc in steady state).
 * Bumps the live-allocation counter that np_live_allocs() reports. */
int np_malloc(void **dev_ptr, size_t bytes);
/* vfree (gpu_alloc.c:30-33). */
int np_free(void *dev_ptr);
/* vmemcheck (gpu_alloc.c:36-40): number of live np_malloc blocks (NDARRAY_VCHECK parity). */
long np_live_allocs(void);
/* Return all cached (free) blocks to the driver; returns bytes released through *host_bytes. */
int np_pool_trim(size_t *host_bytes);
/* Bytes currently held by the pool (live + cached). */
size_t np_pool_reserved_bytes(void);

/* vmemcpyh2d (gpu_alloc.c:25-27) / the cudaMemcpy H2D of NDArray_ToGPU (ndarray.c:1054). */
int np_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes);
/* The cudaMemcpy D2H of NDArray_ToCPU (ndarray.c:1090); blocks until the data is on the host. */
int np_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes);
/* vmemcpyd2d (gpu_alloc.c:20-22).  NOTE argument order here is (dst, src). */
int np_memcpy_d2d(void *dev_dst, const void *dev_src, size_t bytes);
/* cudaMemset(…, 0, …) of NDArray_Zeros (initializers.c:437-446). */
int np_memset0(void *dev_ptr, size_t bytes);
/* cuda_fill_float (cuda_math.cu:829,912). */
int np_fill(float *dev_ptr, float value, size_t n);
/* NDArray_VFLOAT / NDArray_VFLOATF_I (gpu_alloc.c:43-54): one float back to the host. */
int np_read_float(const float *dev_ptr, size_t index, float *host_out);

/* ---- binary elementwise with fused broadcast ------------------------------------------ */

/* Ops of NDArray_{Add,Subtract,Multiply,Divide,Mod,Pow}_Float (arithmetics.c:160-926) and
 * float_arctan2 (double_math.c:259-261, cuda_float_arctan2 cuda_math.cu:489,1224). */
typedef enum np_binary_op {
    NP_ADD = 0, NP_SUBTRACT = 1, NP_MULTIPLY = 2, NP_DIVIDE = 3, NP_MOD = 4, NP_POW = 5,
    NP_ARCTAN2 = 6,
    /* comparison ops of src/logic.c:67-670: 1.0f where true, 0.0f elsewhere.
     * Ordered compares (NaN -> 0).  EQUAL / NOT_EQUAL: the reference's AVX2 body compares exactly
     * (_CMP_EQ_OQ / _CMP_NEQ_OQ, logic.c:541,642), its scalar tail and its CUDA kernels use
     * |a-b| <= 1e-7 (logic.c:552,655, cuda_math.cu:243); NP_QUIRK_AVX_BODY selects the CPU
     * body/tail split, flags = 0 the tolerance form everywhere. */
    NP_EQUAL = 7, NP_NOT_EQUAL = 8, NP_GREATER = 9, NP_GREATER_EQUAL = 10, NP_LESS = 11,
    NP_LESS_EQUAL = 12,
    /* NDArray_Maximum / NDArray_Minimum (ndarray.c:853-931): fmaxf / fminf per element, with glibc's
     * rules — a NaN loses to a number, and when the operands compare equal (+0 / -0) the FIRST one is
     * returned.  (The reference refuses GPU arrays here and its CPU loop stops at numel(a).) */
    NP_MAXIMUM = 13, NP_MINIMUM = 14,
    NP_BINARY_OP_COUNT
} np_binary_op;

/* How an operand maps onto the rows x cols output.  These are exactly the patterns
 * NDArray_Broadcast materialises (ndarray.c:1196-1291); here they are index arithmetic
 * inside the kernel, no temporary is written. */
typedef enum np_operand_kind {
    NP_FULL = 0,    /* rows*cols elements                                                   */
    NP_SCALAR = 1,  /* 1 element        (0-d scalar expand, arithmetics.c:169-181)          */
    NP_ROW = 2,     /* cols elements    (1-D / 1xC -> every row, ndarray.c:1202-1223,1273)  */
    NP_COL = 3,     /* rows elements    (Rx1 -> every column, ndarray.c:1226-1272)          */
    NP_HOST_SCALAR = 4  /* like NP_SCALAR but the pointer is a HOST pointer to one float: the
                         * `$gpu_array + 2.0` case, where the 0-d operand lives on the CPU
                         * (arithmetics.c:163 exempts 0-d operands from the device check)      */
} np_operand_kind;

/* Result-visible CPU-path quirks of the reference that the kernel can reproduce so that GPU
 * results equal the reference's AVX2 CPU results element for element:
 *   NP_QUIRK_AVX_BODY  — elements with index < body_end behave like the AVX2 loop body,
 *                        the rest like the scalar tail:
 *       multiply: body turns every zero product into -0.0f (fix_negative_zero,
 *                 arithmetics.c:280-284,403), tail turns -0.0f into +0.0f (:410-412)
 *       mod:      body is a - floor(a/b)*b (arithmetics.c:794), tail is fmodf (:800)
 *   body_end is what the loop `for (i = 0; i < numel(a) - 7; i += 8)` covers, see
 *   np_avx_body_end().  flags = 0 gives plain IEEE multiply / C fmodf for every element
 *   (what the reference's own CUDA kernels do, cuda_math.cu:617-631). */
#define NP_QUIRK_AVX_BODY 1u

/* Number of leading elements covered by the reference's 8-wide AVX2 loop when the loop bound
 * is `numel_a - 7` (arithmetics.c:251): 0 if numel_a < 8, else 8*ceil((numel_a-7)/8). */
size_t np_avx_body_end(size_t numel_a);

/* out[r*cols + c] = a[...] op b[...];  replaces cuda_{add,subtract,multiply,divide,mod,pow}_float
 * (cuda_math.cu:1064-1109) + the Zeros/Fill/Broadcast temporaries in front of them. */
int np_binary(int op, const float *a, int a_kind, const float *b, int b_kind, float *out,
              size_t rows, size_t cols, unsigned flags, size_t body_end);

/* ---- unary elementwise ------------------------------------------------------------------ */

/* The float_* kernels of src/ndmath/double_math.c:9-265 (order follows double_math.h:7-44). */
typedef enum np_unary_op {
    NP_ABS = 0, NP_SQRT, NP_EXP, NP_EXP2, NP_EXPM1, NP_LOG, NP_LOG2, NP_LOG10, NP_LOG1P, NP_LOGB,
    NP_SIN, NP_COS, NP_TAN, NP_ARCSIN, NP_ARCCOS, NP_ARCTAN, NP_DEGREES, NP_RADIANS,
    NP_SINH, NP_COSH, NP_TANH, NP_ARCSINH, NP_ARCCOSH, NP_ARCTANH,
    NP_RINT, NP_FIX, NP_FLOOR, NP_CEIL, NP_TRUNC, NP_SINC, NP_NEGATE, NP_SIGN,
    NP_CLIP,        /* p0 = min, p1 = max            (float_clip, double_math.c:250-252)    */
    NP_ROUND,       /* p0 = decimals                 (float_round, double_math.c:254-257)   */
    NP_RSQRT,       /* 0x5f3759df bit hack + 1 Newton step (float_rsqrt, :111-126)          */
    NP_POSITIVE, NP_RECIPROCAL,
    NP_UNARY_OP_COUNT
} np_unary_op;

/* out[i] = f(in[i]); in == out is allowed.  Replaces NDArrayMathGPU_ElementWise{,1F,2F}
 * (cuda_math.cu:1532-1558) and the unary kernels behind them, without the preceding
 * NDArray_Copy (one 8 B/elem pass instead of copy + in-place = 16 B/elem). */
int np_unary(int op, const float *in, float *out, size_t n, float p0, float p1);

/* ---- fused elementwise chains --------------------------------------- */

/* One pass over HBM for a whole chain of elementwise ops:
 *     acc = inputs[0];  for each op:  acc = f(acc)            (NP_FUSED_UNARY,  op = np_unary_op)
 *                                     acc = acc (op) in[k]    (NP_FUSED_BINARY, op = np_binary_op,
 *                                     acc = in[k] (op) acc     operand = k, swap = 0 / 1)
 *     out[i] = acc
 * e.g. nd::exp($a) * $b + 2 costs 12 B/elem instead of 8 + 12 + 8 = 28 B/elem and two temporaries
 * (one allocation + one full round trip per PHP-level op in the reference, numpower.c:193-229).
 * Every step runs the same arithmetic as np_unary / np_binary (`value ** 2.0f` with a host scalar is
 * the product x * x in both), so the result is bit-identical to the unfused sequence; flags/body_end have the meaning they have in np_binary.  The result is
 * rows x cols; inputs[0] is NP_FULL (rows*cols elements) or NP_HOST_SCALAR, the other inputs have
 * any np_operand_kind: NP_FULL, NP_ROW (cols floats, added to every row), NP_COL (rows floats, one
 * per row), NP_SCALAR (device 0-d) or NP_HOST_SCALAR — the broadcast cases of ndarray.c:1196-1291
 * resolved by index arithmetic in the kernel, as in np_binary.  At most 6 inputs and 12 ops. */
typedef enum np_fused_kind { NP_FUSED_UNARY = 0, NP_FUSED_BINARY = 1 } np_fused_kind;
typedef struct np_fused_op {
    int kind;      /* np_fused_kind */
    int op;        /* np_unary_op or np_binary_op */
    int operand;   /* binary: index into inputs[] of the other operand */
    int swap;      /* binary: 0 = acc (op) operand, 1 = operand (op) acc */
    float p0, p1;  /* unary parameters (clip min/max, round decimals) */
    unsigned flags;     /* NP_QUIRK_AVX_BODY or 0 */
    size_t body_end;    /* see np_binary */
} np_fused_op;
int np_fused_chain(const float *const *inputs, const int *input_kinds, int n_inputs,
                   const np_fused_op *ops, int n_ops, float *out, size_t rows, size_t cols);
/* The same chain with a full reduction (np_reduce_op) as its last step: the chain value never goes
 * to memory — sum(exp(a) * b) reads 8 B/elem instead of writing 4 and reading 4 more.  Per-workgroup
 * partials + the deterministic second pass of np_reduce_all; NP_MEAN divides the sum by rows*cols
 * as NDArray::mean does (numpower.c:2659). */
int np_fused_chain_reduce(const float *const *inputs, const int *input_kinds, int n_inputs,
                          const np_fused_op *ops, int n_ops, int reduce_op, size_t rows, size_t cols,
                          float *host_out);
/* Same, the result left on the device (dev_out: 1 float) — no host round trip, so calls can be issued back to back. */
int np_fused_chain_reduce_dev(const float *const *inputs, const int *input_kinds, int n_inputs,
                              const np_fused_op *ops, int n_ops, int reduce_op, size_t rows, size_t cols,
                              float *dev_out);
/* ... and with a reduction over ONE axis of the rows x cols chain value as the last step: axis 1 (the
 * last axis) -> out[rows], axis 0 -> out[cols]; out is a DEVICE pointer.  sum(exp(X), 1), max(X - c, 1),
 * mean((X - mu) * (X - mu), 0) in one pass over X: 4 B/elem instead of 12.  Last axis: a wave (or, for
 * long or few rows, a workgroup) per row; first axis: a lane per 4-column slot, the workgroup's waves
 * interleaved over a chunk of rows, chunk partials folded by np_reduce_axis.  Shapes those kernels would
 * run mostly idle on (last axis: rows shorter than 16 floats, or fewer than 128 rows of a small array — a
 * handful of very long rows is cut into several workgroups per row; first axis: fewer than 32 rows or 32
 * column slots) take one fused pass into a temporary + np_reduce_axis instead.  Same combine rules as np_reduce_axis. */
int np_fused_chain_reduce_axis(const float *const *inputs, const int *input_kinds, int n_inputs,
                               const np_fused_op *ops, int n_ops, int reduce_op, size_t rows, size_t cols, int axis,
                               float *out);

/* ---- reductions -------------------------------------------------------------------------- */

typedef enum np_reduce_op {
    NP_SUM = 0, NP_PROD = 1, NP_MIN = 2, NP_MAX = 3, NP_MEAN = 4,
    NP_REDUCE_OP_COUNT
} np_reduce_op;
/* NP_MIN / NP_MAX and NaN, in np_reduce_all(_dev) and np_reduce_axis: the reference's loops (NDArray_Min / NDArray_Max,
 * ndarray.c:752-772, 939-959; the axis forms :818-839) start from position 0 of the reduced slice and replace on a strict
 * compare.  So the result is NaN exactly when position 0 of the slice is NaN; a NaN in any later position never wins; an
 * all-NaN slice gives NaN.  The kernels combine in a tree from +-inf and put the NaN of position 0 back where the final
 * value is written (r_first_nan, np_internal.h).  The np_fused_chain_reduce* calls follow the same rule with the chain's
 * value in position 0.
 * Sign of a zero extreme: where the extreme of a slice is zero and the slice holds both +0 and -0, the reference returns
 * whichever comes first; a tree order cannot promise that, and either zero may be returned.  Everything else about
 * min / max is bit-exact and independent of the launch geometry.
 * NP_SUM / NP_PROD / NP_MEAN propagate NaN and Inf as IEEE arithmetic does in any order. */

/* Full reduction to one host float.  Replaces cuda_sum_float / cuda_prod_float /
 * cuda_min_float / cuda_max_float (cuda_math.cu:921,934,1032,1016).  Deterministic two-pass
 * (wave64 shuffle + LDS, then one block over the per-block partials); no float atomics. */
int np_reduce_all(int op, const float *in, size_t n, float *host_out);
/* Same, result left on the device (1 float). */
int np_reduce_all_dev(int op, const float *in, size_t n, float *dev_out);

/* Statistics (src/ndmath/statistics.c:88-154).  The reference composes these
 * from Sum / Subtract / Abs / Pow with a full-size temporary per step (32 B/elem for variance);
 * here the array is read ONCE (4 B/elem): per-lane (count, mean, M2) merged pairwise in a fixed order
 * (Chan's formula; means carried as anchor + offset, so the result is as accurate as the two-pass form
 * for data with a large mean and a small spread).  host_m2 = sum (x - mean)^2:
 *   variance = m2 / n (NDArray_Variance), std = sqrtf(m2 / n) (NDArray_Std).  n >= 1. */
int np_moments(const float *in, size_t n, float *host_mean, float *host_m2);
/* Same, results left on the device: dev_out[0] = mean, dev_out[1] = m2 (2 floats). */
int np_moments_dev(const float *in, size_t n, float *dev_out);
/* NDArray_Average with weights (statistics.c:131-154): sum(a*w) and sum(w) from one kernel that reads
 * a and w once each (8 B/elem; no a*w temporary, products rounded before they are added as the
 * reference's Multiply-then-Sum). */
int np_weighted_sums(const float *a, const float *w, size_t n, float *host_sum_aw, float *host_sum_w);

/* argmax (is_max != 0) / argmin along the middle axis of outer x axis_len x inner; out receives
 * outer*inner indices AS FLOATS, like the reference (float_argmax / float_argmin,
 * src/ndmath/calculation.c:9-72: first occurrence wins; argmax: a NaN in position 0 is maximal,
 * later NaNs are never selected; argmin: the first NaN wins).  The reference rejects GPU arrays
 * ("GPU not supported.", calculation.c:75-78). */
int np_argreduce(int is_max, const float *in, size_t outer, size_t axis_len, size_t inner, float *out);

/* NDArray_All (logic.c:25-58): *host_out = 1 if every element is non-zero, else 0.
 * flags = NP_QUIRK_AVX_BODY reproduces what the reference's CPU code actually computes: its AVX2
 * body tests `movemask != 0x0F` on an 8-lane mask (logic.c:36-39), i.e. a full 8-element block
 * passes only if elements 0-3 are non-zero (and not NaN) and elements 4-7 ARE zero or NaN; the
 * scalar tail (`== 0.0`) is the only part that means "all non-zero".  flags = 0 gives the
 * intended meaning for every element. */
int np_all(const float *in, size_t n, unsigned flags, int *host_out);

/* Two-array predicates reduced to one flag (one streaming pass, 8 B/elem, no mask temporary):
 *   NP_MISMATCH_EXACT     *host_any = 1 if a[i] != b[i] for some i     compare_ndarrays, logic.c:686-690
 *                         (NaN != NaN counts, as in the reference's C loop; its CUDA path,
 *                         cuda_equal_float, is a launch + D2H of a flag per call)
 *   NP_MISMATCH_ALLCLOSE  *host_any = 1 if |a[i]-b[i]| > atol + rtol*|b[i]| for some i
 *                         float_allclose, logic.c:719-738 (a NaN on either side compares false,
 *                         i.e. "close", exactly as the reference's expression does; the reference
 *                         rejects GPU arrays: "`allclose` is not compatible with GPU operations.") */
typedef enum np_mismatch_mode { NP_MISMATCH_EXACT = 0, NP_MISMATCH_ALLCLOSE = 1 } np_mismatch_mode;
int np_count_mismatch(int mode, const float *a, const float *b, size_t n, float rtol, float atol,
                      int *host_any);

/* Order statistics: host_out2[0] = the k-th smallest element (k counted from 0), host_out2[1] = the
 * (k+1)-th (= the k-th again when k is the last rank).  Exact, by a three-pass radix select (12 B/elem
 * of reads, no sort, no copy) — replaces the copy + qsort() of calculate_median
 * (src/ndmath/arithmetics.c:111-138) and calculate_quantile (src/ndmath/statistics.c:14-50), whose
 * results depend on exactly these two values.  Ordering: IEEE total order on the bits (-0.0 before
 * +0.0, which the reference's comparator calls equal; NaNs at the ends by sign — the comparator is
 * inconsistent for NaNs, so the reference's own result is unspecified there).
 * np_order_stat_dev leaves the two floats in device memory (no synchronisation). */
int np_order_stat(const float *in, size_t n, size_t k, float *host_out2);
int np_order_stat_dev(const float *in, size_t n, size_t k, float *dev_out2);

/* Reduce the middle axis of a contiguous array viewed as outer x axis_len x inner; out has
 * outer*inner elements.  Replaces the host-side recursion reduce()/_reduce()/apply_reduce()
 * (ndarray.c:523-578,394-429,358-368), which issues one Add_Float + alloc + D2D copy + free
 * per slice, by one (or two) kernels.
 * flags: NP_QUIRK_AVX_BODY with NP_PROD reproduces the sign the reference's repeated
 * NDArray_Multiply_Float leaves on ZERO results (arithmetics.c:403,410-412): -0.0f for inner
 * index < np_avx_body_end(inner), +0.0f after it; pass it only when the reduced slices are
 * at least 1-D (0-d slices take the plain a*b short cut, arithmetics.c:302-316). */
int np_reduce_axis(int op, const float *in, size_t outer, size_t axis_len, size_t inner,
                   float *out, unsigned flags);
/* Scratch the axis reduction may need for its partials, in bytes (0 if none); the library
 * allocates it from the pool itself — exported so callers can size memory budgets. */
size_t np_reduce_axis_workspace(size_t outer, size_t axis_len, size_t inner);

/* ---- matmul --------------------------------------------------------------------------------- */

/* C[MxN] = A[MxK] . B[KxN], row-major, alpha = 1, beta = 0, exact fp32 (v_mfma_f32_32x32x2_f32).
 * Replaces cblas_sgemm(RowMajor,N,N,…) / cublasSgemm in NDArray_FMatmul (linalg.c:44-82). */
int np_sgemm(size_t M, size_t N, size_t K, const float *A, const float *B, float *C);
/* batch independent products; matrix b of X starts at X + b*stride_x (strides in elements).
 * The reference has no batched entry point (linalg.c:239-242 rejects ndim > 2); this is the
 * loop-of-2-D-calls collapsed into one launch (BASELINE config 5). */
int np_sgemm_strided_batched(size_t batch, size_t M, size_t N, size_t K,
                             const float *A, size_t stride_a, const float *B, size_t stride_b,
                             float *C, size_t stride_c);
/* The same for `count` matrices that are a PIECE of a batch of `whole` (a caller that pipelines a batch piece by piece,
 * numpower_amd/parallel.py): the piece runs the kernel configuration np_sgemm_strided_batched would pick for the whole
 * batch, so that the pieces together are bit-identical to the one call — a piece of one matrix would otherwise go to
 * the single-product planner (split-K, stream-K ...), which sums in a different order.  whole >= count. */
int np_sgemm_strided_batched_piece(size_t count, size_t whole, size_t M, size_t N, size_t K,
                                   const float *A, size_t stride_a, const float *B, size_t stride_b,
                                   float *C, size_t stride_c);
/* Consecutive large np_sgemm calls (one launch of the LDS-DMA kernel each, from 4e9 flop) that do not touch each other's operands
 * run alternately on the library stream and on a side stream the library owns, so that one launch's workgroups start while
 * the previous launch is still storing C.  Every other entry point first orders the library stream behind the side stream — as
 * does np_get_stream, at the moment it is called (see there for a handle that is kept) — and products that share bytes (C of one is an operand or
 * the C of the next, or the other way round) are never reordered.  Off under a caller's stream (np_set_stream) and inside
 * np_graph_begin .. np_graph_end; NP_SGEMM_OVERLAP=0 in the environment turns it off when the library is loaded.
 * out[0]: launches that went to the side stream, out[1]: launches on the library stream next to one on the side stream,
 * out[2]: launches of that size ordered behind everything (the first of a run, a shared operand, other work in between). */
int np_sgemm_overlap_stats(unsigned long long out[3]);
/* y[M] = A[MxN] . x[N]; replaces cblas_sgemv / matrixVectorMultiplyFloatKernel
 * (linalg.c:367-386, cuda_math.cu:228,1417). */
int np_sgemv(size_t M, size_t N, const float *A, const float *x, float *y);
/* out[M x N] = a (M) outer b (N), row-major: NDArray_Outer (linalg.c:724-751; cblas_sger on a zeroed
 * matrix / cuda_calculate_outer_product), i.e. out[i][j] = 0 + a[i]*b[j] (zero products are +0.0). */
int np_outer(const float *a, size_t M, const float *b, size_t N, float *out);

/* ---- layout ---------------------------------------------------------- */

/* out[b][c][r] = in[b][r][c] for batch matrices of rows x cols (contiguous); in != out.
 * Replaces cuda_float_transpose / transposeCoalesced (cuda_math.cu:136-150,1288-1294: fixed 16x16
 * grid, only correct up to 256 x 256) with a 64 x 64 LDS-tiled transpose, any size. */
int np_transpose2d(const float *in, float *out, size_t batch, size_t rows, size_t cols);
/* General axis permutation into a new contiguous buffer: out.shape[i] = shape[perm[i]]
 * (NDArray_Transpose + NDArray_ToContiguous, manipulation.c:68-130,381-421).  ndim <= 8;
 * shape/perm are host arrays.  Errors: "axes don't match array", "repeated axis in transpose". */
int np_permute(const float *in, float *out, int ndim, const int *host_shape, const int *host_perm);
/* Gather a strided view into a contiguous buffer: out[i0]...[ik] = in[sum i_d * strides[d]]
 * (strides in ELEMENTS, may be negative or zero).  One launch instead of NDArray_ToContiguous's
 * one 4-byte D2D memcpy per element (manipulation.c:381-421); also what NDArray_Diagonal
 * (indexing.c:21-48: one memcpy per diagonal element) and multi-index NDArray_Slice
 * (manipulation.c:193-283) reduce to. */
int np_strided_copy(const float *in, float *out, int ndim, const int *host_shape, const long long *host_strides);
/* Pitched 2-D copy: rows x width floats, consecutive rows dst_pitch / src_pitch floats apart (both
 * >= width).  One launch per input of NDArray_Concatenate along an inner axis (manipulation.c:894-997,
 * where NDArray_AssignArray copies element by element through the sliding view). */
int np_copy2d(float *dst, size_t dst_pitch, const float *src, size_t src_pitch, size_t width, size_t rows);

/* ---- dense LU factorization (np_lu.hip; DESIGN.md "LU") ----------------------------------------
 * All matrices are n x n fp32 on the device; every call runs on the library stream and takes its
 * scratch from the caching pool.  Results are bit-identical from run to run.
 * np_getrf:   LAPACK sgetrf on the COLUMN-MAJOR a, in place: a = P^T L U, ipiv[n] = 0-based pivot rows
 *             (device int32), *info (device int) = 1 + the first exactly-zero pivot, else 0.  A row-major
 *             buffer is factored as its transpose, which is how the reference's LAPACK calls see it.
 * np_getrs:   solves A X = B with np_getrf's factors; b is column-major n x nrhs, overwritten by X.
 * np_det:     det of the buffer as LAPACK sees it (= det(a)): the diagonal of U multiplied in index order
 *             in fp32, the pivot parity's sign; exactly 0.0f when info > 0.  *out_dev is device memory.
 * np_inverse: out = a^-1 (row-major; getrf on the buffer as-is, getrs against I).  *info_host (host)
 *             > 0: a is singular and out is left undefined.  Blocks until info is known.
 * np_solve:   x (n x nrhs, row-major) with a x = b (b row-major n x nrhs).  *info_host as np_inverse.
 * np_lu:      row-major p, l, u with p a = l u: partial pivoting by |value| on the rows of a, l unit-lower
 *             with |l| <= 1, u upper, p a permutation matrix.
 * n == 0 does nothing (np_det writes 1); null pointers are NP_ERR_INVALID; the blocked path takes
 * n <= 65536. */
int np_getrf(float *a, size_t n, int *ipiv, int *info);
int np_getrs(const float *lu, const int *ipiv, size_t n, size_t nrhs, float *b);
int np_det(const float *a, size_t n, float *out_dev);
int np_inverse(const float *a, size_t n, float *out, int *info_host);
int np_solve(const float *a, const float *b, size_t n, size_t nrhs, float *x, int *info_host);
int np_lu(const float *a, size_t n, float *p, float *l, float *u);

/* ---- dense Cholesky factorization (np_cholesky.hip; DESIGN.md "Cholesky") ------------------------
 * a = L L^T for a symmetric positive definite n x n fp32 matrix, ROW-MAJOR, with LAPACK's spotrf('L')
 * semantics: only the lower triangle of a (diagonal included) is read, whatever the strict upper triangle
 * holds.  info = 1 + the first column whose pivot a_jj - sum_k l_jk^2 is not greater than zero (or is NaN),
 * else 0; what the factor holds from that column on is unspecified.  Library stream, pool scratch,
 * bit-identical from run to run.
 * np_potrf:    in place: the lower triangle of a becomes L, the strict upper triangle of a is left exactly
 *              as it was; *info is a device int.
 * np_cholesky: out = L with the strict upper triangle +0.0f, a untouched (out must not overlap a);
 *              *info_host (host).  Blocks until info is known.
 * n == 0 does nothing and reports info = 0; null pointers are NP_ERR_INVALID; n <= 65536. */
int np_potrf(float *a, size_t n, int *info);
int np_cholesky(const float *a, size_t n, float *out, int *info_host);

/* ---- singular value decomposition (np_jacobi.hip; DESIGN.md "SVD") --------------------------------
 * One-sided (Hestenes) Jacobi, blocked: replaces cuda_svd_float (cuda_math.cu:947, cuSOLVER's gesvdj) behind NDArray_SVD.
 * a: m x n fp32, ROW-MAJOR, untouched.  k = min(m, n).
 * u: m x k row-major, s: k, vt: k x n row-major, with  a = u . diag(s) . vt,  s >= 0 and non-increasing.
 * *info_host (host int): 0 = converged, > 0 = the sweep cap (60) was reached — the value: how many column pairs were still
 * above the tolerance (|g_pq| <= 4 eps sqrt(g_pp g_qq)) in the last sweep, clipped to INT_MAX; the factors are returned
 * either way and still reconstruct a.  Blocks until info is known.
 * np_svdvals: singular values only — no V accumulation, no U normalisation; the same s bit for bit as np_svd.
 * Library stream, scratch from the caching pool, no float atomics, one fixed rotation order: bit-identical from run to run.
 * Scratch: with r = min(m, n) rounded up to 64 and c = max(m, n) rounded up to 32, the work matrix r x c, for np_svd the
 * accumulated r x r rotations and one k x max(m, n) staging matrix (np_svdvals: that one only for m >= n), and per pair of
 * 32-row blocks (r / 64 of them) up to 17 matrices of 64 x 64 floats.
 * Fine print:
 *   - signs are not normalised (an SVD is unique only up to the sign of each pair u_i, v_i); they are deterministic.
 *   - for m >= n the columns of a are rotated: vt is a product of rotations and always orthonormal; column i of u is the
 *     rotated column divided by s_i.  If s_i is exactly 0 that column of u is written as +0.0f; for a negligible s_i
 *     (<= max(m, n) eps s_0) it is normalised noise and need not be orthogonal to the others.  For m < n the transposed
 *     problem is solved and the roles of u and vt swap.  (cuSOLVER's gesvdj has the same property; LAPACK completes the
 *     basis.  This library does not.)
 *   - non-finite input: the call returns (the sweep loop is bounded by the cap, nothing spins on a NaN compare), s contains
 *     at least one NaN, nothing else is promised.
 *   - min(m, n) <= 64 with a row length that fits LDS (64 x 557, 5 x 7000 ...) is ONE launch of one workgroup (unblocked, rotations
 *     applied in fp32); everything else is the blocked form.  np_svd and np_svdvals of one shape always take the same path.
 *   - tested up to 4097 x 4097.  The sweep count grows with min(m, n) (26 at 4096 x 4096 on a well-conditioned dense matrix), so
 *     for much larger matrices info > 0 at the cap may be the normal outcome; the factors still reconstruct a then.
 * m == 0 || n == 0 does nothing and reports 0; null pointers are NP_ERR_INVALID; m, n <= 65536.  Outputs must not overlap a. */
int np_svd(const float *a, size_t m, size_t n, float *u, float *s, float *vt, int *info_host);
int np_svdvals(const float *a, size_t m, size_t n, float *s, int *info_host);

/* ---- symmetric eigensolver (np_jacobi.hip; DESIGN.md "eigh") --------------------------------------
 * Two-sided (classical) Jacobi, blocked: what cuda_matrix_eig_float (cuda_math.cu:1645, cuSOLVER's Ssyevd) would have
 * done behind NDArray_Eig, which the reference refuses for GPU arrays (linalg.c:826-833).
 * a: n x n fp32, ROW-MAJOR, untouched.  LAPACK ssyevd('L') semantics, the rule np_potrf documents: only the lower triangle
 * of a (diagonal included, a[i][j] with j <= i) is read, whatever the strict upper triangle holds.
 * w: the n eigenvalues ascending, ties kept in the order of their diagonal position (-0.0f and +0.0f tie).
 * v: n x n row-major, column j is the eigenvector of w[j].  The columns are the accumulated rotations and are not
 * renormalised.  Sign: the component of largest magnitude in each column, the first such in index order, is positive, so the
 * signs are deterministic and comparable with closed forms.
 * np_eigvalsh: eigenvalues only — no vector accumulation; the same w bit for bit as np_eigh.
 * *info_host (host int): 0 = converged, > 0 = the sweep cap (60) was reached — the value: how many off-diagonal pairs were
 * still above the tolerance in the last sweep, clipped to INT_MAX; the results are returned either way.  Blocks until info
 * is known.
 * A pair (p, q) rotates while |w_pq| > eps * scale, scale = the largest |entry| of the lower triangle of a, fixed at the start
 * of the call (diagonals may be zero or negative, so no rule built on w_pp w_qq can serve).
 * Library stream, scratch from the caching pool, no float atomics, one fixed rotation order: bit-identical from run to run.
 * Scratch: with r = n rounded up to 64, the work matrix r x r, for np_eigh the accumulated r x r rotations and one n x n
 * staging matrix, and per pair of 32-row blocks (r / 64 of them) one matrix of 64 x 64 floats.
 * Fine print:
 *   - accuracy class: this is a Jacobi iteration in fp32 storage like the shipped SVD, not LAPACK's ssyevd: residual,
 *     orthogonality and eigenvalue errors grow like a small multiple of n eps relative to ||a||_2 (tests/test_gpu_eigh.py
 *     holds them to the bound a plain fp32 Jacobi emulation reaches), where LAPACK stays near eps.  Eigenvalues are accurate
 *     relative to ||a||_2, not each to its own magnitude.
 *   - non-finite input: the call returns (the sweep loop is bounded by the cap, nothing spins on a NaN compare) and every
 *     entry of w is NaN; nothing else is promised.
 *   - n <= 64 is ONE launch of one workgroup (the whole matrix in LDS, in fp64); everything else is the blocked form.
 *     np_eigh and np_eigvalsh of one n always take the same path.
 *   - not a general eigensolver: a non-symmetric a is answered from its lower triangle.  (The NDArray layer checks the
 *     symmetry first, np_symmetry_mismatch, and refuses.)
 *   - speed: 185 ms at n = 1024, 397 ms at 2048, 939 ms at 4096 on a dense random matrix (12 - 13 sweeps), 0.75 - 0.90 of np_svd's
 *     time on the same matrix.  The crossover with the host's LAPACK (numpy's fp32 eigh) is near n = 2000: below it the host is
 *     faster (89 ms at 1024), above it the device (0.34 of the host's time at 4096).  profiles/linalg/eigh_sweep.log.
 * n == 0 does nothing and reports 0; null pointers are NP_ERR_INVALID; n <= 65536.  Outputs must not overlap a.
 * np_symmetry_mismatch: *host_any (host int) = 1 when some i > j has a[i][j] != a[j][i], two NaNs counting as equal, else 0.
 * Blocks until it is known. */
int np_eigh(const float *a, size_t n, float *w, float *v, int *info_host);
int np_eigvalsh(const float *a, size_t n, float *w, int *info_host);
int np_symmetry_mismatch(const float *a, size_t n, int *host_any);

/* ---- Householder QR and least squares (np_qr.hip; DESIGN.md "qr") -----------------------------------
 * Blocked compact-WY Householder QR of a: m x n fp32, ROW-MAJOR, m >= n; what the reference refuses for GPU arrays
 * ("ndarray::qr not implemented for GPU", "ndarray::lstsq not implemented for GPU", linalg.c:850, 910).
 * Convention: LAPACK's sgeqr2 / slarfg.  H_j = I - tau_j v_j v_j^T with v_j[j] = 1.  With alpha = a_jj and x the part of
 * column j below the diagonal: beta = -sign(alpha) ||(alpha, x)||_2 with sign(+0) = sign(-0) = +, tau_j = (beta - alpha) / beta,
 * v_j = x / (alpha - beta), R_jj = beta.  A zero sub-column (x == 0 exactly) gives tau_j = 0, H_j = I and R_jj = alpha.
 * R's diagonal is not normalised: it is not made positive, and Q's columns carry the matching signs.
 * np_geqrf: in place.  R on and above the diagonal, v_j below it (its leading 1 implied), tau: n device floats.
 * np_qr: the reduced factorization, numpy.linalg.qr's mode='reduced': q (m x n) = H_0 ... H_{n-1} I[:, :n], r (n x n) with a
 * strict lower triangle of exact +0.0f.  a is untouched; q and r must not overlap a.
 *   Different from the reference's CPU qr on purpose: its NDArray_Qr calls sgeqrf and never sorgqr, and hands the packed
 *   reflectors back as "Q".  The device qr returns the mathematically defined Q (Q^T Q = I, Q R = a).
 * np_lstsq: x (n x nrhs) minimises ||a x - b||_2 for b m x nrhs: C = Q^T b by applying the reflectors in order, then
 * x = R^-1 C[:n] by back-substitution.  *info_host (host int): 0, or j + 1 for the first j with R_jj == 0 exactly; then x
 * is not written (LAPACK sgels' rule: a does not have full rank).  Blocks until info is known.  a and b are untouched.
 * m < n is refused by all three with NP_ERR_INVALID before any device work (the reference's NDArray_Qr requires m >= n as well;
 * the minimum-norm branch of sgels for m < n is out of scope).  Null pointers are NP_ERR_INVALID.  n == 0 (and nrhs == 0) does nothing.
 * Limits: m <= 16777216, n <= 65536, nrhs < 2^31; larger sizes are refused, not truncated.
 * The panel (one workgroup per kNB = 64 columns) accumulates the column norm and every v . x inner product in fp64 and rounds once:
 * the factorization is invariant under power-of-two scaling of a (Q bit for bit, R times the power) and entries of 2^+-62
 * neither overflow nor flush in the squares.  The trailing updates, the formation of Q and Q^T b run on the MFMA GEMM.
 * Non-finite input: there is no iteration, the call finishes with NP_OK and NaN / Inf propagate; np_lstsq reports info only
 * for an exact zero on R's diagonal.
 * Scratch (caching pool, released on every path): V (m x 64), V^T (64 x m), two 64 x max(n, nrhs) matrices, 8192 floats per panel
 * for T and T^T; np_qr and np_lstsq add a copy of a (np_lstsq also one of b).
 * Library stream, no float atomics, every fold in a fixed order: bit-identical from run to run.
 * Speed and the crossover with the host's LAPACK: DESIGN.md §3.13, profiles/linalg/qr_sweep.log. */
int np_geqrf(float *a, size_t m, size_t n, float *tau);
int np_qr(const float *a, size_t m, size_t n, float *q, float *r);
int np_lstsq(const float *a, const float *b, size_t m, size_t n, size_t nrhs, float *x, int *info_host);

/* ---- 2-D correlation and convolution (np_signal.hip; DESIGN.md "convolve2d") ------------------------
 * scipy.signal.correlate2d(a, b, mode, boundary, fillvalue) for real fp32 arrays, ROW-MAJOR, and with flip != 0
 * scipy.signal.convolve2d: what the loop of the reference's signal.c:152-207 computes, which the reference refuses for
 * GPU arrays (signal.c:219-221).  mode and boundary take the reference's values (signal.h).
 * np_correlate2d_shape: the result's extents, no device needed.  'full' ah + bh - 1, 'same' those of a (whichever operand
 *   is larger), 'valid' |ah - bh| + 1, where one operand must be at least as large as the other in every dimension.
 * np_correlate2d: the whole SciPy call.  In 'valid' mode an a that does not cover b changes places with it, and the
 *   correlation computed that way is stored reversed along both axes, as SciPy returns it.  out: contiguous, of the extents
 *   _shape reports; it must not overlap a or b.  fill_value is what lies outside a under NP_CONV_FILL.
 * Fine print:
 *   - every tap is multiplied and added: no coefficient and no fill cell is skipped because it is zero, so an Inf under a
 *     0 tap gives NaN, as in SciPy.
 *   - fixed order: each element starts from +0.0f and adds its taps with one fp32 fmaf each, in the order np_signal.hip
 *     documents (footprint columns left to right, each top to bottom; windows beyond 15 x 15 in chunks of 16 x 16 taps,
 *     chunks in row-major order).  The order is stated over the window as it lies on the image, so a convolution and the
 *     correlation with the reversed window agree bit for bit; it does not depend on where the element sits in a tile, and
 *     the result is bit-identical from run to run.
 *   - boundary once per cell: fill / wrap / symm, also many image lengths away, is resolved when a cell of the image's
 *     surroundings is staged, never per tap.
 *   - windows up to 15 x 15 are staged once with their whole halo; larger ones of any size, larger than the image
 *     included, run through LDS in chunks with the accumulators in registers.
 * All extents >= 1.  NP_ERR_INVALID before any launch: a null pointer, an unknown mode or boundary, an extent (of an
 * operand, or of a 'full' result) beyond INT_MAX, the shape of struct NDArray, and the 'valid' case in which neither operand
 * covers the other.  Library stream, no scratch, no atomics. */
typedef enum np_conv_mode { NP_CONV_VALID = 0, NP_CONV_SAME = 1, NP_CONV_FULL = 2 } np_conv_mode;
typedef enum np_conv_boundary { NP_CONV_FILL = 0, NP_CONV_SYMM = 4, NP_CONV_WRAP = 8 } np_conv_boundary;   /* PAD, REFLECT, CIRCULAR */
int np_correlate2d_shape(size_t ah, size_t aw, size_t bh, size_t bw, int mode, size_t *oh, size_t *ow);
int np_correlate2d(const float *a, size_t ah, size_t aw, const float *b, size_t bh, size_t bw,
                   int mode, int boundary, float fill_value, int flip, float *out);

/* ---- convolution layers (np_dnn.hip; DESIGN.md "dnn_conv2d") ----------------------------------------
 * The layer behind NDArray::dnn_conv2d_forward / dnn_conv2d_backward, which the reference refuses for GPU arrays unless it is
 * built against cuDNN (dnn.c:305, 361).  x (N, C, H, W), w (F, C, kh, kw), y and dy (N, F, oh, ow): ROW-MAJOR fp32, contiguous.
 * Cross-correlation with stride 1, dilation 1 and zero padding (ph, pw), 0 <= ph < kh, 0 <= pw < kw; no bias, no activation.
 *   y[n,f,i,j]  = sum_{c,p,q} w[f,c,p,q] . x~[n,c,i+p-ph,j+q-pw]            oh = H + 2 ph - kh + 1, ow = W + 2 pw - kw + 1
 *   dW[f,c,p,q] = sum_{n,i,j} dy[n,f,i,j] . x~[n,c,i+p-ph,j+q-pw]           the filters' own shape
 *   dX[n,c,u,v] = sum_{f,p,q} dy[n,f,u-p+ph,v-q+pw] . w[f,c,p,q]            the input's own shape
 * where x~ is x with STORED zeros around it: a padded zero under an Inf tap gives NaN, as a materialised padded array would.
 * np_conv2d_shape: (oh, ow), no device needed.  The three others compute one array each; the result must not overlap an operand.
 * Fine print:
 *   - implicit GEMM on the fp32 MFMA: no im2col matrix is written.  The data gradient is the forward kernel on dy with the
 *     filters flipped and transposed into pool scratch, pad (kh - 1 - ph, kw - 1 - pw); the filter gradient cuts its reduction
 *     over N.oh.ow into S slices (S from the extents alone), whose partial results go to pool scratch and are added in slice
 *     order by a second kernel.  No float atomics.
 *   - fixed order: every element of y (dX) is one fp32 fmaf chain from +0.0f over k = (c.kh + p).kw + q ascending (over
 *     (f.kh + p').kw + q' of the flipped window); the order depends on (C, kh, kw) (resp. F, kh, kw) alone, never on N, on where
 *     the pixel lies or on the tile, so an image gives the same bits at any batch size and position.  dW: a chain over
 *     n.oh.ow + i.ow + j inside a slice, slices added in order.  All three are bit-identical from run to run.
 *   - nothing outside an output's receptive field is read into it: a NaN in x, w or dy reaches exactly the outputs the formulas
 *     above give it.
 * Convention: pointers are checked first, then the shape, then work begins.  NP_ERR_INVALID before any device work: a null
 * pointer; an extent of zero; ph >= kh or pw >= kw; kh > H + 2 ph or kw > W + 2 pw; any of numel(x), numel(w), numel(y),
 * N.oh.ow, C.kh.kw or F.kh.kw at 2^31 or more (refused, never truncated).  Library stream; scratch comes from the caching pool
 * and is released on every path.
 * These four are the _ex calls below at (sh, sw, dh, dw) = (1, 1, 1, 1) and go through the same checks, so they also refuse a
 * padded extent H + 2 ph or W + 2 pw of 2^31 or more (the kernels form the row index i + p - ph as an int), and a refusal is
 * worded as the _ex calls word it: "every extent, stride and dilation must be at least 1", "the effective window". */
int np_conv2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t *oh, size_t *ow);
int np_conv2d_forward(const float *x, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                      size_t ph, size_t pw, float *y);
int np_conv2d_backward_data(const float *dy, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                            size_t ph, size_t pw, float *dx);
int np_conv2d_backward_filter(const float *x, const float *dy, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                              size_t ph, size_t pw, float *dw);

/* ---- convolution layers with a stride and a dilation (np_dnn.hip; DESIGN.md "dnn_conv2d") ------------
 * The calls above with a window stride (sh, sw) >= 1 and a tap dilation (dh, dw) >= 1, inserted after (ph, pw).  The effective
 * window is keh = dh (kh - 1) + 1, kew = dw (kw - 1) + 1, and 0 <= ph < keh, 0 <= pw < kew.
 *   oh = floor((H + 2 ph - keh) / sh) + 1, ow = floor((W + 2 pw - kew) / sw) + 1
 *   y[n,f,i,j]  = sum_{c,p,q} w[f,c,p,q] . x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
 *   dW[f,c,p,q] = sum_{n,i,j} dy[n,f,i,j] . x~[n,c,i.sh+p.dh-ph,j.sw+q.dw-pw]
 *   dX[n,c,u,v] = sum_{f,p,q} dy~[n,f,(u+ph-p.dh)/sh,(v+pw-q.dw)/sw] . w[f,c,p,q]   a quotient that is no integer in range: a stored zero
 * One gather serves all three: position t = i.s - pad + p.d on the grid of the gathered operand dilated by l reads in[t / l]
 * when t >= 0, t mod l == 0 and t / l < extent, else a STORED zero.  Forward and dW gather x with l = 1; dX is the forward
 * kernel over dy with the filters flipped and transposed, stride 1, the layer's tap dilation, pad (keh - 1 - ph, kew - 1 - pw),
 * input dilation (sh, sw) and output (H, W).  The dilated input spends sh.sw times the useful multiply-adds on stored zeros.
 * Rows and columns of x that no window reads (the remainder of the floor) get dX = +0.0f for finite filters, and a NaN there
 * in x reaches nothing.
 * The reduction orders are the ones stated above and do not depend on the stride or the dilation: a strided y is bit for bit
 * the subsample of the unit-stride y, a dilated y the unit y of the zero-stuffed filter (finite data), a strided dX the unit dX
 * of the zero-stuffed dy where (H + 2 ph - keh) mod sh == 0 and likewise for W.  With (sh, sw, dh, dw) = (1, 1, 1, 1) the calls
 * launch the same kernels as the calls above and return the same bits.
 * Convention as above.  NP_ERR_INVALID before any device work: a null pointer; an extent, stride or dilation of zero;
 * ph >= keh or pw >= kew; keh > H + 2 ph or kew > W + 2 pw; H + 2 ph, W + 2 pw, keh, kew, a stride, any of numel(x), numel(w),
 * numel(y), N.oh.ow, C.kh.kw or F.kh.kw at 2^31 or more. */
int np_conv2d_shape_ex(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw,
                       size_t *oh, size_t *ow);
int np_conv2d_forward_ex(const float *x, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                         size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *y);
int np_conv2d_backward_data_ex(const float *dy, const float *w, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                               size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *dx);
int np_conv2d_backward_filter_ex(const float *x, const float *dy, size_t N, size_t C, size_t H, size_t W, size_t F, size_t kh, size_t kw,
                                 size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, float *dw_out);

/* ---- convolution layers with a bias and an activation (np_dnn.hip; DESIGN.md "dnn_conv2d") ------------
 * np_conv2d_forward_act is np_conv2d_forward_ex with an epilogue in the same kernel, applied to every output while it is still
 * in registers.  With acc the fmaf chain of np_conv2d_forward_ex, untouched, for an output of filter f:
 *   v = bias ? acc + bias[f] : acc        ONE fp32 add after the chain: the bias is NOT the chain's start value
 *   y = act(v)
 *   NP_ACT_NONE     v
 *   NP_ACT_RELU     (v <= 0) ? +0.0f : v          a NaN stays NaN, -0.0 becomes +0.0
 *   NP_ACT_TANH     tanhf(v)                      the function np_unary(NP_TANH) evaluates: bit for bit the unfused result
 *   NP_ACT_SIGMOID  1 / (1 + exp(-v))             with the exp of np_unary(NP_EXP): 0 and 1 at -Inf and +Inf, NaN at NaN
 * bias: F floats, or NULL for no bias; bias[f] is read for f < F only.  A NaN in bias[f] reaches exactly the outputs of filter
 * f.  With bias == NULL and NP_ACT_NONE the call launches the same kernels as np_conv2d_forward_ex and returns the same bits.
 *
 * np_conv2d_backward_act is the backward pass of that epilogue: one streaming kernel over y (the forward RESULT) and dy, both
 * (N, F, P) with P = oh.ow, and a fold.  The derivative is expressed through the output, so a layer keeps y only:
 *   dz[n,f,i,j] = dy . act'(y)
 *   NP_ACT_RELU     (y <= 0) ? +0.0f : dy         a select, not a product: a NaN or Inf in dy over y <= 0 reaches nothing; a NaN y
 *                                                 passes dy
 *   NP_ACT_TANH     dy * (1 - y*y)                each operation rounded on its own, in this order
 *   NP_ACT_SIGMOID  dy * ((1 - y) * y)
 *   db[f]       = sum_{n,i,j} dz[n,f,i,j]
 * With NP_ACT_NONE dz = dy: dz is NOT written (it may be NULL, and so may y) and only db is produced.  With db == NULL only dz is
 * written.  dW and dX of the layer are np_conv2d_backward_filter_ex / np_conv2d_backward_data_ex on dz.
 * The summation order of db: the M = N.P elements of filter f, indexed m = n.P + i.ow + j, are cut into S slices of L elements
 * (S and L from (N, F, P) alone); inside a slice lane t of 256 adds elements t, t + 256, ... in ascending order from +0.0f, the 256
 * lane sums are folded in a fixed tree (lanes 32, 16, 8, 4, 2, 1 apart inside a wave of 64, then the four waves in order), the
 * slices go to pool scratch and a second kernel adds them in slice order (S == 1 writes db directly).  No float atomics; db is
 * bit-identical from run to run, and dz of an image does not depend on the batch it is in.  db of a batch is not the sum of the
 * dbs of its images.
 * dz may not overlap y or dy; db may not overlap anything.
 * Convention as above: pointers are checked first, then the shape, then work begins.  NP_ERR_INVALID before any device work:
 * everything np_conv2d_forward_ex refuses; an unknown act; dz and db both NULL; dz (or y) NULL with an activation; an extent
 * of zero; N.F.P at 2^31 or more. */
typedef enum np_conv_act { NP_ACT_NONE = 0, NP_ACT_RELU = 1, NP_ACT_TANH = 2, NP_ACT_SIGMOID = 3 } np_conv_act;
int np_conv2d_forward_act(const float *x, const float *w, const float *bias, size_t N, size_t C, size_t H, size_t W, size_t F,
                          size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t dh, size_t dw, int act, float *y);
int np_conv2d_backward_act(const float *y, const float *dy, size_t N, size_t F, size_t P, int act, float *dz, float *db);

/* ---- pooling layers: max and average pool2d (np_pool.hip; DESIGN.md "dnn_pool2d") ------------
 * x is (planes, H, W) row-major fp32, contiguous, planes = N.C.  The window is (kh, kw), the stride (sh, sw) >= 1 and the
 * zero-width padding (ph, pw) satisfies 2 ph <= kh and 2 pw <= kw, so every window holds at least one real cell.
 * Out of scope: no dilation and no ceil mode.
 *   oh = floor((H + 2 ph - kh) / sh) + 1, ow = floor((W + 2 pw - kw) / sw) + 1
 * Window (i, j) covers rows i.sh - ph ... i.sh - ph + kh - 1 clipped to [0, H) and columns likewise: its real cells.
 *   NP_POOL_MAX        the real cells are scanned in row-major order from best = -Inf, idx = the first real cell; a cell is
 *                      taken when v > best || v != v.  So the first of equal maxima wins, -0.0 and +0.0 are equal, a NaN in
 *                      the window gives NaN and the index is that of the last NaN.  Padding is never a candidate.
 *                      idx[plane, i, j] = u.W + v is an int32 within the plane; writing idx is optional (NULL).
 *   NP_POOL_AVG        one chain of plain fp32 adds from +0.0f over the real cells in row-major order, then one correctly
 *                      rounded fp32 division by (float) divisor, divisor = kh.kw: padding counts.  No multiplication by a
 *                      reciprocal.
 *   NP_POOL_AVG_VALID  the same with divisor = the number of real cells.
 * Backward: dx[plane, u, v] is a gather, never a scatter.  The lane that owns (u, v) walks the windows (i, j) that cover it with
 * i ascending, then j ascending, and adds its terms from +0.0f with plain fp32 adds.  The max term is dy[i,j] where
 * idx[i,j] == u.W + v; the average term is dy[i,j] / (float) divisor(i,j), rounded on its own before the add.  Cells that no
 * window covers (stride > window, or the floor remainder) get +0.0f.  No float atomics; results are bit-identical from run to
 * run, and a plane's result does not depend on how many planes are in the call.
 * NaN reach: a NaN in x reaches exactly the outputs whose window holds it; a NaN in dy[i,j] reaches exactly the dx cells that
 * term is added to.
 * y, idx and dx may not overlap an input.  The calls run on the library stream and need no scratch; np_pool2d_shape needs no
 * device.
 * Convention as above: pointers are checked first, then the shape, then work begins.  NP_ERR_INVALID before any device work: a
 * null pointer, idx == NULL for a max backward included (idx is ignored by the average modes); a zero extent, window or stride;
 * an unknown mode; 2 ph > kh or 2 pw > kw; kh > H + 2 ph or kw > W + 2 pw; kh.kw at 2^24 or more; H.W, numel(x), numel(y), a
 * stride, H + 2 ph or W + 2 pw at 2^31 or more: refused, never truncated. */
typedef enum np_pool_mode { NP_POOL_MAX = 0, NP_POOL_AVG = 1, NP_POOL_AVG_VALID = 2 } np_pool_mode;
int np_pool2d_shape(size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw, size_t sh, size_t sw, size_t *oh, size_t *ow);
int np_pool2d_forward(const float *x, size_t planes, size_t H, size_t W, size_t kh, size_t kw, size_t ph, size_t pw,
                      size_t sh, size_t sw, int mode, float *y, int32_t *idx);   /* idx: NULL, or planes.oh.ow ints (max only) */
int np_pool2d_backward(const float *dy, const int32_t *idx, size_t planes, size_t H, size_t W, size_t kh, size_t kw,
                       size_t ph, size_t pw, size_t sh, size_t sw, int mode, float *dx);   /* idx needed for max, ignored otherwise */

/* ---- softmax, log-softmax and cross-entropy (np_softmax.hip; DESIGN.md "softmax") ------------
 * The operand is a contiguous fp32 array seen as (outer, cols, inner); the softmax runs over cols; inner == 1 is the row case.
 *   Row statistics  m is the row maximum (a NaN never wins the comparison).  d_i = x_i - m is one fp32 subtract.
 *                   e_i = fast_exp(d_i), the fast_exp that NDArray.exp uses: exp(0) == 1 and exp(-Inf) == 0 exactly.
 *   Row sum         s = sum of e_i: a chain or tree of plain fp32 adds from +0.0f.  Its order depends on (cols, inner) and the
 *                   kernel form alone; it never depends on outer, on the row's position or on pointer alignment.  The
 *                   streaming and strided forms keep a running maximum over chunks of 8 elements: when a chunk raises it, the
 *                   sum so far is multiplied by one fast_exp of the step before the chunk's own chain is added.
 *   Softmax         y_i = e_i / s, one correctly rounded division.  No reciprocal.
 *   Log-softmax     y_i = d_i - logf(s).
 *   Special values  as torch's CPU softmax behaves: a row that holds a NaN or a +Inf, or that is entirely -Inf, comes out NaN in
 *                   every element; no other row is touched.  A -Inf among finite values gives +0.0f for softmax and -Inf for
 *                   log-softmax.
 *   Softmax backward, from the output       dx_i = y_i . (dy_i - sum_j dy_j . y_j)
 *   Log-softmax backward, from the output   dx_i = dy_i - fast_exp(y_i) . sum_j dy_j
 *   Backward sums   fixed-order fp32 sums from +0.0f under the same rule as s; every product is rounded on its own.  No float
 *                   atomics.
 *   Cross-entropy, index targets   target holds `rows` class indices as fp32 (the library has one element type).
 *                   loss_rows[r] = logf(s) - d_label: bit for bit -np_softmax_forward(..., NP_LOG_SOFTMAX)[r, label], the same
 *                   row-statistics code in the same form (a zero loss is +0.0f where the negation would be -0.0f).
 *   Invalid labels  a label that is not an integer in [0, cols), a NaN included, makes that row's loss NaN and every element of
 *                   its gradient NaN.  Nothing is read out of bounds and no sticky device error is raised.
 *   Cross-entropy, probability targets   target is (rows, cols).  loss_r = sum_j t_j . (logf(s) - d_j), summed from +0.0f in
 *                   ascending j by the lane that owns the elements (the whole row in the short-row form), lanes then joined as
 *                   for s.  Terms with t_j == 0 are skipped, so a one-hot row over -Inf logits is finite, and a one-hot target
 *                   gives the same bits as the index form.
 *   Gradient        when dlogits != NULL: dlogits_i = (p_i - t_i) . scale, one fp32 subtract and then one multiply; p_i is bit
 *                   for bit what np_softmax_forward returns; t is assumed to sum to 1; for index targets t is the one-hot of
 *                   the label.
 *   One launch      loss and gradient come from ONE read of the logits, in one launch (the streaming form reads a row twice).
 *   Aliasing        outputs may not overlap inputs, with one exception: dx may alias dy (dx == dy).
 *   Sizes           all size_t.  cols >= 2^31 is refused with a message, never truncated; outer.cols.inner beyond 2^31
 *                   elements works.
 *   Determinism     the work runs on the library stream and needs no scratch.  Results are bit-identical from run to run; a
 *                   row alone gives the same bits as the same row inside a larger outer.
 *   Alignment       any 4-byte-aligned pointer is accepted and gives the same bits as a 16-byte-aligned one.
 * Convention as above: pointers are checked first, then the extents, the mode, the aliasing, then work begins.  NP_ERR_INVALID
 * before any device work: a null pointer (dlogits may be NULL), a zero extent, an unknown mode or target kind, cols at 2^31 or
 * more, overlapping operands. */
typedef enum np_softmax_mode { NP_SOFTMAX = 0, NP_LOG_SOFTMAX = 1 } np_softmax_mode;
typedef enum np_xent_target { NP_XENT_INDEX = 0, NP_XENT_PROB = 1 } np_xent_target;
int np_softmax_forward(const float *x, size_t outer, size_t cols, size_t inner, int mode, float *y);
int np_softmax_backward(const float *y, const float *dy, size_t outer, size_t cols, size_t inner, int mode, float *dx);
int np_cross_entropy(const float *logits, const float *target, size_t rows, size_t cols, int target_kind, float scale,
                     float *loss_rows, float *dlogits /* may be NULL */);

/* ---- batch normalization (np_batchnorm.hip; DESIGN.md "batch normalization") ------------
 * The operand is a contiguous fp32 array seen as (N, C, inner): inner == 1 is the (N, C) output of a dense layer, inner = H.W is
 * NCHW.  The statistics are per channel c over the n = N.inner values x[., c, .].
 *   Statistics      carried in fp64.  Per channel a shift K = x[0, c, 0]; S1 = sum of (x - K) and S2 = sum of (x - K)^2 are
 *                   accumulated in double from +0.0 (the difference of two floats is exact in double except for exponent gaps
 *                   beyond 29).
 *                   mean64 = K + S1 / n.  var64 = S2 / n - (S1 / n)^2, the biased variance.  The order of the additions
 *                   depends on (N, C, inner) and the kernel form alone; it moves the fp64 values far below fp32 resolution.
 *   Saved values    save_mean = f32(mean64), save_invstd = f32(1 / sqrt(var64 + eps)): each ONE rounding of an fp64 value.
 *                   eps and momentum are doubles.
 *   Element         identical in training and inference, three separately rounded fp32 steps, no contraction:
 *                   d = x - mean; h = d . invstd; y = h . gamma[c] + beta[c], a multiply, then an add.  A NULL gamma means 1 and
 *                   a NULL beta means 0, and their steps are skipped.
 *   Inference       training == 0 takes running_mean and running_var (both required): mean = running_mean,
 *                   invstd = f32(1 / sqrt((double) running_var + eps)).  Inference on the statistics that training saved gives
 *                   training's y bit for bit.  save_mean and save_invstd are not touched.
 *   Running statistics   optional in training (NULL pointers skip them), updated in place:
 *                   r = f32((1 - momentum) . (double) r + momentum . s64), s64 = mean64 for the running mean and
 *                   s64 = var64 . n / (n - 1), the unbiased variance, for the running variance.
 *   n == 1          training with one value per channel is refused with a message; inference with n == 1 is fine.
 *   Backward        training mode, from x, dy, gamma, save_mean, save_invstd.  xh = (x - mean) . invstd rounded as above.
 *                   sum of dy and sum of dy . xh are accumulated in fp64 from +0.0, each product formed in double from the two floats.
 *                   dbeta = f32(sum dy); dgamma = f32(sum dy . xh); mb = f32(sum dy / n); mg = f32(sum dy . xh / n);
 *                   dx = (gamma . invstd) . ((dy - mb) - xh . mg), every step a separately rounded fp32 operation in exactly
 *                   that association (a NULL gamma: invstd alone).  dgamma and dbeta may be NULL.
 *   Special values  a channel that holds a NaN or +-Inf comes out NaN in every element of y and dx; no other channel is
 *                   touched.  A constant channel has var64 = 0: with eps > 0, y = beta exactly; with eps = 0, invstd = +Inf
 *                   and y = NaN.  eps < 0 is refused; momentum outside [0, 1] is refused.
 *   Aliasing        dx may alias dy (dx == dy).  No other output may overlap an input or another output.
 *   Sizes           all size_t.  C >= 2^31 is refused with a message, never truncated; N.C.inner beyond 2^31 elements works.
 *   Determinism     no float or double atomics; partial sums go to pool scratch that is released on every path; the work runs
 *                   on the library stream.  Results are bit-identical from run to run.
 *   Alignment       any 4-byte-aligned pointer is accepted and gives the same bits as a 16-byte-aligned one.
 * Convention as above: pointers are checked first, then the extents, the parameters, the aliasing, then work begins.
 * NP_ERR_INVALID before any device work: a null pointer (gamma, beta, dgamma, dbeta and, in training, the running statistics may
 * be NULL), a zero extent, C at 2^31 or more, a negative eps, a momentum outside [0, 1], n == 1 in training, overlapping
 * operands. */
int np_batchnorm_forward(const float *x, const float *gamma, const float *beta, size_t N, size_t C, size_t inner, int training,
                         double momentum, double eps, float *running_mean, float *running_var, float *y, float *save_mean,
                         float *save_invstd);
int np_batchnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd,
                          size_t N, size_t C, size_t inner, float *dx, float *dgamma /* may be NULL */, float *dbeta /* may be NULL */);

/* ---- layer and group normalization (np_groupnorm.hip; DESIGN.md "layer and group normalization") ------------
 * One geometry serves both.  The operand is a contiguous fp32 array seen as (N, G, D, inner): M = N.G rows of L = D.inner
 * contiguous floats, P = G.D affine parameters, and element j of row r uses parameter (r mod G).D + j / inner.
 *   Layer normalization over the trailing axes is G = 1, D = L, inner = 1 (P = L).  Group normalization of (N, C, spatial...)
 *   with num_groups = G is D = C / G, inner = the product of the spatial extents (P = C).  Instance normalization is G = C.
 * It is batch normalization's definition applied per row:
 *   Statistics      carried in fp64.  Per row a shift K = x[r, 0]; S1 = sum of (x - K) and S2 = sum of (x - K)^2 are accumulated
 *                   in double from +0.0.  mean64 = K + S1 / L.  var64 = S2 / L - (S1 / L)^2, the biased variance.  The order of
 *                   the additions depends on (N, G, D, inner) and the kernel form alone.
 *   Saved values    save_mean[r] = f32(mean64), save_invstd[r] = f32(1 / sqrt(var64 + eps)), r = 0 .. N.G - 1: each ONE rounding of
 *                   an fp64 value.  eps is a double.
 *   Element         three separately rounded fp32 steps, no contraction: d = x - mean; h = d . invstd;
 *                   y = h . gamma[p] + beta[p], a multiply, then an add.  A NULL gamma means 1 and a NULL beta means 0, and
 *                   their steps are skipped.
 *   Backward, per row        xh = (x - mean) . invstd rounded as above.  g = f32(dy . gamma[p]) (a NULL gamma: g = dy).  sum of g
 *                   and sum of g . xh are accumulated in fp64 from +0.0, each product formed in double from the two floats.
 *                   mb = f32(sum g / L); mg = f32(sum g . xh / L); dx = invstd . ((g - mb) - xh . mg), every step a separately
 *                   rounded fp32 operation in exactly that association.
 *   Backward, per parameter  dbeta[p] = f32(sum dy) and dgamma[p] = f32(sum dy . xh) over every element that uses parameter p,
 *                   in fp64 from +0.0, products formed in double.  Either may be NULL; with both NULL the reduction is not
 *                   launched.
 *   Special values  a row that holds a NaN or +-Inf comes out NaN in every element of y and dx; no other row is touched.  A
 *                   constant row has var64 = 0: with eps > 0, y = beta exactly; with eps = 0, invstd = +Inf and y = NaN.  The
 *                   same holds for L = 1, which is accepted.  eps < 0 is refused.
 *   Aliasing        dx may alias dy (dx == dy).  No other output may overlap an input or another output.
 *   Sizes           all size_t.  M = N.G or P = G.D at 2^31 or more is refused with a message, never truncated; element offsets
 *                   are size_t, so N.G.D.inner beyond 2^31 elements works.
 *   Determinism     no float or double atomics; partial sums go to pool scratch that is released on every path; the work runs
 *                   on the library stream; forms and slice counts come from (N, G, D, inner) alone.  Results are bit-identical
 *                   from run to run.
 *   Alignment       any 4-byte-aligned pointer is accepted and gives the same bits as a 16-byte-aligned one.
 * Convention as above: pointers are checked first, then the extents, the parameters, the aliasing, then work begins.
 * NP_ERR_INVALID before any device work: a null pointer (gamma, beta, dgamma and dbeta may be NULL), a zero extent, M or P at 2^31
 * or more, a negative eps, overlapping operands. */
int np_groupnorm_forward(const float *x, const float *gamma /* P, may be NULL */, const float *beta /* P, may be NULL */,
                         size_t N, size_t G, size_t D, size_t inner, double eps,
                         float *y, float *save_mean /* N.G */, float *save_invstd /* N.G */);
int np_groupnorm_backward(const float *x, const float *dy, const float *gamma, const float *save_mean, const float *save_invstd,
                          size_t N, size_t G, size_t D, size_t inner,
                          float *dx, float *dgamma /* P, may be NULL */, float *dbeta /* P, may be NULL */);

/* ---- scaled dot-product attention (np_attention.hip; DESIGN.md "scaled dot-product attention") ------------
 * o = softmax(q . k^T . scale) . v per slice, fused: the (Sq x Sk) score matrix is never stored.  Operands are contiguous fp32:
 * q (BH, Sq, D), k (BH, Sk, D), v (BH, Sk, D), o (BH, Sq, D), the row statistics save_max and save_sum (BH, Sq).
 * 1 <= D <= 128; Sq, Sk, BH >= 1.  For query row i of slice b the visible keys are all j, or j <= i when causal: the alignment is
 * top-left, so every row sees at least key 0 whatever Sq and Sk are.
 *   Score           s_ij = f32(chain_d(q_id . k_jd) . scale): the matrix core's fp32 fmaf chain from +0.0f over d ascending, then
 *                   ONE fp32 multiply of the finished dot product by scale.  scale is a float argument.
 *   Maximum         m_i = the maximum over the visible j, from -Inf; a NaN never wins (row_max of the softmax unit).
 *   Sum             e_ij = fast_exp(s_ij - m_i); l_i = sum of e_ij, evaluated online over key tiles: a tile that raises the running
 *                   maximum multiplies the running sum and the running output by ONE fast_exp of the step (the rescaling of
 *                   online_add), then adds its own e against the new maximum.  Key tiles are always walked from key 0 in
 *                   ascending order; the order of the keys inside a tile is a fixed permutation.
 *   Output          o_id = (sum of e_ij . v_jd) / l_i: ONE correctly rounded division per element, no reciprocal.
 *   Saved values    save_max = m_i, save_sum = l_i: what the online evaluation ended with.  Either may be NULL.
 *   Backward        takes q, k, v, o, dout, save_max, save_sum.  p_ij = fast_exp(s_ij - m_i) / l_i, the same instruction sequence
 *                   as the forward probability.  delta_i = sum over d of dout_id . o_id; dp_ij = chain_d(dout_id . v_jd);
 *                   ds_ij = p_ij . (dp_ij - delta_i); dv_jd = sum over i of p_ij . dout_id; dk_jd = (sum over i of ds_ij . q_id) . scale;
 *                   dq_id = (sum over j of ds_ij . k_jd) . scale.  Any of dq, dk, dv may be NULL; a kernel that would only
 *                   produce NULL outputs is not launched.
 *   Determinism     no float atomics; every reduction order is a function of the extents and the compile-time tile constants
 *                   alone.  Results are bit-identical from run to run.
 *   Independence    by bits: a slice alone equals the same slice inside a larger batch.  Without causal, the first n rows of a
 *                   call equal the call on q[:, :n].  With causal, row i reads the key tiles 0 .. i / T alone (T = the key tile,
 *                   np_debug_attention_bounds) and masks the keys above i to -Inf, which is what a key past Sk gets too: on
 *                   finite operands row i equals row i of the call on q[:, :n], k[:, :c], v[:, :c] for every n > i and every
 *                   c with min(c, i + 1) = min(Sk, i + 1); cutting both to i + 1 rounded up to T is one such call.
 *   Special values  a NaN or +-Inf anywhere in q[b, i, :] makes row i of o, save_sum and dq NaN, and no other row of o.  A NaN in
 *                   k[b, j] or v[b, j] makes every row that sees j NaN.  Under causal, rows i < j that share a key tile with j
 *                   are NOT specified: 0 . NaN on the matrix core is NaN, as in a materialised computation, and skipped tiles never
 *                   read it.  No other slice b is ever reached.  A row whose visible scores are all -Inf is NaN in o and in save_sum
 *                   (e_ij = fast_exp(-Inf + Inf)); its save_max is -Inf.
 *   Memory          the forward pass takes no scratch.  The backward pass takes pool scratch for delta (BH.Sq floats) and for
 *                   nothing proportional to Sq.Sk; it is released on every path.  The work runs on the library stream.
 *   Sizes           all size_t; every offset is formed in size_t, so BH.S.D may pass 2^31.  Sq or Sk at 2^31 or more, or BH times
 *                   the tiles of a slice at 2^31 or more, does not fit the grid arithmetic and is refused.
 * Convention as above: pointers are checked first, then the extents, the scale, the aliasing, then work begins.
 * NP_ERR_INVALID before any device work: a null pointer (save_max, save_sum, dq, dk, dv may be NULL), a zero extent, D > 128, an
 * extent that does not fit, a scale that is not finite, an output that overlaps an input or another output. */
int np_attention_forward(const float *q, const float *k, const float *v, size_t BH, size_t Sq, size_t Sk, size_t D,
                         int causal, float scale, float *o, float *save_max /* may be NULL */, float *save_sum /* may be NULL */);
int np_attention_backward(const float *q, const float *k, const float *v, const float *o, const float *dout,
                          const float *save_max, const float *save_sum, size_t BH, size_t Sq, size_t Sk, size_t D,
                          int causal, float scale, float *dq, float *dk, float *dv);

/* ---- optimizer steps (np_optim.hip; DESIGN.md "optimizer steps") ------------
 * One call updates a LIST of T tensors in place: tensor t has counts[t] contiguous fp32 elements, a parameter params[t], a
 * gradient grads[t] and zero, one or two state arrays.  The pointer arrays and counts are HOST arrays of device pointers; the list
 * travels in the kernel arguments, so a call copies nothing, takes no scratch and does not synchronise; it runs on the library
 * stream and may be captured between np_graph_begin and np_graph_end.  T tensors take ceil(T / 64) launches.
 *   Element         an element's result depends on that element's operands and the scalar arguments alone: the length of the
 *                   list, the order of the tensors, the packing into launches, the chunking and the alignment cannot change a bit.
 *                   Every step below is a separately rounded fp32 operation, no contraction; division and square root are
 *                   correctly rounded, there is no reciprocal and no rsqrt; denormals are kept.
 *   Coefficients    computed in double on the host from the double arguments and rounded to fp32 ONCE: lr, wd = weight_decay,
 *                   mu = momentum, omd = f32(1 - dampening); for Adam b1 = beta1, b2 = beta2, omb1 = f32(1 - beta1),
 *                   omb2 = f32(1 - beta2), lrwd = f32(lr . weight_decay), bc2s = f32(sqrt(1 - beta2^step)),
 *                   ss = f32(lr / (1 - beta1^step)), eps.  s = *grad_scale is a DEVICE float that the kernel reads.
 *   Skipping        a step that a coefficient makes the identity is SKIPPED, not multiplied through (0 . Inf would otherwise
 *                   differ): weight_decay == 0 skips the decay step; momentum == 0 skips the buffer, and bufs and its entries
 *                   may be NULL; a NULL grad_scale skips the scale.  Nothing else is skipped: omd . g2 is formed when dampening == 0.
 *   np_sgd_step     torch.optim.SGD.  g1 = g . s.  g2 = g1 + (wd . p), a multiply, then an add.  With momentum:
 *                   b = g2 when first_step, else b = (mu . b) + (omd . g2), two multiplies, then an add; d = g2 + (mu . b) with
 *                   nesterov (the new b), else d = b.  Without momentum d = g2.  p = p - (lr . d), a multiply, then a subtract.
 *                   first_step does not read the buffer.
 *   np_adam_step    torch.optim.Adam, and AdamW when decoupled.  g1 = g . s.  decoupled: p1 = p - (lrwd . p), g2 = g1; otherwise
 *                   g2 = g1 + (wd . p), p1 = p.  m = (b1 . m) + (omb1 . g2).  v = (b2 . v) + ((omb2 . g2) . g2).
 *                   den = (sqrt(v) / bc2s) + eps.  p = p1 - (ss . (m / den)).  step >= 1 is the number of this update; exp_avg and
 *                   exp_avg_sq are required.
 *   Special values  a NaN or +-Inf gradient element reaches its own element of p and the states, and no other.  weight_decay == 0
 *                   with p = +-Inf leaves g untouched.  eps = 0 with v = 0 gives m / 0: NaN for m = 0.
 *   Aliasing        no written range (the parameters and states of ALL tensors) may overlap another written range, a gradient or
 *                   grad_scale; found on the host by sorting the ranges.  Two gradients may share memory: grads[t] == grads[u].
 *   Sizes           all size_t; counts[t] beyond 2^31 works.
 *   Alignment       any 4-byte-aligned pointer is accepted.  A tensor whose pointers are all congruent mod 16 is updated with
 *                   16-byte accesses over its aligned middle and scalar accesses at its head and tail, any other with scalar
 *                   accesses; the choice is per tensor and both forms give the same bits.
 *   Determinism     no atomics, no scratch.  Results are bit-identical from run to run.
 * Convention as above: pointers are checked first, then the extents, the parameters, the aliasing, then work begins.
 * NP_ERR_INVALID before any device work: a null list or a null required pointer; T = 0 or a counts[t] = 0; an lr, weight_decay or eps
 * that is negative or not finite; a momentum or dampening outside [0, 1]; nesterov with momentum == 0 or dampening != 0; a beta
 * outside [0, 1); step < 1; overlapping ranges. */
int np_sgd_step(float *const *params, const float *const *grads, float *const *bufs /* may be NULL when momentum == 0 */,
                const size_t *counts, size_t T, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                int first_step, const float *grad_scale /* device, may be NULL */);
int np_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                 const size_t *counts, size_t T, long long step, double lr, double beta1, double beta2, double eps,
                 double weight_decay, int decoupled, const float *grad_scale /* device, may be NULL */);
/* The gradient norm of a list and torch's clip_grad_norm_ coefficient, written to two DEVICE floats; no host read, so dev_out2 + 1
 * is what the step calls take as grad_scale and clipping costs no synchronisation.
 *   S               sum over t and i of g^2, each square formed in double from the float (exact), accumulated in fp64 from +0.0.
 *                   One partial per 8192 elements of a tensor goes to pool scratch that is released on every path; one workgroup
 *                   adds the partials in a fixed order.  The order depends on (counts, T) alone: no atomics, bit-identical from
 *                   run to run, the same at every alignment.
 *   dev_out2[0]     f32(sqrt(S)): ONE rounding of an fp64 value.
 *   dev_out2[1]     f32(min(1, max_norm / ((double) dev_out2[0] + 1e-6))); 1 when max_norm is +Inf and the norm is finite.
 *   Classes         squares are never negative, so S is NaN exactly when an element is NaN, else +Inf when an element is +-Inf
 *                   (or f32(sqrt(S)) overflows), else finite.  norm NaN: the coefficient is NaN.
 *                   norm +Inf: the coefficient is 0, or NaN when max_norm is +Inf too.
 * NP_ERR_INVALID before any device work: a null pointer, T = 0, a counts[t] = 0, a max_norm that is negative or NaN, a result that
 * overlaps a gradient. */
int np_grad_norm(const float *const *grads, const size_t *counts, size_t T, double max_norm, float *dev_out2);

/* ---- dense layers (np_linear.hip; DESIGN.md "dnn_linear") ------------
 * torch's layout: x (M, K), w (N, K) = (out_features, in_features), bias (N) or NULL, y (M, N), all contiguous row-major fp32.
 *   y[m,n]  = act(sum_k x[m,k] . w[n,k] + bias[n])
 *   dz[m,n] = dy[m,n] . act'(y[m,n])
 *   dx[m,k] = sum_n dz[m,n] . w[n,k]
 *   dw[n,k] = sum_m dz[m,n] . x[m,k]
 *   db[n]   = sum_m dz[m,n]
 * act is an np_conv_act with exactly the rules written above np_conv2d_forward_act / np_conv2d_backward_act: v = acc + bias[n] is
 * ONE fp32 add after the reduction, then the activation; the derivative goes through the OUTPUT y, relu a select, tanh
 * dy * (1 - y*y), sigmoid dy * ((1 - y) * y), each operation rounded on its own.
 * One MFMA tile kernel (v_mfma_f32_32x32x2_f32) serves the three products, reading every operand along its own contiguous axis;
 * no transposed copy of x, w or dz is written.
 *   Order     every element of y, dx and dw is ONE fp32 fmaf chain from +0.0f over its reduction index in ascending order.  For y
 *             the order depends on K alone, for dx on N alone, not on M, the row's position, the tile or any device state: a row
 *             of x alone gives bit for bit the row it gives inside any batch.
 *             dw reduces over M: the ceil(M / 32) steps of 32 rows are cut into S slices of whole steps, S from (M, K, N) alone:
 *             tiles = ceil(N / TM) . ceil(K / 128) with TM the smallest of 32, 64, 128 that covers N (128 beyond),
 *             want = min(steps / 8, ceil(512 / tiles), 256), at least 1, steps_per_slice = ceil(steps / want),
 *             S = ceil(steps / steps_per_slice).  Inside a slice the chain runs over m ascending from +0.0f; the slices' tiles go
 *             to pool scratch and a second kernel adds them in slice order (S == 1 writes dw directly).
 *             dz and db come from one streaming kernel over y and dy whose lanes run along n.  The M rows are cut into S' slices
 *             of R rows, from (M, N) alone: want = min(M / 256, ceil(1024 / ceil(N / 64)), 256), at least 1, R = ceil(M / want)
 *             rounded up to a multiple of 4, S' = ceil(M / R).  Inside a slice that begins at row m0, four row groups g = 0 .. 3
 *             add rows m0 + g, m0 + g + 4, ... in ascending order from +0.0f, the four sums are added as ((s0 + s1) + s2) + s3,
 *             the slices go to pool scratch and a second kernel adds them in slice order (S' == 1 writes db directly).
 *             No float atomics anywhere; every result is bit-identical from run to run.  dw and db of a batch are not the sums of
 *             the dws and dbs of its rows.
 *   NaN       the reduction's tail and the tile edges are stored zeros on both operands: a NaN in row m of x reaches exactly row
 *             m of y, a NaN in row n of w exactly column n, a NaN in bias[n] exactly column n.  A NaN in dy[m,n] reaches dz[m,n],
 *             row m of dx, row n of dw and db[n]; an Inf or NaN dy over a relu-dead output (y <= 0) reaches nothing.
 *   Backward  with NP_ACT_NONE dz = dy: dz is NOT written and neither y nor dz is read; both may be NULL.  With an activation dz is
 *             a caller buffer of M.N floats that receives dz; it may be NULL only when dx and dw are both NULL (db alone).
 *             Each of dx, dw and db may be NULL and then costs no launch; at least one must not be.  x is read for dw only and w
 *             for dx only: either may be NULL when its product is not asked for.
 *   Overlaps  forward: y may not overlap x, w or bias.  Backward: dz may be dy itself (dz == dy: an element is read and then
 *             written by the same lane) and may not overlap dy in any other way; apart from that no written range (dz, dx, dw,
 *             db) may overlap another written range or a range the call reads (x, w, y, dy).
 *   Alignment any 4-byte-aligned pointer is accepted.  An operand whose pointer is 16-byte aligned and whose row length is a
 *             multiple of 4 is staged with 16-byte loads, any other with dword loads; the choice is per operand and both give
 *             the same bits.
 * Convention as above: pointers are checked first, then the extents, the activation, the pointers an activation needs, the
 * overlaps, then work begins.  NP_ERR_INVALID before any device work: a null required pointer; dx, dw and db all NULL; an extent
 * of zero; M.N, M.K or N.K at 2^31 or more; an unknown act; a refused overlap.
 *   Two forms each product (y, dx, dw) takes one of two forms, chosen per product from (M, K, N) alone: the tile form described above
 *             below a constant number of multiply-adds M.K.N, the library form from it up.  The library form sends the product through
 *             np_sgemm; the operand np_sgemm needs the other way round is first written to pool scratch by np_transpose2d (w for y,
 *             dz for dw; dx needs none) and released on every path; bias and activation are ONE in-place pass over y (the same
 *             one add, the same activation text).  Its results have the bits of the composition of the public calls np_transpose2d,
 *             np_sgemm, an fp32 add and the activation, on equally aligned operands.  np_sgemm's plan depends on M: batch
 *             invariance holds for the tile form only, and so do the summation orders stated above; the NaN rules, the
 *             refusals and dz / db (always the streaming kernel above) are the same in both forms.  The constants are measured
 *             (np_debug_linear_bounds reports them; DESIGN.md says which table fixed them). */
int np_linear_forward(const float *x, const float *w, const float *bias /* may be NULL */, size_t M, size_t K, size_t N, int act, float *y);
int np_linear_backward(const float *x, const float *w, const float *y, const float *dy, size_t M, size_t K, size_t N, int act,
                       float *dz, float *dx, float *dw, float *db);

/* ---- device-side initializers (the reference's own phpbench suite, benchmarks/initializers/) ------
 * The reference builds every array on the CPU (initializers.c) and a GPU user pays the PCIe copy on
 * ->gpu(); zeros / ones / full are np_memset0 / np_fill above.
 * np_identity: n x n, ones on the diagonal (NDArray_Identity, initializers.c:479-510).
 * np_arange:   x[0] = (float)start, x[i] = (float)((double)x[i-1] + step) — NDArray_Arange's
 *              recurrence (initializers.c:836-839), bit for bit, evaluated as per-binade arithmetic
 *              segments (see np_layout.hip). */
int np_identity(float *out, size_t n);
int np_arange(float *out, double start, double step, size_t n);

/* ---- the path's one collective (BASELINE config 5) --------------------------------------
 * One process per GPU (the reference's device model: NDArray::setDevice, numpower.c:615-635; it has no
 * multi-device code).  A batch-parallel workload keeps contiguous slabs per rank — e.g. batch b of a batched
 * matmul on rank b / (batch / world) — computes them with np_sgemm_strided_batched, and replicates the
 * result with ONE all-gather over xGMI (RCCL, loaded on demand).  All calls are enqueued on the library stream,
 * ordered with the kernels; nothing here is needed — or loaded — by a single-GPU process.
 *
 * np_comm_init   rank in [0, world); endpoint = "tcp://host:port" (rank 0 serves the RCCL id on that port
 *                to peers that introduce themselves; use 127.0.0.1 and a free port on one node) or a file path
 *                (rank 0 publishes the id there — replacing a stale file — peers poll for it; removed by
 *                np_comm_destroy and on a failed init).  Blocks until every rank has joined (120 s limit).  The
 *                device is the one np_init selected.
 * np_allgather   recv[r * bytes_per_rank ...] = rank r's send buffer, for every r; in place when
 *                send == recv + rank * bytes_per_rank.  Enqueued on the LIBRARY stream: ordered behind the kernels,
 *                no overlap with them.  Asynchronous for the host (np_sync / a read-back waits for it).
 * np_comm_max    max of one host float over the ranks (timing: the slowest rank); blocks.
 * np_comm_barrier returns once every rank's streams (library and communication) have reached the call. */
int np_comm_init(int rank, int world, const char *endpoint);
int np_comm_rank(void);    /* -1 without a communicator */
/* The collective library behind np_comm_*: ncclGetVersion() of the librccl.so.1 the library loads (e.g. 22707 = 2.27.7);
 * needs no communicator and no device — what bench.py prints next to a multi-GPU line. */
int np_comm_rccl_version(int *host_version);
int np_comm_world(void);   /*  0 without a communicator */
int np_allgather(const void *dev_send, void *dev_recv, size_t bytes_per_rank);
int np_comm_max(float value, float *host_max);
int np_comm_barrier(void);
int np_comm_destroy(void);

/* The overlapped form.  The communicator owns a second, high-priority stream.  np_allgather_async makes that stream
 * wait (an event, on the device) for everything the library stream has been given so far, then enqueues the gather
 * THERE and returns: kernels launched afterwards on the library stream run while the data travels.
 *   dev_recv_base + r * recv_stride_bytes  <-  rank r's `bytes` at dev_send, for every r  (recv_stride_bytes >= bytes;
 *   in place when dev_send is this rank's destination).
 * How the bytes travel:
 *   NP_GATHER_COLLECTIVE  one ncclAllGather; needs recv_stride_bytes == bytes
 *   NP_GATHER_P2P         one grouped exchange of ncclSend / ncclRecv pairs: each peer's piece crosses that peer's own
 *                         xGMI link straight into place (any stride; no staging buffer, no scatter copy)
 *   NP_GATHER_AUTO        COLLECTIVE when the destinations are contiguous, else P2P
 * np_comm_wait makes the library stream wait (on the device; the host does not block) for everything given to the
 * communication stream so far: call it before the gathered data is read by a kernel, np_sync or a copy.  Until then
 * the send region must not be rewritten and the destination not read. */
typedef enum np_gather_mode { NP_GATHER_AUTO = 0, NP_GATHER_COLLECTIVE = 1, NP_GATHER_P2P = 2 } np_gather_mode;
int np_allgather_async(const void *dev_send, void *dev_recv_base, size_t bytes, size_t recv_stride_bytes, int mode);
int np_comm_wait(void);
void *np_comm_stream(void);   /* the communication stream as a raw hipStream_t (NULL without a communicator) */

/* BASELINE config 5 as one call: C_full is the replicated result, world * slab matrices of M x N, contiguous.  This
 * rank multiplies its slab (A, B: `slab` matrices, strides in elements) straight into its window
 * C_full + rank * slab * M * N, in `chunks` pieces (as equal as they come; clipped to slab); the gather of piece c is
 * handed to the communication stream as soon as piece c's GEMM is enqueued and travels while piece c + 1 computes.
 * Ends with np_comm_wait(), so the next call on the library stream (or np_sync) sees the whole result.  chunks = 0
 * leaves the piece count to the library: a step model of the pipeline (GEMM rate, one xGMI link per peer, the start delay
 * a transfer pays while the GEMM holds the CUs) picks it from 1, 2, 4, 8, 16 — one piece when nothing travels (a one-rank
 * communicator) or under NP_GATHER_COLLECTIVE; this is what a caller without a reason of its own should pass.  chunks = 1
 * is "compute, then one all-gather" on two streams (mode picks the transport); chunks > 1 always travels P2P (the
 * pieces of a slab are one slab apart across ranks) and mode NP_GATHER_COLLECTIVE is refused.  The result is
 * bit-identical for every chunks / mode: the same GEMM kernel computes every matrix.  The reference has no batched
 * or multi-device matmul (linalg.c:239-242 rejects ndim > 2, numpower.c:615-635): the oracle for this call is the
 * loop of 2-D NDArray_Matmul over the batch. */
/* How the call above cuts a slab: piece c of `chunks` starts at item *host_lo and holds *host_count items (the first
 * slab % chunks pieces hold one more).  Pure arithmetic; needs no device and no communicator. */
int np_comm_piece(size_t slab, int chunks, int c, size_t *host_lo, size_t *host_count);
int np_sgemm_strided_batched_allgather(size_t slab, size_t M, size_t N, size_t K, const float *A, size_t stride_a,
                                       const float *B, size_t stride_b, float *C_full, int chunks, int mode);

/* Device-side waits.  A wait for this GPU's own work (a stream-ordering wait of the sharded matmul whose producer never ran,
 * a GEMM workgroup that never saw its siblings' partial tiles) gives up after a bounded number of polls and raises the
 * device's error word: np_sync / np_memcpy_d2h / host-result calls / np_comm_* calls on that device return NP_ERR_DEVICE until
 * np_clear_device_error() acknowledges it.
 * A wait for TRANSFERS (which depend on other ranks) gives up after np_comm_set_wait_limit seconds (default 600; 0 = never,
 * like the RCCL kernel it waits for) and raises the same error; np_comm_destroy releases whatever still waits
 * (after a grace period of 30 s, or of the wait limit if that is shorter, for transfers that are merely still travelling).
 * With peers (world > 1) the sharded GEMM is one launch per piece; see np_hip_debug.h (np_comm_set_variant) for the
 * forms kept for A/B measurements. */
int np_comm_set_wait_limit(double seconds);

/* Everything that only tests, sweeps and A/B measurements need — kernel-variant switches (process-global state),
 * planner / rendezvous / transport probes, error injection — is declared in np_hip_debug.h.  Same library; a binding
 * needs none of it. */

#ifdef __cplusplus
}
#endif

#endif /* NUMPOWER_AMD_NP_HIP_H */
