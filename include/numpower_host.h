/*
 * numpower_host.h — host-side mirror of the reference's NDArray L2/L3 interface for the hot path.
 *
 * PHP (and its headers) are not available where this was built, so the layer that sits between
 * the Zend glue (numpower.c) and the device back end is provided as a plain C-callable library
 * (libnumpower_host.so, written in C++) with the SAME entry-point names, argument meaning,
 * ownership rules and error messages as the reference's C files, so that numpower.c's
 * PHP_METHODs can call it unchanged:
 *
 *   struct NDArray / NDArrayDescriptor          src/ndarray.h:52-74   (same field order)
 *   NDArray_Zeros/Empty/EmptyLike/Copy/Fill,
 *   NDArray_CreateFrom{Double,Float,Long}Scalar  src/initializers.c:379-448,633-790
 *   NDArray_FREE                                 src/ndarray.c:587-632
 *   NDArray_ToGPU / NDArray_ToCPU                src/ndarray.c:1037-1093
 *   NDArray_{Add,Subtract,Multiply,Divide,Mod,Pow}_Float, NDArray_Abs,
 *   NDArray_Sum_Float / Float_Prod / Mean_Float  src/ndmath/arithmetics.c:36-947
 *   NDArray_Min / NDArray_Max                    src/ndarray.c:752-772,939-959
 *   reduce()                                     src/ndarray.c:523-578
 *   NDArrayMathGPU_ElementWise{,1F,2F,1N}        src/ndmath/cuda/cuda_math.cu:1532-1558
 *   NDArray_Matmul / NDArray_FMatmul / NDArray_Dot   src/ndmath/linalg.c:44-82,216-245,354-393
 *
 * Device work goes through the C ABI of include/np_hip.h; this library contains no kernels and
 * no CPU arithmetic.  Arrays on NDARRAY_DEVICE_CPU exist only as staging for ->gpu()/->cpu()
 * and as 0-d scalar operands: an arithmetic call whose array operands live on the CPU fails with
 * an error (the reference's CPU path — AVX2/OpenBLAS — stays the reference's own code; this
 * library never computes on the host).
 *
 * Errors: where the reference calls zend_throw_error(NULL, msg) and returns NULL, these
 * functions call the installed error handler with the same message (default: remember it for
 * numpower_host_last_error()) and return NULL.
 */
#ifndef NUMPOWER_AMD_HOST_H
#define NUMPOWER_AMD_HOST_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDARRAY_DEVICE_CPU 0
#define NDARRAY_DEVICE_GPU 1

typedef struct NDArrayDescriptor {
    const char *type;   /* "float32" */
    int elsize;
    long numElements;
} NDArrayDescriptor;

typedef struct NDArray {
    int uuid;
    int *strides;       /* bytes */
    int *dimensions;
    int ndim;
    char *data;         /* host pointer (device == CPU) or device pointer (device == GPU) */
    struct NDArray *base;
    int flags;
    NDArrayDescriptor *descriptor;
    void *iterator;
    void *php_iterator;
    int refcount;
    int device;
} NDArray;

#define NDArray_FDATA(a) ((float *) ((a)->data))
#define NDArray_NDIM(a) ((int) ((a)->ndim))
#define NDArray_SHAPE(a) ((int *) ((a)->dimensions))
#define NDArray_NUMELEMENTS(a) ((long) ((a)->descriptor->numElements))
#define NDArray_DEVICE(a) ((int) ((a)->device))
#define NDArray_ADDREF(a) ((a)->refcount++)          /* src/ndarray.h:31 */

/* ---- errors (zend_throw_error stand-in) ---- */
typedef void (*numpower_error_handler)(const char *message);
void numpower_host_set_error_handler(numpower_error_handler handler);   /* NULL = default */
const char *numpower_host_last_error(void);   /* "" if none since the last clear */
void numpower_host_clear_error(void);

/* ---- allocation / placement ---- */
/* shape is copied (the reference takes ownership of an emalloc'd shape; copying keeps the C API
 * usable from ctypes — the Zend glue frees its own vector). */
NDArray *NDArray_Zeros(const int *shape, int ndim, const char *type, int device);
NDArray *NDArray_Empty(const int *shape, int ndim, const char *type, int device);
NDArray *NDArray_EmptyLike(NDArray *a);
NDArray *NDArray_Copy(NDArray *a, int device);   /* same-device copy (device must equal a's) */
NDArray *NDArray_Fill(NDArray *a, float fill_value);
NDArray *NDArray_CreateFromDoubleScalar(double scalar);
NDArray *NDArray_CreateFromFloatScalar(float scalar);
NDArray *NDArray_CreateFromLongScalar(long scalar);
/* CPU array from a host buffer (stands in for Create_NDArray_FromZval, initializers.c:30-247) */
NDArray *NDArray_FromHostBuffer(const float *host_data, const int *shape, int ndim);
/* View of slice `index` along the leading axis: what $a[i] / NDArrayIterator_GET return
 * (iterators.c:94-111): shares data, base = a, ADDREFs a. */
NDArray *NDArray_LeadingSlice(NDArray *a, int index);
void NDArray_FREE(NDArray *array);
NDArray *NDArray_ToGPU(NDArray *target);
NDArray *NDArray_ToCPU(NDArray *target);
float NDArray_GetFloatScalar(NDArray *a);        /* ndarray.c:1302-1310 */
/* copy numElements floats of a CPU array into host_out (toArray() plumbing) */
int NDArray_CopyToHostBuffer(NDArray *a, float *host_out);
/* live device allocations (vmemcheck, gpu_alloc.c:36-40) */
long NDArray_LiveDeviceAllocations(void);

/* ---- binary elementwise (arithmetics.c:160-926) ---- */
NDArray *NDArray_Add_Float(NDArray *a, NDArray *b);
NDArray *NDArray_Subtract_Float(NDArray *a, NDArray *b);
NDArray *NDArray_Multiply_Float(NDArray *a, NDArray *b);
NDArray *NDArray_Divide_Float(NDArray *a, NDArray *b);
NDArray *NDArray_Mod_Float(NDArray *a, NDArray *b);
NDArray *NDArray_Pow_Float(NDArray *a, NDArray *b);
int NDArray_IsBroadcastable(const NDArray *array1, const NDArray *array2);   /* ndarray.c:1124-1162 */

/* ---- comparisons (src/logic.c:25-670): 1.0f / 0.0f masks ---- */
NDArray *NDArray_Equal(NDArray *nda, NDArray *ndb);
NDArray *NDArray_NotEqual(NDArray *nda, NDArray *ndb);
NDArray *NDArray_Greater(NDArray *nda, NDArray *ndb);
NDArray *NDArray_GreaterEqual(NDArray *nda, NDArray *ndb);
NDArray *NDArray_Less(NDArray *nda, NDArray *ndb);
NDArray *NDArray_LessEqual(NDArray *nda, NDArray *ndb);
/* elementwise fmaxf / fminf with broadcast (ndarray.c:853-931; GPU arrays are refused there) */
NDArray *NDArray_Maximum(NDArray *a, NDArray *b);
NDArray *NDArray_Minimum(NDArray *a, NDArray *b);
float NDArray_All(NDArray *a);   /* 1 / 0, reproduces the reference's CPU result (logic.c:25-58) */

/* ---- layout (src/manipulation.c:68-130) ---- */
typedef struct NDArray_Dims {   /* src/ndarray.h:40-43 */
    int *ptr;
    int len;
} NDArray_Dims;
/* New contiguous array with the axes permuted (NULL = reverse all axes). */
NDArray *NDArray_Transpose(NDArray *a, NDArray_Dims *permute);

/* ---- initializers (src/initializers.c:458-510,655-660,818-841; the reference's benchmarks/initializers) ----
 * Reference names create CPU arrays as in the reference; the ...On variants take the device, so an
 * array can be born on the GPU without a PCIe copy.  NDArray_ArangeOn reproduces the reference's
 * float recurrence bit for bit (np_arange); on NDARRAY_DEVICE_CPU it raises (host arithmetic stays
 * the reference's own code). */
NDArray *NDArray_Ones(const int *shape, int ndim, const char *type);
NDArray *NDArray_Full(const int *shape, int ndim, double fill_value);
NDArray *NDArray_Identity(int size);
NDArray *NDArray_FullOn(const int *shape, int ndim, double fill_value, int device);
NDArray *NDArray_IdentityOn(int size, int device);
NDArray *NDArray_ArangeOn(double start, double stop, double step, int device);

/* ---- views, layout and equality around the path ----
 * NDArray_ArrayEqual   logic.c:703-716      1 / 0 (0 on shape mismatch)
 * NDArray_AllClose     logic.c:750-772      1 / 0, -1 + error on shape / device mismatch (the
 *                                           reference rejects GPU arrays; here it is one reduction)
 * NDArray_ToContiguous manipulation.c:381-421   strided view -> new contiguous array, one launch
 * NDArray_Diagonal     indexing.c:21-48     (`offset` is ignored, as in the reference)
 * NDArray_Trace        linalg.c:758-767     0-d CPU scalar
 * NDArray_Reshape      manipulation.c:138-162   view sharing data (ADDREFs target)
 * NDArray_Flatten      manipulation.c:169-184   1-D copy
 * NDArray_ExpandDim    manipulation.c:453-513   axis: 0-d or 1-D CPU array
 * NDArray_ConcatenateFlat / NDArray_Append  manipulation.c:293-374 (axis must be -1)
 * NDArray_Slice        manipulation.c:193-283   indexes[i] = CPU array [start(,stop(,step))] */
int NDArray_ArrayEqual(NDArray *a, NDArray *b);
int NDArray_AllClose(NDArray *a, NDArray *b, float rtol, float atol);
NDArray *NDArray_ToContiguous(NDArray *a);
/* `a` itself when it is C-contiguous, else a contiguous copy that is also stored in *owned (the caller frees it; *owned is
 * NULL otherwise); NULL after a raised error.  The one contiguity rule of the host layer (host/numpower_linalg.cpp). */
NDArray *numpower_host_contiguous(NDArray *a, NDArray **owned);
NDArray *NDArray_Diagonal(NDArray *target, int offset);
NDArray *NDArray_Trace(NDArray *a);
NDArray *NDArray_Reshape(NDArray *target, int *new_shape, int ndim);
NDArray *NDArray_Flatten(NDArray *target);
NDArray *NDArray_ExpandDim(NDArray *a, NDArray *axis);
NDArray *NDArray_ConcatenateFlat(NDArray **arrays, int num_arrays);
NDArray *NDArray_Append(NDArray **arrays, int axis, int num_arrays);
NDArray *NDArray_Slice(NDArray *array, NDArray **indexes, int num_indices);

/* ---- fused elementwise chains ----
 * Evaluates acc = inputs[0]; acc = op_k(acc [, inputs[operand_k]]) ... in one kernel; `ops` uses
 * np_fused_op of np_hip.h (flags/body_end are filled in here).  Bit-identical to calling the
 * stand-alone entry points one after the other. */
#include "np_hip.h"
NDArray *NDArray_FusedChain(NDArray **inputs, int n_inputs, const np_fused_op *ops, int n_ops);
/* ... ending in a full reduction (np_reduce_op: sum / prod / min / max / mean) of the chain value,
 * which is never written to memory.  Returns NaN and raises on error. */
float NDArray_FusedChainReduce(NDArray **inputs, int n_inputs, const np_fused_op *ops, int n_ops, int reduce_op);
/* ... ending in a reduction over one axis (same `axis` rules and error as reduce(), ndarray.c:534-538): the
 * result has the chain's shape without that axis.  The last axis of any array and the first axis of a
 * 2-d array run as ONE kernel (np_fused_chain_reduce_axis); any other axis evaluates the chain into a
 * temporary and reduces that. */
NDArray *NDArray_FusedChainReduceAxis(NDArray **inputs, int n_inputs, const np_fused_op *ops, int n_ops, int reduce_op,
                                      int axis);

/* ---- argmax / argmin (src/ndmath/calculation.c:73-194) ----
 * axis = 128 (NDARRAY_MAX_DIMS) reduces the flattened array; indices are returned as floats. */
#ifndef __cplusplus
#include <stdbool.h>
#endif
NDArray *NDArray_ArgMinMaxCommon(NDArray *op, int axis, bool keepdims, bool is_argmax);

/* ---- statistics (src/ndmath/statistics.c:88-154): 0-d CPU scalar results ---- */
NDArray *NDArray_Variance(NDArray *a);
NDArray *NDArray_Std(NDArray *a);
NDArray *NDArray_Average(NDArray *a, NDArray *weights /* may be NULL */);

/* ---- unary elementwise: the reference's drivers with the reference's signatures ----
 * (src/ndmath/cuda/cuda_math.h:10-15,75-76; implemented in ext/hip_math_drivers.c).  `op` is one of the
 * cuda_float_* functions of ext/hip_math.h — also exported by this library — exactly as numpower.c
 * passes them: NDArrayMathGPU_ElementWise(nda, cuda_float_sin) (numpower.c:1651).  Recognised pointers
 * run as ONE out-of-place np_unary pass (no NDArray_Copy first); any other pointer gets the reference's
 * copy + in-place call. */
#ifndef NUMPOWER_AMD_EXT_HIP_MATH_H
typedef void (*ElementWiseFloatGPUOperation)(int, float *);
typedef void (*ElementWiseFloatGPUOperation2F)(int, float *, float, float);
typedef void (*ElementWiseFloatGPUOperation1F)(int, float *, float);
typedef void (*ElementWiseFloatGPUOperation1N)(int, float *, float *);
#endif
NDArray *NDArrayMathGPU_ElementWise(NDArray *ndarray, ElementWiseFloatGPUOperation op);
NDArray *NDArrayMathGPU_ElementWise1F(NDArray *ndarray, ElementWiseFloatGPUOperation1F op, float val1);
NDArray *NDArrayMathGPU_ElementWise2F(NDArray *ndarray, ElementWiseFloatGPUOperation2F op, float val1, float val2);
NDArray *NDArrayMathGPU_ElementWise1N(NDArray *ndarray, ElementWiseFloatGPUOperation1N op, NDArray *val1);
NDArray *NDArray_Abs(NDArray *nda);
/* float_rsqrt (double_math.c:111-126) on the device; numpower.c:1791 passes cuda_float_arccos to the
 * driver for GPU arrays by mistake (no cuda_float_rsqrt exists), so rsqrt gets its own entry point */
NDArray *NDArray_Rsqrt(NDArray *nda);
/* float_exp2 (double_math.c:31-33) on the device: the reference has no GPU exp2 at all (numpower.c:3153 maps
 * the CPU kernel over whatever pointer the array holds; cuda_math.h declares no cuda_float_exp2) */
NDArray *NDArray_Exp2(NDArray *nda);

/* ---- reductions ---- */
float NDArray_Sum_Float(NDArray *a);
float NDArray_Float_Prod(NDArray *a);
float NDArray_Mean_Float(NDArray *a);
float NDArray_Min(NDArray *target);
float NDArray_Max(NDArray *target);
/* NDArray_Median_Float  arithmetics.c:149-158 (calculate_median :111-138): (t[n/2-1] + t[n/2]) / 2.0f for an
 *                       even count, t[n/2] for an odd one, t = the sorted elements.
 * NDArray_Quantile      statistics.c:60-79 (calculate_quantile :14-50): q a 0-d array in [0, 1];
 *                       index = (float)(n-1)*q, linear interpolation between t[(int)index] and the next
 *                       element, in the reference build's arithmetic (one fma); errors "Q must be a
 *                       scalar", "Q must be between 0 and 1".  Returns a 0-d array on the device.
 * The reference refuses device arrays for both ("Median not available for GPU.", "Quantile not
 * available for GPU device.") and sorts a host copy; here the two order statistics come from
 * np_order_stat (radix select on the device). */
float NDArray_Median_Float(NDArray *a);

/* ---- manipulation wrappers (manipulation.c:554-1073, initializers.c:597-625), device arrays ----
 * atleast_* / squeeze are views (reshape) of the contiguous input; swapaxes / rollaxis / moveaxis
 * materialise through NDArray_Transpose (np_permute); concatenate is one pitched copy (np_copy2d) per
 * input, v/h/d/column_stack are concatenate over atleast_2d / 1d / 3d / transposed inputs; diag of a
 * vector is a zero fill + one pitched copy, of a matrix its diagonal.  Error messages are the
 * reference's.  Deviations, where the reference is undefined or wrong: atleast_3d of a 2-d array is
 * numpy's (r, c, 1) (the reference overflows a 2-int buffer there); rollaxis / moveaxis follow
 * numpy's definition (the reference's index shuffling is only right for the cases it agrees with). */
NDArray *NDArray_AtLeast1D(NDArray *a);
NDArray *NDArray_AtLeast2D(NDArray *a);
NDArray *NDArray_AtLeast3D(NDArray *a);
NDArray *NDArray_Squeeze(NDArray *a, NDArray *axis);   /* axis: NULL, a CPU 0-d or 1-d array */
NDArray *NDArray_SwapAxes(NDArray *a, int axis1, int axis2);
NDArray *NDArray_Rollaxis(NDArray *a, int axis, int start);
NDArray *NDArray_Moveaxis(NDArray *a, int *src, int *dest, int n_source, int n_dest);
NDArray *NDArray_Concatenate(NDArray **arrays, int narrays, int axis);
NDArray *NDArray_VSTACK(NDArray **arrays, int narrays);
NDArray *NDArray_HSTACK(NDArray **arrays, int narrays);
NDArray *NDArray_DSTACK(NDArray **arrays, int narrays);
NDArray *NDArray_ColumnStack(NDArray **arrays, int narrays);
NDArray *NDArray_Diag(NDArray *a);
NDArray *NDArray_Quantile(NDArray *target, NDArray *q);
/* operation must be NDArray_Add_Float or NDArray_Multiply_Float (the two the reference passes,
 * numpower.c:4637,4742,2661); anything else is an error. */
NDArray *reduce(NDArray *array, int *axis, NDArray *(*operation)(NDArray *, NDArray *));
/* min/max along an axis: the reference's single_reduce path is unreachable/broken
 * (numpower.c:4654 parses one argument; apply_single_reduce writes element 0 only), so these are
 * additions with NumPy semantics. */
NDArray *NDArray_MinAxis(NDArray *target, int axis);
NDArray *NDArray_MaxAxis(NDArray *target, int axis);

/* ---- matmul ---- */
NDArray *NDArray_Matmul(NDArray *a, NDArray *b);
NDArray *NDArray_FMatmul(NDArray *a, NDArray *b);
NDArray *NDArray_Dot(NDArray *nda, NDArray *ndb);
NDArray *NDArray_Outer(NDArray *a, NDArray *b);   /* linalg.c:724-751 */
NDArray *NDArray_Inner(NDArray *nda, NDArray *ndb);   /* linalg.c:310-345: sum of all products */
/* batch x M x K times batch x K x N -> batch x M x N (BASELINE config 5; no reference entry
 * point: linalg.c:239-242 rejects ndim > 2 with "Stack of matrices not allowed") */
NDArray *NDArray_BatchedMatmul(NDArray *a, NDArray *b);

/* ---- the sharded form of the batched matmul (BASELINE config 5) ----
 * One PHP process per GPU (NDArray::setDevice, numpower.c:615-635, picks the process's device; the reference has
 * no multi-device code).  NDArray_CommInit joins the node's ranks (np_comm_init: endpoint "tcp://127.0.0.1:port"
 * or a file path); 0 on success, -1 + a thrown Error otherwise.
 * NDArray_ShardedBatchedMatmul: a_slab [slab x M x K] and b_slab [slab x K x N] are THIS rank's contiguous share of
 * a batch of `batch` = slab * world products (rank r holds matrices r*slab ... (r+1)*slab - 1).
 *   gather_mode  NP_SHARD_KEEP (0)      -> [slab x M x N], this rank's products only: no collective at all
 *                NP_SHARD_GATHER (1)    -> [batch x M x N] replicated on every rank: the GEMM, then ONE all-gather
 *                k >= 2                 -> the same result, slab computed in k pieces, each piece's transfer
 *                                          overlapped with the next piece's GEMM (np_sgemm_strided_batched_allgather)
 *                NP_SHARD_OVERLAP (-1)  -> the same, the number of pieces chosen by the library's step model (chunks = 0):
 *                                          what a caller without a reason of its own passes
 * Without a communicator the process is a world of one: batch must equal slab.  Errors (thrown like every other
 * method's): device mismatch / shape mismatch with NDArray_Matmul's messages (linalg.c:219-237),
 * "Batch of %d is not %d slab(s) of %d" when the shares do not add up. */
#define NP_SHARD_KEEP 0
#define NP_SHARD_GATHER 1
#define NP_SHARD_OVERLAP (-1)
int NDArray_CommInit(int rank, int world, const char *endpoint);
int NDArray_CommDestroy(void);
int NDArray_CommRank(void);
int NDArray_CommWorld(void);
NDArray *NDArray_ShardedBatchedMatmul(NDArray *a_slab, NDArray *b_slab, int batch, int gather_mode);

/* ---- dense linear algebra on the LU (host/numpower_linalg.cpp; linalg.c:253, 584, 620, 981) ----
 * GPU operands only (the CPU path is the reference's own LAPACK calls).  Strided views are made contiguous
 * (numpower_host_contiguous), then ext/hip_linalg.c does the work — the same code a --with-hip tree runs.
 * NDArray_Det     0-d GPU array: the product of U's diagonal in index order, the pivot parity's sign, 0 when singular
 * NDArray_Inverse a^-1; singular -> "LU factorization failed. Unable to compute the matrix inverse.\n"
 * NDArray_LU      malloc'd vector {P, L, U} with P a = L U (the caller free()s the vector, the reference efree()s it)
 * NDArray_Solve   x with a x = b, b n x k (any k); singular -> the same throw as NDArray_Inverse
 * Shape errors: "Array must be at least two-dimensional", "Array must be square", "Incompatible shapes",
 * "Both NDArray must be in the same device." (the reference's messages). */
NDArray *NDArray_Det(NDArray *a);
NDArray *NDArray_Inverse(NDArray *target);
NDArray **NDArray_LU(NDArray *target);
NDArray *NDArray_Solve(NDArray *a, NDArray *b);

/* ---- Cholesky factorization (host/numpower_linalg.cpp; linalg.c:1056-1102) ----
 * NDArray_Cholesky  the lower-triangular L with a = L L^T, strict upper triangle +0.0f; only the lower triangle of a
 *                   is read (the reference: LAPACKE_spotrf(ROW_MAJOR, 'L') on a copy).  GPU operands only, views made
 *                   contiguous; ext/hip_linalg.c (NPH_Cholesky) does the work.
 * Errors: "NDArray_Cholesky: $a must be a square matrix." for a non-square or non-2-D operand,
 * "Error calculating the cholesky decomposition. (Is $a not positive definite?)" when a pivot is not positive. */
NDArray *NDArray_Cholesky(NDArray *a);

/* ---- singular value decomposition (host/numpower_linalg.cpp; linalg.c:111-209, 402-470, 668-715, 1038-1050) ----
 * GPU operands only, views made contiguous; the device Jacobi SVD (np_svd / np_svdvals) does the work.
 * NDArray_SVD         malloc'd vector {U (m, m), S (k), V (n, n)}, k = min(m, n): the thin factors in the leading k columns of U
 *                     and the leading k rows of V (rows of V are right singular vectors, as on the reference's CPU path),
 *                     +0.0f elsewhere, S descending.  1-d: "Array must be at least two-dimensional"; ndim > 2 is refused.
 * NDArray_MatrixRank  a 0-d array: how many singular values are > tol (default s_max max(m, n) FLT_EPSILON when tol is NULL)
 * NDArray_Norm        type 2: the largest singular value as a 0-d GPU array; type 1 is refused for GPU arrays; any other
 *                     type: "NDArray_Norm: The provided norm `%d` is invalid"
 * NDArray_Cond        norm2(a) norm2(inv(a)); a singular a raises NDArray_Inverse's message */
NDArray **NDArray_SVD(NDArray *target);
NDArray *NDArray_MatrixRank(NDArray *target, float *tol);
NDArray *NDArray_Norm(NDArray *target, int type);
NDArray *NDArray_Cond(NDArray *a);

/* ---- symmetric eigendecomposition (host/numpower_linalg.cpp; linalg.c:795-838) ----
 * NDArray_Eig  malloc'd vector {eigenvalues (n) ascending, eigenvectors (n, n), eigenvector j in column j}: the order and shapes
 *              of the reference's CPU path.  GPU operands only, views made contiguous; the device Jacobi eigensolver (np_eigh)
 *              does the work, and it is a SYMMETRIC eigensolver: a matrix with a[i][j] != a[j][i] anywhere is refused with a
 *              message that says so (a general matrix goes through ->cpu() in a patched tree).
 * Errors: "Error: Input matrix is not square.\n" for a non-square or non-2-D operand; the not-symmetric refusal; a message
 * that names the sweep cap when the iteration did not converge. */
NDArray **NDArray_Eig(NDArray *a);

/* ---- Householder QR and least squares (host/numpower_linalg.cpp; linalg.c:848-899, 908-970) ----
 * NDArray_Qr     malloc'd vector {Q (m, n), R (n, n)} for a (m, n) with m >= n: the reduced factorization (np_qr), Q^T Q = I,
 *                Q R = a, R upper triangular with a strict lower triangle of +0.0f and a diagonal of either sign.  NOT what the
 *                reference's CPU path returns: that calls sgeqrf without sorgqr and hands the packed reflectors back as Q.
 * NDArray_Lstsq  x (n, nrhs) minimising ||a x - b|| for a (m, n), m >= n, and b (m, nrhs) (np_lstsq).
 * GPU operands only, views made contiguous.  Errors: qr of a non-2-D operand or with m < n (this project's messages; the
 * reference returns NULL without one); "Invalid dimensions to calculate lstsq, both arrays must have 2 dimensions and $b must
 * contain the same amount of rows as $a"; "The diagonal element %i of the triangular factor of $a is zero, so that $a does not
 * have full rank."; lstsq with one operand on each device or with m < n is refused. */
NDArray **NDArray_Qr(NDArray *a);
NDArray *NDArray_Lstsq(NDArray *a, NDArray *b);

/* ---- 2-D correlation and convolution (host/numpower_signal.cpp; signal.c:217-303) ----
 * NDArray_Correlate2D  scipy.signal.correlate2d(a, b, mode, boundary, fillvalue) of two 2-D GPU arrays, with flip != 0
 *                      scipy.signal.convolve2d; mode 0 valid / 1 same / 2 full, boundary 0 fill / 4 symm / 8 wrap (signal.h).
 *                      fill_value: NULL (0) or an array with one element on either device, read under boundary 0 only.
 *                      Views are made contiguous; ext/hip_signal.c (NPH_Correlate2D, np_correlate2d) does the work.  A new
 *                      GPU array of SciPy's shape: 'full' (ah + bh - 1, aw + bw - 1), 'same' a's, 'valid' |a - b| + 1 with
 *                      the operands changing places when a does not cover b (DESIGN.md §3.11 lists where the
 *                      reference's CPU wrapper differs).
 * Errors: "NDArray::correlate2d inputs must be both 2-D arrays", "For 'valid' mode, one input must be at least as large as
 * the other in every dimension", "fillValue must be a scalar or an array with one element.", "invalid mode.", for one
 * operand on each device "correlate2d not implemented for GPU computation.", for two CPU operands "... only computes on
 * the GPU". */
NDArray *NDArray_Correlate2D(NDArray *a, NDArray *b, int mode, int boundary, NDArray *fill_value, int flip);

/* ---- convolution layers (host/numpower_dnn.cpp; dnn.c:273-368, dnn.h:7-8) ----
 * NDArrayDNN_Conv2D_Forward   y (N, F, H - kh + 1, W - kw + 1) of a GPU input x (N, C, H, W) and GPU filters (F, C, kh, kw):
 *                             cross-correlation, stride 1, no padding, no bias, no activation.
 * NDArrayDNN_Conv2D_Backward  for y = the gradient of that result: a malloc'd vector {dW (F, C, kh, kw), dX (N, C, H, W)}, the
 *                             reference's order.
 * The reference's signatures; kernel_size, activation and use_bias are ignored (the reference ignores the last two on both of
 * its paths; PHP passes NULL / 3, 'r', 1).  Views are made contiguous; ext/hip_dnn.c (NPH_Conv2D_Forward / _Backward over
 * np_conv2d_forward / _backward_filter / _backward_data) does the work.  DESIGN.md §3.14 lists where the reference's CPU path
 * differs: F is shape[0], kh != kw is allowed, dW has the filters' own shape.
 * Errors (ext/hip_dnn.h, NPH_DNN_MSG_*): operands that are not 4-dimensional, a channel mismatch, a window larger than the input,
 * a gradient of the wrong shape, operands on different devices, and for CPU operands "... only computes on the GPU": the host
 * library has no CPU convolution. */
NDArray *NDArrayDNN_Conv2D_Forward(NDArray *x, NDArray *filters, int *kernel_size, char activation, int use_bias);
NDArray **NDArrayDNN_Conv2D_Backward(NDArray *input, NDArray *y, NDArray *filters, int kernel_size, char activation, int use_bias);
/* The same layer with a window stride, a zero padding and a tap dilation, each (rows, columns), NULL meaning (1, 1), (0, 0),
 * (1, 1): y (N, F, oh, ow), oh = floor((H + 2 ph - keh) / sh) + 1 with the effective window keh = dh (kh - 1) + 1.  The reference
 * has no such functions (its layer names the three and hard-wires stride 1, no padding: dnn.c:196-200).  Views are made
 * contiguous; NPH_Conv2D_ForwardEx / _BackwardEx over np_conv2d_*_ex do the work.  Errors as above, with NPH_DNN_MSG_STRIDE,
 * _DILATION, _PADDING, _EFFECTIVE and _STRIDED_GRADIENT in place of the window and gradient messages. */
NDArray *NDArrayDNN_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int *stride, const int *padding, const int *dilation);
NDArray **NDArrayDNN_Conv2D_BackwardEx(NDArray *input, NDArray *y, NDArray *filters, const int *stride, const int *padding, const int *dilation);
/* The layer with a bias per filter and an activation: y = act(conv(x, filters) + bias[f]), the bias ONE fp32 add after the
 * reduction, the activation applied in the forward kernel (np_conv2d_forward_act).  bias: a 1-D GPU array (F,) or NULL;
 * activation: 'r' relu, 't' tanh, 's' sigmoid, 'n' or 0 none.  _LayerBackward takes `out`, the forward result (gradients are
 * expressed through the output; NULL is allowed without an activation), and dy, the gradient of that result, and returns a
 * malloc'd vector of THREE: dW, dX (the reference's order) and db (F,), which is NULL without use_bias.  Views are made
 * contiguous; NPH_Conv2D_LayerForward / _LayerBackward do the work.  Errors as for the Ex functions, and before them
 * NPH_DNN_MSG_ACTIVATION, _BIAS, _OUT and _BIAS_DEVICE.  The reference-signature functions above still ignore `activation` and
 * `use_bias`. */
NDArray *NDArrayDNN_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int *stride, const int *padding, const int *dilation,
                                        char activation);
NDArray **NDArrayDNN_Conv2D_LayerBackward(NDArray *input, NDArray *out, NDArray *dy, NDArray *filters, const int *stride, const int *padding,
                                          const int *dilation, char activation, int use_bias);
/* Pooling (host/numpower_dnn.cpp; the reference has none): y (N, C, oh, ow) of a GPU input x (N, C, H, W), pooled as N.C planes.
 * kernel (kh, kw); stride (sh, sw), NULL meaning the window; padding (ph, pw), NULL meaning 0, with 2 ph <= kh and 2 pw <= kw;
 * mode 'm' max (the first of equal maxima, a NaN wins), 'a' average with divisor kh.kw (padding counts), 'v' average over the real
 * cells.  oh = floor((H + 2 ph - kh) / sh) + 1; no dilation, no ceil mode.  _Backward takes the layer's input x and dy, the
 * gradient of the result, and returns dx (N, C, H, W): a gather in a fixed order, no float atomics; cells no window covers get +0.
 * Views are made contiguous; NPH_Pool2D_Forward / _Backward over np_pool2d_forward / _backward do the work.  Errors (ext/hip_dnn.h,
 * NPH_POOL_MSG_*): an unknown mode, operands that are not 4-dimensional, a window, stride or padding out of range, a window larger
 * than the padded input, a gradient of the wrong shape, operands on different devices, and CPU operands. */
NDArray *NDArrayDNN_Pool2D_Forward(NDArray *x, const int *kernel, const int *stride, const int *padding, char mode);
NDArray *NDArrayDNN_Pool2D_Backward(NDArray *x, NDArray *dy, const int *kernel, const int *stride, const int *padding, char mode);
/* Softmax, log-softmax and cross-entropy (host/numpower_dnn.cpp; the reference has none): GPU operands of any ndim >= 1, the
 * softmax along `axis` (negative axes count from the end); mode 's' softmax, 'l' log-softmax.  _Backward works from the forward
 * OUTPUT y and its gradient dy.  NDArrayDNN_CrossEntropy takes logits (rows, classes) and a target of (rows) class indices
 * stored as fp32 or (rows, classes) probabilities; reduction 'n' none ((rows) losses), 's' sum, 'm' mean (0-dimensional
 * results); with_grad: *dlogits receives (softmax - target) . scale, scale = 1 / rows for the mean and 1 otherwise, from the same
 * launch.  An invalid label gives NaN for its row alone.  Views are made contiguous; NPH_Softmax_Forward / _Backward and
 * NPH_CrossEntropy over np_softmax_forward / _backward and np_cross_entropy do the work.  Errors (ext/hip_dnn.h,
 * NPH_SOFTMAX_MSG_*, NPH_XENT_MSG_*): an unknown mode, an axis out of range, a gradient of another shape, logits that are not
 * 2-dimensional, a target of neither shape, an unknown reduction, operands on different devices, and CPU operands. */
NDArray *NDArrayDNN_Softmax_Forward(NDArray *x, int axis, char mode);
NDArray *NDArrayDNN_Softmax_Backward(NDArray *y, NDArray *dy, int axis, char mode);
NDArray *NDArrayDNN_CrossEntropy(NDArray *logits, NDArray *target, char reduction, int with_grad, NDArray **dlogits);
/* Batch normalization (host/numpower_dnn.cpp; the reference has none): GPU operands, x of ndim >= 2 with the channel on axis 1,
 * gamma / beta / running_mean / running_var (C) arrays or NULL.  training != 0: a vector of three new arrays (y, save_mean,
 * save_invstd), the running statistics updated in place when given (momentum in [0, 1]; they must be contiguous arrays);
 * training == 0: both running statistics are required, the vector holds y and two NULLs.  _Backward is training mode's backward
 * pass from x, dy, gamma (or NULL) and the saved statistics: a vector (dx, dgamma, dbeta).  The caller frees the vector.  Views are
 * made contiguous; NPH_BatchNorm_Forward / _Backward over np_batchnorm_forward / _backward do the work.  Errors (ext/hip_dnn.h,
 * NPH_BN_MSG_*): ndim < 2, gamma, beta or statistics that are not (C), inference without running statistics, a gradient of another
 * shape, eps < 0, momentum outside [0, 1], operands on different devices, CPU operands, one value per channel in training. */
NDArray **NDArrayDNN_BatchNorm_Forward(NDArray *x, NDArray *gamma, NDArray *beta, NDArray *running_mean, NDArray *running_var, int training,
                                       double momentum, double eps);
NDArray **NDArrayDNN_BatchNorm_Backward(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd);
/* Layer and group normalization (host/numpower_dnn.cpp; the reference has none): GPU operands.  Layer normalization takes the
 * normalized_ndim trailing extents of x as normalized_shape; gamma and beta have that shape or are NULL; the statistics have the
 * shape of the leading axes ((1) without one).  Group normalization takes x of ndim >= 2 with the channel on axis 1 and
 * num_groups dividing C; gamma and beta are (C) arrays or NULL; the statistics are (N, num_groups); instance normalization is
 * num_groups = C.  _Forward: a vector of three new arrays (y, save_mean, save_invstd); _Backward, from x, dy, gamma (or NULL) and
 * the saved statistics: (dx, dgamma, dbeta).  The caller frees the vector.  Views are made contiguous; NPH_LayerNorm_* and
 * NPH_GroupNorm_* over np_groupnorm_forward / _backward do the work.  Errors: ext/hip_dnn.h, NPH_LN_MSG_* and NPH_GN_MSG_*. */
NDArray **NDArrayDNN_LayerNorm_Forward(NDArray *x, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *beta, double eps);
NDArray **NDArrayDNN_LayerNorm_Backward(NDArray *x, NDArray *dy, const int *normalized_shape, int normalized_ndim, NDArray *gamma,
                                        NDArray *save_mean, NDArray *save_invstd);
NDArray **NDArrayDNN_GroupNorm_Forward(NDArray *x, int num_groups, NDArray *gamma, NDArray *beta, double eps);
NDArray **NDArrayDNN_GroupNorm_Backward(NDArray *x, NDArray *dy, int num_groups, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd);
/* Scaled dot-product attention (host/numpower_dnn.cpp; the reference has none): GPU operands q (..., Sq, D), k and v (..., Sk, D)
 * with equal leading axes, D <= 128.  causal masks the keys above the row (top-left alignment).  scale: a value that is not greater
 * than zero, or a NaN, means 1 / sqrt(D).  _Forward: a vector of three new arrays (o, save_max, save_sum), the statistics in q's
 * shape without its last axis; _Backward, from q, k, v, o, the gradient dout of o and the saved statistics: (dq, dk, dv).  The caller
 * frees the vector.  Views are made contiguous; NPH_Attention_* over np_attention_forward / _backward do the work.  Errors:
 * ext/hip_dnn.h, NPH_ATTN_MSG_*. */
NDArray **NDArrayDNN_Attention_Forward(NDArray *q, NDArray *k, NDArray *v, int causal, float scale);
NDArray **NDArrayDNN_Attention_Backward(NDArray *q, NDArray *k, NDArray *v, NDArray *o, NDArray *dout, NDArray *save_max, NDArray *save_sum,
                                        int causal, float scale);
/* Optimizer steps (host/numpower_dnn.cpp; the reference has none): GPU operands in lists, entry t of each list belonging to
 * tensor t.  _SGD_Step is torch.optim.SGD's update (bufs may be NULL with n_bufs = 0 when momentum == 0; first_step != 0 sets the
 * buffers to the gradients), _Adam_Step torch.optim.Adam's, and AdamW's when decoupled != 0 (step >= 1 counts the updates).
 * Parameters and states are updated in place and must be contiguous arrays; gradients may be views, which are made contiguous.
 * grad_scale (or NULL) is a GPU array whose element grad_scale_index multiplies every gradient, read on the device.  Both return 1,
 * or 0 after an error.  _GradNorm returns a new (2) array: the norm of all the gradients and the coefficient
 * min(1, max_norm / (norm + 1e-6)) that, passed as (grad_scale, 1), clips by the norm.  NPH_SGD_Step, NPH_Adam_Step and NPH_GradNorm
 * over np_sgd_step, np_adam_step and np_grad_norm do the work.  Errors: ext/hip_dnn.h, NPH_OPTIM_MSG_*. */
int NDArrayDNN_SGD_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **bufs, int n_bufs, double lr, double momentum,
                        double dampening, double weight_decay, int nesterov, int first_step, NDArray *grad_scale, int grad_scale_index);
int NDArrayDNN_Adam_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **exp_avg, int n_exp_avg, NDArray **exp_avg_sq,
                         int n_exp_avg_sq, long step, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                         NDArray *grad_scale, int grad_scale_index);
NDArray *NDArrayDNN_GradNorm(NDArray **grads, int n_grads, double max_norm);
/* Dense layers (host/numpower_dnn.cpp; the reference has none): GPU operands in torch's layout, x (..., K) with its leading axes
 * flattened to rows, weight (N, K), bias a 1-D (N,) array or NULL; y = act(x . weight^T + bias), the bias ONE fp32 add after the
 * reduction, activation 'r' relu, 't' tanh, 's' sigmoid, 'n' or 0 none, all in one kernel.  _Backward takes `out`, the forward
 * result (NULL is allowed without an activation), and dy, its gradient, and returns a malloc'd vector of THREE in the conv
 * layer's order: dW (N, K), dX in x's shape (NULL without need_dx: a first layer does not pay for it) and db (N,) (NULL without
 * use_bias).  The caller frees the vector.  Views are made contiguous; NPH_Linear_Forward / _Backward over np_linear_forward /
 * _backward do the work.  Errors: ext/hip_dnn.h, NPH_LINEAR_MSG_*. */
NDArray *NDArrayDNN_Linear_Forward(NDArray *x, NDArray *weight, NDArray *bias, char activation);
NDArray **NDArrayDNN_Linear_Backward(NDArray *x, NDArray *out, NDArray *dy, NDArray *weight, char activation, int use_bias, int need_dx);

#ifdef __cplusplus
}
#endif

#endif /* NUMPOWER_AMD_HOST_H */
