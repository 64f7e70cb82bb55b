/*
 * hip_linalg.h — det / inv / lu / solve of GPU arrays on the device LU (np_getrf / np_getrs of include/np_hip.h), and
 * cholesky on the device Cholesky factorization (np_cholesky).
 *
 * The reference computes these with LAPACK on the CPU and, under --with-cuda, through cuSOLVER / its own kernel
 * (cuda_math.cu); its NDArray_Solve refuses GPU arrays.  tools/apply_with_hip.py inserts an early-out into each of the
 * four functions of src/ndmath/linalg.c:
 *
 *     NDArray_Det      at the top                                   return NPH_Det(a);
 *     NDArray_Inverse  at the top                                   return NPH_Inverse(target);
 *     NDArray_LU       behind its shape checks and result arrays   NPH_LU(target, p, l, u), then its own rtns[]
 *     NDArray_Solve    behind its device check, before its GPU throw  return NPH_Solve(a, b);
 *
 *
 * and one into NDArray_Cholesky, which the reference leaves "@todo Implement GPU":
 *
 *     NDArray_Cholesky at the top, before its GPU throw             return NPH_Cholesky(a);
 *
 * and one into NDArray_SVD, whose GPU branch calls cuSOLVER under --with-cuda and returns NULL without it:
 *
 *     NDArray_SVD      at the top                                   return NPH_SVD(target);
 *
 * (NDArray_MatrixRank, NDArray_L2Norm and NDArray_Cond are host code over NDArray_SVD and work for GPU arrays with it.)
 *
 * and, only under the tool's --eig, one into NDArray_Eig, whose GPU branch throws "GPU eig currently unavailable":
 *
 *     NDArray_Eig      behind its squareness check, before its first allocation   return NPH_Eig(a);
 *
 * and, only under the tool's --qr, one each into NDArray_Lstsq and NDArray_Qr, in front of their "not implemented for GPU" throws:
 *
 *     NDArray_Lstsq    at the top, before its GPU throw             return NPH_Lstsq(a, b);
 *     NDArray_Qr       at the top, before its GPU throw             return NPH_Qr(a);
 *
 * each guarded by `#ifdef HAVE_NP_HIP` and NPH_LINALG_TAKES: CPU operands fall through to the reference's LAPACK code.
 * The cuda_det_float / cuda_matrix_float_inverse stubs of hip_math.c are never reached in such a tree.
 *
 * Plain C over the reference's headers in a PHP build (results are the reference's own arrays and die in its
 * NDArray_FREE), over include/numpower_host.h in libnumpower_host.so, whose NDArray_Det / Inverse / LU / Solve call
 * these functions after making their operands contiguous.  Operands must be contiguous (the reference's arrays are).
 * Errors: the reference's messages (linalg.c:123-125, 488-490, 577-588, 981-995, 1063, 1072); NULL / 0 after a raised error.
 */
#ifndef NUMPOWER_AMD_EXT_HIP_LINALG_H
#define NUMPOWER_AMD_EXT_HIP_LINALG_H

#ifdef __cplusplus
extern "C" {
#endif

struct NDArray;

/* true when the early-out takes the call: the (first) operand lives on the GPU */
#define NPH_LINALG_TAKES(a) (NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU)

/* a 0-d GPU array: the product of U's diagonal in index order, the pivot parity's sign, 0 when singular */
struct NDArray *NPH_Det(struct NDArray *a);
/* a^-1; a singular a raises "LU factorization failed. Unable to compute the matrix inverse.\n" */
struct NDArray *NPH_Inverse(struct NDArray *a);
/* p, l, u (n x n GPU arrays the caller allocated) := P, L, U with P a = L U; 1 on success, 0 after a raised error */
int NPH_LU(struct NDArray *a, struct NDArray *p, struct NDArray *l, struct NDArray *u);
/* x with a x = b, b n x k (any k); singular: the same throw as NPH_Inverse */
struct NDArray *NPH_Solve(struct NDArray *a, struct NDArray *b);
/* the lower-triangular L with a = L L^T (upper triangle +0.0f), from a's lower triangle alone; not square:
 * "NDArray_Cholesky: $a must be a square matrix."; a pivot that is not positive:
 * "Error calculating the cholesky decomposition. (Is $a not positive definite?)" */
struct NDArray *NPH_Cholesky(struct NDArray *a);
/* the vector {U (m, m), S (k), V (n, n)}, k = min(m, n), allocated the way the host allocates result vectors: the thin
 * factors of np_svd in the leading k columns of U and the leading k rows of V (V holds the right singular vectors as ROWS,
 * as on the reference's CPU path), +0.0f elsewhere, so U diag(S, 0) V = a.  1-d: "Array must be at least two-dimensional";
 * other ranks are refused (the reference reads the first two extents). */
struct NDArray **NPH_SVD(struct NDArray *a);
/* the vector {eigenvalues (n), eigenvectors (n, n)} of a SYMMETRIC a, allocated as NPH_SVD allocates its own: the order and
 * shapes of the reference's CPU path (linalg.c:800-837), eigenvalues ascending, eigenvector j in column j (np_eigh).  Not 2-d
 * or not square: "Error: Input matrix is not square.\n"; a[i][j] != a[j][i] anywhere: refused, the message says that the device
 * solver is a symmetric eigensolver and that a general matrix goes through ->cpu(); the sweep cap reached: a message that names it. */
struct NDArray **NPH_Eig(struct NDArray *a);
/* the vector {Q (m, n), R (n, n)} of a (m, n) with m >= n, allocated as NPH_SVD allocates its own: the reduced factorization
 * (np_qr), Q with orthonormal columns, R upper triangular with a strict lower triangle of +0.0f and a diagonal of either sign.
 * Not the reference's CPU result, which holds the packed reflectors in place of Q.  Not 2-d, or m < n: an error with a message
 * of this project's (the reference returns NULL without one). */
struct NDArray **NPH_Qr(struct NDArray *a);
/* x (n, nrhs) minimising ||a x - b|| for a (m, n), m >= n, and b (m, nrhs) (np_lstsq).  Shapes: "Invalid dimensions to calculate
 * lstsq, both arrays must have 2 dimensions and $b must contain the same amount of rows as $a"; a zero on R's diagonal: "The
 * diagonal element %i of the triangular factor of $a is zero, so that $a does not have full rank."; one operand on each
 * device and m < n are refused. */
struct NDArray *NPH_Lstsq(struct NDArray *a, struct NDArray *b);

#ifdef __cplusplus
}
#endif
#endif
