/*
 * hip_linalg.c — the device side of NDArray_Det / Inverse / LU / Solve / Cholesky / SVD / Eig / Qr / Lstsq (hip_linalg.h).  Compiled into a --with-hip tree
 * against the reference's headers (-DNUMPOWER_NDARRAY_HEADER='"src/initializers.h"') and into libnumpower_host.so
 * against include/numpower_host.h; it uses only what both declare, with one switch: the reference's arrays take ownership of
 * an emalloc'd shape and its result vectors are emalloc'd, the host library copies shapes and hands out malloc'd vectors.
 */
#ifndef NUMPOWER_NDARRAY_HEADER
#define NUMPOWER_NDARRAY_HEADER "numpower_host.h"
#endif
#include NUMPOWER_NDARRAY_HEADER

#include <stddef.h>
#include <stdio.h>

#include "hip_linalg.h"
#include "np_ext_hooks.h"
#include "np_hip.h"

#ifdef NUMPOWER_AMD_HOST_H
#include <stdlib.h>
#define NPH_ALLOC(bytes) malloc(bytes)
#define NPH_RELEASE(ptr) free(ptr)
#define NPH_SHAPE_IS_COPIED 1
#else
#define NPH_ALLOC(bytes) emalloc(bytes)
#define NPH_RELEASE(ptr) efree(ptr)
#define NPH_SHAPE_IS_COPIED 0
#endif

static const char kSingular[] = "LU factorization failed. Unable to compute the matrix inverse.\n";   /* linalg.c:488-490 */

static int on_gpu(const NDArray *a) {
    if (NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU) return 1;
    np_ext_throw("linear algebra: operand is on the CPU; numpower_amd only computes on the GPU "
                 "(call ->gpu() first, the CPU path is the reference's own)");
    return 0;
}

/* linalg.c:577-588, 614-622 */
static int square(const NDArray *a) {
    if (NDArray_NDIM(a) != 2) {
        np_ext_throw("Array must be at least two-dimensional");
        return 0;
    }
    if (NDArray_SHAPE(a)[0] != NDArray_SHAPE(a)[1]) {
        np_ext_throw("Array must be square");
        return 0;
    }
    return 1;
}

NDArray *NPH_Det(NDArray *a) {
    if (a == NULL || !square(a) || !on_gpu(a)) return NULL;
    NDArray *scalar = NDArray_CreateFromFloatScalar(0.0f);
    if (scalar == NULL) return NULL;
    NDArray *rtn = NDArray_ToGPU(scalar);                      /* a 0-d GPU array, as the reference's GPU det returns */
    NDArray_FREE(scalar);
    if (rtn == NULL) return NULL;
    if (np_det(NDArray_FDATA(a), (size_t) NDArray_SHAPE(a)[0], NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray *NPH_Inverse(NDArray *a) {
    if (a == NULL || !square(a) || !on_gpu(a)) return NULL;
    NDArray *rtn = NDArray_EmptyLike(a);
    if (rtn == NULL) return NULL;
    int info = 0;
    if (np_inverse(NDArray_FDATA(a), (size_t) NDArray_SHAPE(a)[0], NDArray_FDATA(rtn), &info) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    if (info > 0) {
        np_ext_throw(kSingular);
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

int NPH_LU(NDArray *a, NDArray *p, NDArray *l, NDArray *u) {
    if (a == NULL || p == NULL || l == NULL || u == NULL || !square(a) || !on_gpu(a)) return 0;
    if (np_lu(NDArray_FDATA(a), (size_t) NDArray_SHAPE(a)[0], NDArray_FDATA(p), NDArray_FDATA(l), NDArray_FDATA(u)) != NP_OK) {
        np_ext_throw_last();
        return 0;
    }
    return 1;
}

NDArray *NPH_Solve(NDArray *a, NDArray *b) {
    if (a == NULL || b == NULL) return NULL;
    if (NDArray_DEVICE(a) != NDArray_DEVICE(b)) {                  /* linalg.c:982-985 */
        np_ext_throw("Both NDArray must be in the same device.");
        return NULL;
    }
    if (NDArray_NDIM(a) != 2 || NDArray_NDIM(b) != 2 || NDArray_SHAPE(a)[0] != NDArray_SHAPE(a)[1] ||
        NDArray_SHAPE(a)[0] != NDArray_SHAPE(b)[0]) {                 /* linalg.c:995-998 */
        np_ext_throw("Incompatible shapes");
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    NDArray *rtn = NDArray_EmptyLike(b);
    if (rtn == NULL) return NULL;
    int info = 0;
    if (np_solve(NDArray_FDATA(a), NDArray_FDATA(b), (size_t) NDArray_SHAPE(a)[0], (size_t) NDArray_SHAPE(b)[1],
                 NDArray_FDATA(rtn), &info) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    if (info > 0) {
        np_ext_throw(kSingular);
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray *NPH_Cholesky(NDArray *a) {
    if (a == NULL) return NULL;
    if (NDArray_NDIM(a) != 2 || NDArray_SHAPE(a)[0] != NDArray_SHAPE(a)[1]) {   /* linalg.c:1062-1065 */
        np_ext_throw("NDArray" "_Cholesky: $a must be a square matrix.");   /* split: this file names only functions it may call */
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    NDArray *rtn = NDArray_EmptyLike(a);
    if (rtn == NULL) return NULL;
    int info = 0;
    if (np_cholesky(NDArray_FDATA(a), (size_t) NDArray_SHAPE(a)[0], NDArray_FDATA(rtn), &info) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    if (info > 0) {                                                              /* linalg.c:1070-1074 */
        NDArray_FREE(rtn);
        np_ext_throw("Error calculating the cholesky decomposition. (Is $a not positive definite?)");
        return NULL;
    }
    return rtn;
}

/* a zero-filled fp32 GPU array of ndim (1 or 2) dimensions */
static NDArray *zeros_on_gpu(int ndim, int d0, int d1) {
    int *shape = (int *) NPH_ALLOC(sizeof(int) * 2);
    if (shape == NULL) return NULL;
    shape[0] = d0;
    shape[1] = d1;
    NDArray *rtn = NDArray_Zeros(shape, ndim, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

NDArray **NPH_SVD(NDArray *a) {
    if (a == NULL) return NULL;
    if (NDArray_NDIM(a) == 1) {                                                  /* linalg.c:122-125 */
        np_ext_throw("Array must be at least two-dimensional");
        return NULL;
    }
    if (NDArray_NDIM(a) != 2) {   /* the reference reads the first two extents of whatever it is given */
        np_ext_throw("svd: only two-dimensional GPU arrays are supported (batches of matrices are not)");
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    const int m = NDArray_SHAPE(a)[0], n = NDArray_SHAPE(a)[1], k = m < n ? m : n;
    /* the reference's shapes (linalg.c:171-184): U (m, m), S (k), V (n, n); the thin factors fill the leading k columns of U
     * and the leading k rows of V, the rest is +0.0f */
    NDArray *u = zeros_on_gpu(2, m, m), *s = zeros_on_gpu(1, k, 0), *v = zeros_on_gpu(2, n, n);
    NDArray *thin = (m > n) ? zeros_on_gpu(2, m, k) : NULL;                      /* m x k does not sit in m x m as it is */
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    int ok = u != NULL && s != NULL && v != NULL && rtns != NULL && (m <= n || thin != NULL);
    int info = 0;
    if (ok && np_svd(NDArray_FDATA(a), (size_t) m, (size_t) n, NDArray_FDATA(thin != NULL ? thin : u), NDArray_FDATA(s),
                     NDArray_FDATA(v), &info) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (ok && thin != NULL &&
        np_copy2d(NDArray_FDATA(u), (size_t) m, NDArray_FDATA(thin), (size_t) k, (size_t) k, (size_t) m) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (thin != NULL) NDArray_FREE(thin);
    if (!ok) {   /* info > 0 (the sweep cap) is no error: the factors still reconstruct a, as cuSOLVER's gesvdj reports it */
        if (u != NULL) NDArray_FREE(u);
        if (s != NULL) NDArray_FREE(s);
        if (v != NULL) NDArray_FREE(v);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = u;
    rtns[1] = s;
    rtns[2] = v;
    return rtns;
}

NDArray **NPH_Eig(NDArray *a) {
    if (a == NULL) return NULL;
    if (NDArray_NDIM(a) != 2 || NDArray_SHAPE(a)[0] != NDArray_SHAPE(a)[1]) {   /* linalg.c:796-799 */
        np_ext_throw("Error: Input matrix is not square.\n");
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    const int n = NDArray_SHAPE(a)[0];
    int asymmetric = 0;
    if (np_symmetry_mismatch(NDArray_FDATA(a), (size_t) n, &asymmetric) != NP_OK) {
        np_ext_throw_last();
        return NULL;
    }
    if (asymmetric) {   /* np_eigh would answer from the lower triangle alone: a wrong answer to the question that was asked */
        np_ext_throw("eig: the matrix is not symmetric; the device solver is a symmetric eigensolver (real eigenvalues, "
                     "orthonormal eigenvectors), a general matrix goes through ->cpu() and the reference's own LAPACK path");
        return NULL;
    }
    /* the reference's shapes and order (linalg.c:800-837): rtn[0] the eigenvalues (n), rtn[1] the eigenvectors (n, n),
     * eigenvector j in column j */
    NDArray *w = zeros_on_gpu(1, n, 0), *v = zeros_on_gpu(2, n, n);
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 2);
    int ok = w != NULL && v != NULL && rtns != NULL;
    int info = 0;
    if (ok && np_eigh(NDArray_FDATA(a), (size_t) n, NDArray_FDATA(w), NDArray_FDATA(v), &info) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (ok && info > 0) {   /* unlike the SVD's factors, a half-converged eigendecomposition answers nothing */
        np_ext_throw("eig: the Jacobi iteration reached its sweep cap before every off-diagonal pair fell under the tolerance");
        ok = 0;
    }
    if (!ok) {
        if (w != NULL) NDArray_FREE(w);
        if (v != NULL) NDArray_FREE(v);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = w;
    rtns[1] = v;
    return rtns;
}

NDArray **NPH_Qr(NDArray *a) {
    if (a == NULL) return NULL;
    /* the reference returns NULL without a message in both cases (linalg.c:916-926), which its PHP_METHOD then dereferences */
    if (NDArray_NDIM(a) != 2) {
        np_ext_throw("qr: the operand must be two-dimensional");
        return NULL;
    }
    if (NDArray_SHAPE(a)[0] < NDArray_SHAPE(a)[1]) {
        np_ext_throw("qr: the operand must have at least as many rows as columns (m >= n)");
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    const int m = NDArray_SHAPE(a)[0], n = NDArray_SHAPE(a)[1];
    /* the reference's shapes and order (linalg.c:929-968): rtn[0] = Q (m, n), rtn[1] = R (n, n); Q is the reduced orthonormal
     * factor (np_qr), not the packed reflectors the reference's CPU path hands back */
    NDArray *q = zeros_on_gpu(2, m, n), *r = zeros_on_gpu(2, n, n);
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 2);
    int ok = q != NULL && r != NULL && rtns != NULL;
    if (ok && np_qr(NDArray_FDATA(a), (size_t) m, (size_t) n, NDArray_FDATA(q), NDArray_FDATA(r)) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (!ok) {
        if (q != NULL) NDArray_FREE(q);
        if (r != NULL) NDArray_FREE(r);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = q;
    rtns[1] = r;
    return rtns;
}

NDArray *NPH_Lstsq(NDArray *a, NDArray *b) {
    if (a == NULL || b == NULL) return NULL;
    if (NDArray_NDIM(a) != 2 || NDArray_NDIM(b) != 2 || NDArray_SHAPE(a)[0] != NDArray_SHAPE(b)[0]) {   /* linalg.c:856-859 */
        np_ext_throw("Invalid dimensions to calculate lstsq, both arrays must have 2 dimensions and $b must contain the same "
                     "amount of rows as $a");
        return NULL;
    }
    if (NDArray_DEVICE(a) != NDArray_DEVICE(b)) {
        np_ext_throw("lstsq: both operands must be on the same device");
        return NULL;
    }
    if (!on_gpu(a)) return NULL;
    const int m = NDArray_SHAPE(a)[0], n = NDArray_SHAPE(a)[1], nrhs = NDArray_SHAPE(b)[1];
    if (m < n) {   /* the reference's sgels answers with the minimum-norm solution there */
        np_ext_throw("lstsq: the device solver needs at least as many rows as columns (m >= n); an underdetermined system goes "
                     "through ->cpu() and the reference's own LAPACK path");
        return NULL;
    }
    NDArray *x = zeros_on_gpu(2, n, nrhs);                                       /* linalg.c:865-868 */
    if (x == NULL) return NULL;
    int info = 0;
    if (np_lstsq(NDArray_FDATA(a), NDArray_FDATA(b), (size_t) m, (size_t) n, (size_t) nrhs, NDArray_FDATA(x), &info) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(x);
        return NULL;
    }
    if (info > 0) {                                                              /* linalg.c:882-886 */
        char msg[160];
        snprintf(msg, sizeof msg, "The diagonal element %i of the triangular factor of $a is zero, so that $a does not have full rank.", info);
        np_ext_throw(msg);
        NDArray_FREE(x);
        return NULL;
    }
    return x;
}
