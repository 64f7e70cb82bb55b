/*
 * hip_linalg.c — the device side of NDArray_Det / Inverse / LU / Solve / Cholesky (hip_linalg.h).  Compiled into a --with-hip tree
 * against the reference's headers (-DNUMPOWER_NDARRAY_HEADER='"src/initializers.h"') and into libnumpower_host.so
 * against include/numpower_host.h; it uses only what both declare.
 */
#ifndef NUMPOWER_NDARRAY_HEADER
#define NUMPOWER_NDARRAY_HEADER "numpower_host.h"
#endif
#include NUMPOWER_NDARRAY_HEADER

#include <stddef.h>

#include "hip_linalg.h"
#include "np_ext_hooks.h"
#include "np_hip.h"

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
