/*
 * hip_signal.c — the device side of NDArray_Correlate2D (hip_signal.h).  Compiled into a --with-hip tree against the
 * reference's headers (-DNUMPOWER_NDARRAY_HEADER='"src/initializers.h"') and into libnumpower_host.so against
 * include/numpower_host.h; it uses only what both declare, with one switch: the reference's arrays take ownership of an
 * emalloc'd shape, the host library copies shapes.
 */
#ifndef NUMPOWER_NDARRAY_HEADER
#define NUMPOWER_NDARRAY_HEADER "numpower_host.h"
#endif
#include NUMPOWER_NDARRAY_HEADER

#include <stddef.h>

#include "hip_signal.h"
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

static const char kValid[] = "For 'valid' mode, one input must be at least as large as the other in every dimension";   /* signal.c:235 */

NDArray *NPH_Correlate2D(NDArray *a, NDArray *b, int mode, int boundary, NDArray *fill_value, int flip) {
    if (a == NULL || b == NULL) return NULL;
    if (NDArray_NDIM(a) != 2 || NDArray_NDIM(b) != 2) {                          /* signal.c:227-230 */
        np_ext_throw("NDArray::correlate2d inputs must be both 2-D arrays");
        return NULL;
    }
    const int ah = NDArray_SHAPE(a)[0], aw = NDArray_SHAPE(a)[1], bh = NDArray_SHAPE(b)[0], bw = NDArray_SHAPE(b)[1];
    if (mode == NP_CONV_VALID && !(ah >= bh && aw >= bw) && !(bh >= ah && bw >= aw)) {   /* scipy's _inputs_swap_needed */
        np_ext_throw(kValid);
        return NULL;
    }
    float fill = 0.0f;
    if (boundary == NP_CONV_FILL && fill_value != NULL) {                        /* signal.c:245-249 */
        if (NDArray_NUMELEMENTS(fill_value) != 1) {
            np_ext_throw("fillValue must be a scalar or an array with one element.");
            return NULL;
        }
        if (NDArray_DEVICE(fill_value) != NDARRAY_DEVICE_GPU) {
            fill = NDArray_FDATA(fill_value)[0];
        } else if (np_memcpy_d2h(&fill, NDArray_FDATA(fill_value), sizeof(float)) != NP_OK) {
            np_ext_throw_last();
            return NULL;
        }
    }
    if (mode != NP_CONV_VALID && mode != NP_CONV_SAME && mode != NP_CONV_FULL) {   /* signal.c:280-282 */
        np_ext_throw("invalid mode.");
        return NULL;
    }
    if (NDArray_DEVICE(a) != NDArray_DEVICE(b)) {                                /* signal.c:219-222 */
        np_ext_throw("correlate2d not implemented for GPU computation.");
        return NULL;
    }
    if (NDArray_DEVICE(a) != NDARRAY_DEVICE_GPU) {
        np_ext_throw("correlate2d: operands are on the CPU; numpower_amd only computes on the GPU "
                     "(call ->gpu() first, the CPU path is the reference's own)");
        return NULL;
    }
    size_t oh = 0, ow = 0;
    if (ah < 1 || aw < 1 || bh < 1 || bw < 1 ||
        np_correlate2d_shape((size_t) ah, (size_t) aw, (size_t) bh, (size_t) bw, mode, &oh, &ow) != NP_OK) {
        if (ah < 1 || aw < 1 || bh < 1 || bw < 1) np_ext_throw("correlate2d: an operand has no elements");
        else np_ext_throw_last();
        return NULL;
    }
    int *shape = (int *) NPH_ALLOC(sizeof(int) * 2);
    if (shape == NULL) return NULL;
    shape[0] = (int) oh;
    shape[1] = (int) ow;
    NDArray *rtn = NDArray_Empty(shape, 2, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    if (rtn == NULL) return NULL;
    if (np_correlate2d(NDArray_FDATA(a), (size_t) ah, (size_t) aw, NDArray_FDATA(b), (size_t) bh, (size_t) bw, mode, boundary,
                       fill, flip, NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}
