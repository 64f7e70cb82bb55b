/*
 * hip_dnn.c — the device side of NDArrayDNN_Conv2D_Forward / _Backward (hip_dnn.h).  Compiled into a --with-hip tree against the
 * reference's headers (-DNUMPOWER_NDARRAY_HEADER='"src/initializers.h"') and into libnumpower_host.so against
 * include/numpower_host.h; it uses only what both declare, with one switch: the reference's arrays take ownership of an
 * emalloc'd shape and its result vectors are emalloc'd, the host library copies shapes and hands out malloc'd vectors.
 */
#ifndef NUMPOWER_NDARRAY_HEADER
#define NUMPOWER_NDARRAY_HEADER "numpower_host.h"
#endif
#include NUMPOWER_NDARRAY_HEADER

#include <stddef.h>

#include "hip_dnn.h"
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

/* the layer's extents, read once the shapes have been checked */
typedef struct { size_t N, C, H, W, F, kh, kw; } nph_layer;
/* stride, padding and dilation of an Ex call, as given */
typedef struct { int sh, sw, ph, pw, dh, dw; } nph_geometry;

/* the checks both directions share; y == NULL: forward; g == NULL: stride 1, no padding, dilation 1 and the messages of the
 * reference-signature calls.  0 after a raised error */
static int layer_of(NDArray *x, NDArray *y, NDArray *filters, const nph_geometry *g, nph_layer *l) {
    if (NDArray_NDIM(x) != 4 || NDArray_NDIM(filters) != 4 || (y != NULL && NDArray_NDIM(y) != 4)) {
        np_ext_throw(NPH_DNN_MSG_NDIM);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x), *fs = NDArray_SHAPE(filters);
    if (fs[1] != xs[1]) {
        np_ext_throw(NPH_DNN_MSG_CHANNELS);
        return 0;
    }
    if (g == NULL && (fs[2] > xs[2] || fs[3] > xs[3])) {
        np_ext_throw(NPH_DNN_MSG_WINDOW);
        return 0;
    }
    /* the forward result's extents, in 64 bits: a dilation times a window may not fit an int */
    long long oh = (long long) xs[2] - fs[2] + 1, ow = (long long) xs[3] - fs[3] + 1;
    if (g != NULL) {
        if (g->sh < 1 || g->sw < 1) {
            np_ext_throw(NPH_DNN_MSG_STRIDE);
            return 0;
        }
        if (g->dh < 1 || g->dw < 1) {
            np_ext_throw(NPH_DNN_MSG_DILATION);
            return 0;
        }
        const long long keh = (long long) g->dh * (fs[2] - 1) + 1, kew = (long long) g->dw * (fs[3] - 1) + 1;
        if (fs[2] >= 1 && fs[3] >= 1 && (g->ph < 0 || g->pw < 0 || g->ph >= keh || g->pw >= kew)) {
            np_ext_throw(NPH_DNN_MSG_PADDING);
            return 0;
        }
        if (keh > xs[2] + 2LL * g->ph || kew > xs[3] + 2LL * g->pw) {
            np_ext_throw(NPH_DNN_MSG_EFFECTIVE);
            return 0;
        }
        oh = (xs[2] + 2LL * g->ph - keh) / g->sh + 1, ow = (xs[3] + 2LL * g->pw - kew) / g->sw + 1;
    }
    if (y != NULL) {
        const int *ys = NDArray_SHAPE(y);
        if (ys[0] != xs[0] || ys[1] != fs[0] || ys[2] != oh || ys[3] != ow) {
            np_ext_throw(g == NULL ? NPH_DNN_MSG_GRADIENT : NPH_DNN_MSG_STRIDED_GRADIENT);
            return 0;
        }
    }
    if (NDArray_DEVICE(x) != NDArray_DEVICE(filters) || (y != NULL && NDArray_DEVICE(y) != NDArray_DEVICE(x))) {
        np_ext_throw(NPH_DNN_MSG_DEVICE);
        return 0;
    }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_DNN_MSG_CPU);
        return 0;
    }
    l->N = (size_t) xs[0], l->C = (size_t) xs[1], l->H = (size_t) xs[2], l->W = (size_t) xs[3];
    l->F = (size_t) fs[0], l->kh = (size_t) fs[2], l->kw = (size_t) fs[3];
    return 1;
}

/* a new 4-d GPU array, allocated as the reference allocates its results (NDArray_Empty over an emalloc'd shape, dnn.c:284) */
static NDArray *empty4_on_gpu(size_t d0, size_t d1, size_t d2, size_t d3) {
    int *shape = (int *) NPH_ALLOC(sizeof(int) * 4);
    if (shape == NULL) return NULL;
    shape[0] = (int) d0, shape[1] = (int) d1, shape[2] = (int) d2, shape[3] = (int) d3;
    NDArray *rtn = NDArray_Empty(shape, 4, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

NDArray *NPH_Conv2D_Forward(NDArray *x, NDArray *filters) {
    nph_layer l;
    if (x == NULL || filters == NULL || !layer_of(x, NULL, filters, NULL, &l)) return NULL;
    size_t oh = 0, ow = 0;
    if (np_conv2d_shape(l.H, l.W, l.kh, l.kw, 0, 0, &oh, &ow) != NP_OK || l.N < 1 || l.C < 1 || l.F < 1) {
        if (l.N < 1 || l.C < 1 || l.F < 1) np_ext_throw("dnn_conv2d: an operand has no elements");
        else np_ext_throw_last();
        return NULL;
    }
    NDArray *rtn = empty4_on_gpu(l.N, l.F, oh, ow);
    if (rtn == NULL) return NULL;
    if (np_conv2d_forward(NDArray_FDATA(x), NDArray_FDATA(filters), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, 0, 0, NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray **NPH_Conv2D_Backward(NDArray *x, NDArray *y, NDArray *filters) {
    nph_layer l;
    if (x == NULL || y == NULL || filters == NULL || !layer_of(x, y, filters, NULL, &l)) return NULL;
    if (NDArray_NUMELEMENTS(x) < 1 || NDArray_NUMELEMENTS(filters) < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    /* the reference's order (dnn.c:365-366): rtn[0] = dW in the filters' shape, rtn[1] = dX in the input's */
    NDArray *dw = empty4_on_gpu(l.F, l.C, l.kh, l.kw), *dx = empty4_on_gpu(l.N, l.C, l.H, l.W);
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 2);
    int ok = dw != NULL && dx != NULL && rtns != NULL;
    if (ok && (np_conv2d_backward_filter(NDArray_FDATA(x), NDArray_FDATA(y), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, 0, 0, NDArray_FDATA(dw)) != NP_OK ||
               np_conv2d_backward_data(NDArray_FDATA(y), NDArray_FDATA(filters), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, 0, 0, NDArray_FDATA(dx)) != NP_OK)) {
        np_ext_throw_last();
        ok = 0;
    }
    if (!ok) {
        if (dw != NULL) NDArray_FREE(dw);
        if (dx != NULL) NDArray_FREE(dx);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = dw;
    rtns[1] = dx;
    return rtns;
}

/* NULL: the default */
static nph_geometry geometry_of(const int stride[2], const int padding[2], const int dilation[2]) {
    nph_geometry g = {1, 1, 0, 0, 1, 1};
    if (stride != NULL) g.sh = stride[0], g.sw = stride[1];
    if (padding != NULL) g.ph = padding[0], g.pw = padding[1];
    if (dilation != NULL) g.dh = dilation[0], g.dw = dilation[1];
    return g;
}

NDArray *NPH_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int stride[2], const int padding[2], const int dilation[2]) {
    nph_layer l;
    const nph_geometry g = geometry_of(stride, padding, dilation);
    if (x == NULL || filters == NULL || !layer_of(x, NULL, filters, &g, &l)) return NULL;
    size_t oh = 0, ow = 0;
    if (l.N < 1 || l.C < 1 || l.F < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    if (np_conv2d_shape_ex(l.H, l.W, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw, (size_t) g.sh, (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, &oh, &ow) != NP_OK) {
        np_ext_throw_last();
        return NULL;
    }
    NDArray *rtn = empty4_on_gpu(l.N, l.F, oh, ow);
    if (rtn == NULL) return NULL;
    if (np_conv2d_forward_ex(NDArray_FDATA(x), NDArray_FDATA(filters), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw, (size_t) g.sh,
                             (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray **NPH_Conv2D_BackwardEx(NDArray *x, NDArray *y, NDArray *filters, const int stride[2], const int padding[2], const int dilation[2]) {
    nph_layer l;
    const nph_geometry g = geometry_of(stride, padding, dilation);
    if (x == NULL || y == NULL || filters == NULL || !layer_of(x, y, filters, &g, &l)) return NULL;
    if (NDArray_NUMELEMENTS(x) < 1 || NDArray_NUMELEMENTS(filters) < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    NDArray *dw = empty4_on_gpu(l.F, l.C, l.kh, l.kw), *dx = empty4_on_gpu(l.N, l.C, l.H, l.W);
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 2);
    int ok = dw != NULL && dx != NULL && rtns != NULL;
    if (ok && (np_conv2d_backward_filter_ex(NDArray_FDATA(x), NDArray_FDATA(y), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw,
                                            (size_t) g.sh, (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, NDArray_FDATA(dw)) != NP_OK ||
               np_conv2d_backward_data_ex(NDArray_FDATA(y), NDArray_FDATA(filters), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw,
                                          (size_t) g.sh, (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, NDArray_FDATA(dx)) != NP_OK)) {
        np_ext_throw_last();
        ok = 0;
    }
    if (!ok) {
        if (dw != NULL) NDArray_FREE(dw);
        if (dx != NULL) NDArray_FREE(dx);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = dw;
    rtns[1] = dx;
    return rtns;
}

/* ---- the layer: a bias and an activation (hip_dnn.h) ---- */

/* 'r', 't', 's', 'n' or 0 -> np_conv_act, -1 for anything else */
static int activation_of(char activation) {
    switch (activation) {
    case 'r': return NP_ACT_RELU;
    case 't': return NP_ACT_TANH;
    case 's': return NP_ACT_SIGMOID;
    case 'n': case 0: return NP_ACT_NONE;
    default: return -1;
    }
}

/* the layer's own checks, which come before layer_of()'s; bias may be NULL, and so may out and dy (forward).  0 after a raised error */
static int layer_extras(NDArray *x, NDArray *filters, NDArray *bias, NDArray *out, NDArray *dy, int act) {
    if (act < 0) {
        np_ext_throw(NPH_DNN_MSG_ACTIVATION);
        return 0;
    }
    if (bias != NULL && NDArray_NDIM(filters) == 4 && (NDArray_NDIM(bias) != 1 || NDArray_SHAPE(bias)[0] != NDArray_SHAPE(filters)[0])) {
        np_ext_throw(NPH_DNN_MSG_BIAS);
        return 0;
    }
    if (dy != NULL && (out != NULL || act != NP_ACT_NONE)) {
        int same = out != NULL && NDArray_NDIM(out) == NDArray_NDIM(dy);
        for (int d = 0; same && d < NDArray_NDIM(dy); ++d) same = NDArray_SHAPE(out)[d] == NDArray_SHAPE(dy)[d];
        if (!same) {
            np_ext_throw(NPH_DNN_MSG_OUT);
            return 0;
        }
    }
    if (bias != NULL && (NDArray_DEVICE(bias) != NDArray_DEVICE(x) || NDArray_DEVICE(bias) != NDArray_DEVICE(filters))) {
        np_ext_throw(NPH_DNN_MSG_BIAS_DEVICE);
        return 0;
    }
    if (dy != NULL && out != NULL && NDArray_DEVICE(out) != NDArray_DEVICE(dy)) {
        np_ext_throw(NPH_DNN_MSG_DEVICE);
        return 0;
    }
    return 1;
}

/* a new 1-d GPU array of n floats */
static NDArray *empty1_on_gpu(size_t n) {
    int *shape = (int *) NPH_ALLOC(sizeof(int));
    if (shape == NULL) return NULL;
    shape[0] = (int) n;
    NDArray *rtn = NDArray_Empty(shape, 1, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

NDArray *NPH_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int stride[2], const int padding[2], const int dilation[2],
                                 char activation) {
    nph_layer l;
    const nph_geometry g = geometry_of(stride, padding, dilation);
    const int act = activation_of(activation);
    if (x == NULL || filters == NULL || !layer_extras(x, filters, bias, NULL, NULL, act) || !layer_of(x, NULL, filters, &g, &l)) return NULL;
    size_t oh = 0, ow = 0;
    if (l.N < 1 || l.C < 1 || l.F < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    if (np_conv2d_shape_ex(l.H, l.W, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw, (size_t) g.sh, (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, &oh, &ow) != NP_OK) {
        np_ext_throw_last();
        return NULL;
    }
    NDArray *rtn = empty4_on_gpu(l.N, l.F, oh, ow);
    if (rtn == NULL) return NULL;
    if (np_conv2d_forward_act(NDArray_FDATA(x), NDArray_FDATA(filters), bias != NULL ? NDArray_FDATA(bias) : NULL, l.N, l.C, l.H, l.W, l.F, l.kh, l.kw,
                              (size_t) g.ph, (size_t) g.pw, (size_t) g.sh, (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, act, NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray **NPH_Conv2D_LayerBackward(NDArray *x, NDArray *out, NDArray *dy, NDArray *filters, const int stride[2], const int padding[2],
                                   const int dilation[2], char activation, int use_bias) {
    nph_layer l;
    const nph_geometry g = geometry_of(stride, padding, dilation);
    const int act = activation_of(activation);
    if (x == NULL || dy == NULL || filters == NULL) return NULL;
    if (!layer_extras(x, filters, NULL, out, dy, act) || !layer_of(x, dy, filters, &g, &l)) return NULL;
    if (NDArray_NUMELEMENTS(x) < 1 || NDArray_NUMELEMENTS(filters) < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    const size_t P = (size_t) NDArray_SHAPE(dy)[2] * (size_t) NDArray_SHAPE(dy)[3];
    NDArray *dw = empty4_on_gpu(l.F, l.C, l.kh, l.kw), *dx = empty4_on_gpu(l.N, l.C, l.H, l.W), *db = use_bias ? empty1_on_gpu(l.F) : NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    void *dz = NULL;   /* pool scratch, only with an activation: dz = dy otherwise */
    int ok = dw != NULL && dx != NULL && rtns != NULL && (db != NULL || !use_bias);
    if (ok && act != NP_ACT_NONE && np_malloc(&dz, l.N * l.F * P * sizeof(float)) != NP_OK) {
        np_ext_throw_last();
        dz = NULL;
        ok = 0;
    }
    const float *grad = dz != NULL ? (const float *) dz : NDArray_FDATA(dy);
    if (ok && (act != NP_ACT_NONE || use_bias) &&
        np_conv2d_backward_act(out != NULL ? NDArray_FDATA(out) : NULL, NDArray_FDATA(dy), l.N, l.F, P, act, (float *) dz,
                               db != NULL ? NDArray_FDATA(db) : NULL) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (ok && (np_conv2d_backward_filter_ex(NDArray_FDATA(x), grad, l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw, (size_t) g.sh,
                                            (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, NDArray_FDATA(dw)) != NP_OK ||
               np_conv2d_backward_data_ex(grad, NDArray_FDATA(filters), l.N, l.C, l.H, l.W, l.F, l.kh, l.kw, (size_t) g.ph, (size_t) g.pw, (size_t) g.sh,
                                          (size_t) g.sw, (size_t) g.dh, (size_t) g.dw, NDArray_FDATA(dx)) != NP_OK)) {
        np_ext_throw_last();
        ok = 0;
    }
    if (dz != NULL) np_free(dz);   /* released on every path; the pool is stream-ordered: safe right behind the launches that read it */
    if (!ok) {
        if (dw != NULL) NDArray_FREE(dw);
        if (dx != NULL) NDArray_FREE(dx);
        if (db != NULL) NDArray_FREE(db);
        if (rtns != NULL) NPH_RELEASE(rtns);
        return NULL;
    }
    rtns[0] = dw;
    rtns[1] = dx;
    rtns[2] = db;
    return rtns;
}
