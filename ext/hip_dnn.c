/*
 * hip_dnn.c — the device side of NDArrayDNN_Conv2D_Forward / _Backward, of the pooling layers, of softmax / cross-entropy and of batch normalization (hip_dnn.h).  Compiled into a --with-hip tree against the
 * reference's headers (-DNUMPOWER_NDARRAY_HEADER='"src/initializers.h"') and into libnumpower_host.so against
 * include/numpower_host.h; it uses only what both declare, with one switch: the reference's arrays take ownership of an
 * emalloc'd shape and its result vectors are emalloc'd, the host library copies shapes and hands out malloc'd vectors.
 */
#ifndef NUMPOWER_NDARRAY_HEADER
#define NUMPOWER_NDARRAY_HEADER "numpower_host.h"
#endif
#include NUMPOWER_NDARRAY_HEADER

#include <math.h>
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

/* NULL: the default */
static nph_geometry geometry_of(const int stride[2], const int padding[2], const int dilation[2]) {
    nph_geometry g = {1, 1, 0, 0, 1, 1};
    if (stride != NULL) g.sh = stride[0], g.sw = stride[1];
    if (padding != NULL) g.ph = padding[0], g.pw = padding[1];
    if (dilation != NULL) g.dh = dilation[0], g.dw = dilation[1];
    return g;
}

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

/* the layer's own checks, which come before layer_of()'s; bias may be NULL, and so may out and dy (forward).  A call without a
 * bias, an out and an activation passes them all.  0 after a raised error */
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

/* a new GPU array, allocated as the reference allocates its results (NDArray_Empty over an emalloc'd shape, dnn.c:284) */
static NDArray *empty_on_gpu(int ndim, const size_t *dims) {
    int *shape = (int *) NPH_ALLOC(sizeof(int) * (size_t) ndim);
    if (shape == NULL) return NULL;
    for (int d = 0; d < ndim; ++d) shape[d] = (int) dims[d];
    NDArray *rtn = NDArray_Empty(shape, ndim, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

/* a layer as the np_conv2d_*_ex calls take it */
#define NPH_LAYER_ARGS(l, g) \
    (l).N, (l).C, (l).H, (l).W, (l).F, (l).kh, (l).kw, (size_t) (g)->ph, (size_t) (g)->pw, (size_t) (g)->sh, (size_t) (g)->sw, (size_t) (g)->dh, (size_t) (g)->dw

static const nph_geometry nph_unit_geometry = {1, 1, 0, 0, 1, 1};

/* The forward pass of all three public functions.  g == NULL: the reference-signature call (layer_of).  Without a bias and an
 * activation np_conv2d_forward_act launches the plain kernels. */
static NDArray *forward(NDArray *x, NDArray *filters, NDArray *bias, const nph_geometry *g, int act) {
    nph_layer l;
    if (x == NULL || filters == NULL || !layer_extras(x, filters, bias, NULL, NULL, act) || !layer_of(x, NULL, filters, g, &l)) return NULL;
    if (l.N < 1 || l.C < 1 || l.F < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    if (g == NULL) g = &nph_unit_geometry;
    size_t oh = 0, ow = 0;
    if (np_conv2d_shape_ex(l.H, l.W, l.kh, l.kw, (size_t) g->ph, (size_t) g->pw, (size_t) g->sh, (size_t) g->sw, (size_t) g->dh, (size_t) g->dw, &oh, &ow) != NP_OK) {
        np_ext_throw_last();
        return NULL;
    }
    const size_t dims[4] = {l.N, l.F, oh, ow};
    NDArray *rtn = empty_on_gpu(4, dims);
    if (rtn == NULL) return NULL;
    if (np_conv2d_forward_act(NDArray_FDATA(x), NDArray_FDATA(filters), bias != NULL ? NDArray_FDATA(bias) : NULL, NPH_LAYER_ARGS(l, g), act,
                              NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

/* The backward pass of all three public functions: a vector of n_rtn, rtn[0] = dW in the filters' shape and rtn[1] = dX in the
 * input's, the reference's order (dnn.c:365-366), rtn[2] = db or NULL.  dy goes through np_conv2d_backward_act first where there
 * is an activation or a bias; dW and dX are the _ex gradients of the result. */
static NDArray **backward(NDArray *x, NDArray *out, NDArray *dy, NDArray *filters, const nph_geometry *g, int act, int use_bias, int n_rtn) {
    nph_layer l;
    if (x == NULL || dy == NULL || filters == NULL) return NULL;
    if (!layer_extras(x, filters, NULL, out, dy, act) || !layer_of(x, dy, filters, g, &l)) return NULL;
    if (NDArray_NUMELEMENTS(x) < 1 || NDArray_NUMELEMENTS(filters) < 1) {
        np_ext_throw("dnn_conv2d: an operand has no elements");
        return NULL;
    }
    if (g == NULL) g = &nph_unit_geometry;
    const size_t P = (size_t) NDArray_SHAPE(dy)[2] * (size_t) NDArray_SHAPE(dy)[3];
    const size_t dw_dims[4] = {l.F, l.C, l.kh, l.kw}, dx_dims[4] = {l.N, l.C, l.H, l.W};
    NDArray *dw = empty_on_gpu(4, dw_dims), *dx = empty_on_gpu(4, dx_dims), *db = use_bias ? empty_on_gpu(1, &l.F) : NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * (size_t) n_rtn);
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
    if (ok && (np_conv2d_backward_filter_ex(NDArray_FDATA(x), grad, NPH_LAYER_ARGS(l, g), NDArray_FDATA(dw)) != NP_OK ||
               np_conv2d_backward_data_ex(grad, NDArray_FDATA(filters), NPH_LAYER_ARGS(l, g), NDArray_FDATA(dx)) != NP_OK)) {
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
    if (n_rtn > 2) rtns[2] = db;
    return rtns;
}

/* ---- the public functions (hip_dnn.h): each fills in its defaults ---- */

NDArray *NPH_Conv2D_Forward(NDArray *x, NDArray *filters) { return forward(x, filters, NULL, NULL, NP_ACT_NONE); }

NDArray **NPH_Conv2D_Backward(NDArray *x, NDArray *y, NDArray *filters) { return backward(x, NULL, y, filters, NULL, NP_ACT_NONE, 0, 2); }

NDArray *NPH_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int stride[2], const int padding[2], const int dilation[2]) {
    const nph_geometry g = geometry_of(stride, padding, dilation);
    return forward(x, filters, NULL, &g, NP_ACT_NONE);
}

NDArray **NPH_Conv2D_BackwardEx(NDArray *x, NDArray *y, NDArray *filters, const int stride[2], const int padding[2], const int dilation[2]) {
    const nph_geometry g = geometry_of(stride, padding, dilation);
    return backward(x, NULL, y, filters, &g, NP_ACT_NONE, 0, 2);
}

NDArray *NPH_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int stride[2], const int padding[2], const int dilation[2],
                                 char activation) {
    const nph_geometry g = geometry_of(stride, padding, dilation);
    return forward(x, filters, bias, &g, activation_of(activation));
}

NDArray **NPH_Conv2D_LayerBackward(NDArray *x, NDArray *out, NDArray *dy, NDArray *filters, const int stride[2], const int padding[2],
                                   const int dilation[2], char activation, int use_bias) {
    const nph_geometry g = geometry_of(stride, padding, dilation);
    return backward(x, out, dy, filters, &g, activation_of(activation), use_bias, 3);
}

/* ---- pooling (hip_dnn.h): N.C planes through np_pool2d_forward / np_pool2d_backward ---- */

typedef struct { size_t planes, H, W, kh, kw, ph, pw, sh, sw, oh, ow; int mode; } nph_pool;

/* 'm', 'a', 'v' -> np_pool_mode, -1 for anything else */
static int pool_mode_of(char mode) {
    switch (mode) {
    case 'm': return NP_POOL_MAX;
    case 'a': return NP_POOL_AVG;
    case 'v': return NP_POOL_AVG_VALID;
    default: return -1;
    }
}

/* the checks both directions share, in the order of hip_dnn.h; dy == NULL: forward.  0 after a raised error */
static int pool_of(NDArray *x, NDArray *dy, const int kernel[2], const int stride[2], const int padding[2], char mode, nph_pool *p) {
    p->mode = pool_mode_of(mode);
    if (p->mode < 0) {
        np_ext_throw(NPH_POOL_MSG_MODE);
        return 0;
    }
    if (NDArray_NDIM(x) != 4 || (dy != NULL && NDArray_NDIM(dy) != 4)) {
        np_ext_throw(NPH_POOL_MSG_NDIM);
        return 0;
    }
    if (kernel == NULL || kernel[0] < 1 || kernel[1] < 1) {
        np_ext_throw(NPH_POOL_MSG_WINDOW);
        return 0;
    }
    const int sh = stride != NULL ? stride[0] : kernel[0], sw = stride != NULL ? stride[1] : kernel[1];
    const int ph = padding != NULL ? padding[0] : 0, pw = padding != NULL ? padding[1] : 0;
    if (sh < 1 || sw < 1) {
        np_ext_throw(NPH_POOL_MSG_STRIDE);
        return 0;
    }
    if (ph < 0 || pw < 0 || ph > kernel[0] / 2 || pw > kernel[1] / 2) {
        np_ext_throw(NPH_POOL_MSG_PADDING);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x);
    if (kernel[0] > xs[2] + 2LL * ph || kernel[1] > xs[3] + 2LL * pw) {
        np_ext_throw(NPH_POOL_MSG_LARGER);
        return 0;
    }
    const long long oh = (xs[2] + 2LL * ph - kernel[0]) / sh + 1, ow = (xs[3] + 2LL * pw - kernel[1]) / sw + 1;
    if (dy != NULL) {
        const int *ys = NDArray_SHAPE(dy);
        if (ys[0] != xs[0] || ys[1] != xs[1] || ys[2] != oh || ys[3] != ow) {
            np_ext_throw(NPH_POOL_MSG_GRADIENT);
            return 0;
        }
        if (NDArray_DEVICE(dy) != NDArray_DEVICE(x)) {
            np_ext_throw(NPH_POOL_MSG_DEVICE);
            return 0;
        }
    }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_POOL_MSG_CPU);
        return 0;
    }
    if (xs[0] < 1 || xs[1] < 1 || xs[2] < 1 || xs[3] < 1) {
        np_ext_throw("dnn_pool2d: an operand has no elements");
        return 0;
    }
    p->planes = (size_t) xs[0] * (size_t) xs[1], p->H = (size_t) xs[2], p->W = (size_t) xs[3];
    p->kh = (size_t) kernel[0], p->kw = (size_t) kernel[1], p->ph = (size_t) ph, p->pw = (size_t) pw, p->sh = (size_t) sh, p->sw = (size_t) sw;
    p->oh = (size_t) oh, p->ow = (size_t) ow;
    return 1;
}

/* a pooling as the np_pool2d_* calls take it */
#define NPH_POOL_ARGS(p) (p).planes, (p).H, (p).W, (p).kh, (p).kw, (p).ph, (p).pw, (p).sh, (p).sw

NDArray *NPH_Pool2D_Forward(NDArray *x, const int kernel[2], const int stride[2], const int padding[2], char mode) {
    nph_pool p;
    if (x == NULL || !pool_of(x, NULL, kernel, stride, padding, mode, &p)) return NULL;
    const int *xs = NDArray_SHAPE(x);
    const size_t dims[4] = {(size_t) xs[0], (size_t) xs[1], p.oh, p.ow};
    NDArray *rtn = empty_on_gpu(4, dims);
    if (rtn == NULL) return NULL;
    if (np_pool2d_forward(NDArray_FDATA(x), NPH_POOL_ARGS(p), p.mode, NDArray_FDATA(rtn), NULL) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray *NPH_Pool2D_Backward(NDArray *x, NDArray *dy, const int kernel[2], const int stride[2], const int padding[2], char mode) {
    nph_pool p;
    if (x == NULL || dy == NULL || !pool_of(x, dy, kernel, stride, padding, mode, &p)) return NULL;
    const int *xs = NDArray_SHAPE(x);
    const size_t dims[4] = {(size_t) xs[0], (size_t) xs[1], p.H, p.W};
    NDArray *dx = empty_on_gpu(4, dims);
    if (dx == NULL) return NULL;
    const size_t numel_y = p.planes * p.oh * p.ow;
    void *again = NULL;   /* pool scratch, max only: the forward pass again, y in the first half and idx in the second */
    int ok = 1;
    if (p.mode == NP_POOL_MAX && np_malloc(&again, numel_y * (sizeof(float) + sizeof(int32_t))) != NP_OK) {
        np_ext_throw_last();
        again = NULL;
        ok = 0;
    }
    int32_t *idx = again != NULL ? (int32_t *) ((float *) again + numel_y) : NULL;
    if (ok && p.mode == NP_POOL_MAX && np_pool2d_forward(NDArray_FDATA(x), NPH_POOL_ARGS(p), p.mode, (float *) again, idx) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (ok && np_pool2d_backward(NDArray_FDATA(dy), idx, NPH_POOL_ARGS(p), p.mode, NDArray_FDATA(dx)) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (again != NULL) np_free(again);   /* released on every path; the pool is stream-ordered: safe right behind the launches that read it */
    if (!ok) {
        NDArray_FREE(dx);
        return NULL;
    }
    return dx;
}

/* ---- softmax, log-softmax and cross-entropy (hip_dnn.h): np_softmax_forward / _backward and np_cross_entropy ---- */

typedef struct { size_t outer, cols, inner; int mode; } nph_softmax;

/* 's', 'l' -> np_softmax_mode, -1 for anything else */
static int softmax_mode_of(char mode) {
    switch (mode) {
    case 's': return NP_SOFTMAX;
    case 'l': return NP_LOG_SOFTMAX;
    default: return -1;
    }
}

/* the checks both directions share, in the order of hip_dnn.h; dy == NULL: forward.  0 after a raised error */
static int softmax_of(NDArray *x, NDArray *dy, int axis, char mode, nph_softmax *s) {
    s->mode = softmax_mode_of(mode);
    if (s->mode < 0) {
        np_ext_throw(NPH_SOFTMAX_MSG_MODE);
        return 0;
    }
    const int ndim = NDArray_NDIM(x);
    if (ndim < 1 || axis < -ndim || axis >= ndim) {
        np_ext_throw(NPH_SOFTMAX_MSG_AXIS);
        return 0;
    }
    if (axis < 0) axis += ndim;
    const int *xs = NDArray_SHAPE(x);
    if (dy != NULL) {
        int same = NDArray_NDIM(dy) == ndim;
        for (int d = 0; same && d < ndim; ++d) same = NDArray_SHAPE(dy)[d] == xs[d];
        if (!same) {
            np_ext_throw(NPH_SOFTMAX_MSG_GRADIENT);
            return 0;
        }
        if (NDArray_DEVICE(dy) != NDArray_DEVICE(x)) {
            np_ext_throw(NPH_SOFTMAX_MSG_DEVICE);
            return 0;
        }
    }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_SOFTMAX_MSG_CPU);
        return 0;
    }
    s->outer = 1, s->inner = 1, s->cols = (size_t) xs[axis];
    for (int d = 0; d < axis; ++d) s->outer *= (size_t) xs[d];
    for (int d = axis + 1; d < ndim; ++d) s->inner *= (size_t) xs[d];
    if (s->outer < 1 || s->cols < 1 || s->inner < 1) {
        np_ext_throw("softmax: an operand has no elements");
        return 0;
    }
    return 1;
}

/* a new GPU array of a's shape */
static NDArray *empty_like_on_gpu(NDArray *a) {
    const int ndim = NDArray_NDIM(a);
    int *shape = (int *) NPH_ALLOC(sizeof(int) * (size_t) ndim);
    if (shape == NULL) return NULL;
    for (int d = 0; d < ndim; ++d) shape[d] = NDArray_SHAPE(a)[d];
    NDArray *rtn = NDArray_Empty(shape, ndim, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

NDArray *NPH_Softmax_Forward(NDArray *x, int axis, char mode) {
    nph_softmax s;
    if (x == NULL || !softmax_of(x, NULL, axis, mode, &s)) return NULL;
    NDArray *rtn = empty_like_on_gpu(x);
    if (rtn == NULL) return NULL;
    if (np_softmax_forward(NDArray_FDATA(x), s.outer, s.cols, s.inner, s.mode, NDArray_FDATA(rtn)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(rtn);
        return NULL;
    }
    return rtn;
}

NDArray *NPH_Softmax_Backward(NDArray *y, NDArray *dy, int axis, char mode) {
    nph_softmax s;
    if (y == NULL || dy == NULL || !softmax_of(y, dy, axis, mode, &s)) return NULL;
    NDArray *dx = empty_like_on_gpu(y);
    if (dx == NULL) return NULL;
    if (np_softmax_backward(NDArray_FDATA(y), NDArray_FDATA(dy), s.outer, s.cols, s.inner, s.mode, NDArray_FDATA(dx)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(dx);
        return NULL;
    }
    return dx;
}

/* the checks of the cross-entropy, in the order of hip_dnn.h: *kind is the np_xent_target.  0 after a raised error */
static int xent_of(NDArray *logits, NDArray *target, char reduction, int *kind) {
    if (NDArray_NDIM(logits) != 2) {
        np_ext_throw(NPH_XENT_MSG_LOGITS);
        return 0;
    }
    const int *ls = NDArray_SHAPE(logits), *ts = NDArray_SHAPE(target);
    if (NDArray_NDIM(target) == 1 && ts[0] == ls[0]) *kind = NP_XENT_INDEX;
    else if (NDArray_NDIM(target) == 2 && ts[0] == ls[0] && ts[1] == ls[1]) *kind = NP_XENT_PROB;
    else {
        np_ext_throw(NPH_XENT_MSG_TARGET);
        return 0;
    }
    if (reduction != 'n' && reduction != 's' && reduction != 'm') {
        np_ext_throw(NPH_XENT_MSG_REDUCTION);
        return 0;
    }
    if (NDArray_DEVICE(target) != NDArray_DEVICE(logits)) {
        np_ext_throw(NPH_XENT_MSG_DEVICE);
        return 0;
    }
    if (NDArray_DEVICE(logits) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_XENT_MSG_CPU);
        return 0;
    }
    if (ls[0] < 1 || ls[1] < 1) {
        np_ext_throw("dnn_cross_entropy: an operand has no elements");
        return 0;
    }
    return 1;
}

NDArray *NPH_CrossEntropy(NDArray *logits, NDArray *target, char reduction, int with_grad, NDArray **dlogits) {
    int kind = 0;
    if (dlogits != NULL) *dlogits = NULL;
    if (logits == NULL || target == NULL || !xent_of(logits, target, reduction, &kind)) return NULL;
    const size_t rows = (size_t) NDArray_SHAPE(logits)[0], cols = (size_t) NDArray_SHAPE(logits)[1];
    NDArray *loss_rows = empty_on_gpu(1, &rows);
    if (loss_rows == NULL) return NULL;
    NDArray *grad = (with_grad && dlogits != NULL) ? empty_like_on_gpu(logits) : NULL;
    if (with_grad && dlogits != NULL && grad == NULL) {
        NDArray_FREE(loss_rows);
        return NULL;
    }
    const float scale = reduction == 'm' ? 1.0f / (float) rows : 1.0f;
    if (np_cross_entropy(NDArray_FDATA(logits), NDArray_FDATA(target), rows, cols, kind, scale, NDArray_FDATA(loss_rows),
                         grad != NULL ? NDArray_FDATA(grad) : NULL) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(loss_rows);
        if (grad != NULL) NDArray_FREE(grad);
        return NULL;
    }
    NDArray *rtn = loss_rows;
    if (reduction != 'n') {      /* the library's sum of the rows' losses; the mean divides it once */
        float total = 0.0f;
        const int summed = np_reduce_all(NP_SUM, NDArray_FDATA(loss_rows), rows, &total) == NP_OK;
        if (!summed) np_ext_throw_last();
        if (reduction == 'm') total = total / (float) rows;
        NDArray_FREE(loss_rows);
        rtn = summed ? NDArray_CreateFromFloatScalar(total) : NULL;
        if (rtn == NULL) {
            if (grad != NULL) NDArray_FREE(grad);
            return NULL;
        }
    }
    if (grad != NULL) *dlogits = grad;
    return rtn;
}


/* ---- batch normalization (hip_dnn.h): np_batchnorm_forward / np_batchnorm_backward ---- */

typedef struct { size_t N, C, inner; } nph_batchnorm;

/* 1 when a is a (C) array */
static int is_channel_vector(NDArray *a, int C) { return NDArray_NDIM(a) == 1 && NDArray_SHAPE(a)[0] == C; }

/* the checks both directions share, in the order of hip_dnn.h.  Forward: dy == NULL, s1 / s2 the running statistics; backward:
 * s1 / s2 the saved statistics.  Absent operands are NULL.  0 after a raised error */
static int batchnorm_of(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *beta, NDArray *s1, NDArray *s2, int backward, int training,
                        double momentum, double eps, nph_batchnorm *b) {
    const int ndim = NDArray_NDIM(x);
    if (ndim < 2) {
        np_ext_throw(NPH_BN_MSG_NDIM);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x);
    const int C = xs[1];
    b->N = (size_t) xs[0], b->C = (size_t) C, b->inner = 1;
    for (int d = 2; d < ndim; ++d) b->inner *= (size_t) xs[d];
    if (xs[0] < 1 || C < 1 || b->inner < 1) {
        np_ext_throw(NPH_BN_MSG_EMPTY);
        return 0;
    }
    if (gamma != NULL && !is_channel_vector(gamma, C)) {
        np_ext_throw(NPH_BN_MSG_GAMMA);
        return 0;
    }
    if (beta != NULL && !is_channel_vector(beta, C)) {
        np_ext_throw(NPH_BN_MSG_BETA);
        return 0;
    }
    if ((s1 != NULL && !is_channel_vector(s1, C)) || (s2 != NULL && !is_channel_vector(s2, C))) {
        np_ext_throw(backward ? NPH_BN_MSG_SAVED : NPH_BN_MSG_RUNNING);
        return 0;
    }
    if (!backward && !training && (s1 == NULL || s2 == NULL)) {
        np_ext_throw(NPH_BN_MSG_INFERENCE);
        return 0;
    }
    if (dy != NULL) {
        int same = NDArray_NDIM(dy) == ndim;
        for (int d = 0; same && d < ndim; ++d) same = NDArray_SHAPE(dy)[d] == xs[d];
        if (!same) {
            np_ext_throw(NPH_BN_MSG_GRADIENT);
            return 0;
        }
    }
    if (!(eps >= 0.0)) {
        np_ext_throw(NPH_BN_MSG_EPS);
        return 0;
    }
    if (!(momentum >= 0.0 && momentum <= 1.0)) {
        np_ext_throw(NPH_BN_MSG_MOMENTUM);
        return 0;
    }
    NDArray *others[5] = {dy, gamma, beta, s1, s2};
    for (int k = 0; k < 5; ++k)
        if (others[k] != NULL && NDArray_DEVICE(others[k]) != NDArray_DEVICE(x)) {
            np_ext_throw(NPH_BN_MSG_DEVICE);
            return 0;
        }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_BN_MSG_CPU);
        return 0;
    }
    if (!backward && training && b->N * b->inner == 1) {
        np_ext_throw(NPH_BN_MSG_ONE_VALUE);
        return 0;
    }
    return 1;
}

/* frees what a failed call had built; NULL */
static NDArray **batchnorm_drop(NDArray **rtns, NDArray *a, NDArray *b, NDArray *c) {
    if (a != NULL) NDArray_FREE(a);
    if (b != NULL) NDArray_FREE(b);
    if (c != NULL) NDArray_FREE(c);
    if (rtns != NULL) NPH_RELEASE(rtns);
    return NULL;
}

NDArray **NPH_BatchNorm_Forward(NDArray *x, NDArray *gamma, NDArray *beta, NDArray *running_mean, NDArray *running_var, int training,
                                double momentum, double eps) {
    nph_batchnorm b;
    if (x == NULL || !batchnorm_of(x, NULL, gamma, beta, running_mean, running_var, 0, training, momentum, eps, &b)) return NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *y = empty_like_on_gpu(x);
    NDArray *mean = training ? empty_on_gpu(1, &b.C) : NULL, *invstd = training ? empty_on_gpu(1, &b.C) : NULL;
    if (rtns == NULL || y == NULL || (training && (mean == NULL || invstd == NULL))) return batchnorm_drop(rtns, y, mean, invstd);
    if (np_batchnorm_forward(NDArray_FDATA(x), gamma != NULL ? NDArray_FDATA(gamma) : NULL, beta != NULL ? NDArray_FDATA(beta) : NULL, b.N, b.C,
                             b.inner, training, momentum, eps, running_mean != NULL ? NDArray_FDATA(running_mean) : NULL,
                             running_var != NULL ? NDArray_FDATA(running_var) : NULL, NDArray_FDATA(y), training ? NDArray_FDATA(mean) : NULL,
                             training ? NDArray_FDATA(invstd) : NULL) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, y, mean, invstd);
    }
    rtns[0] = y, rtns[1] = mean, rtns[2] = invstd;
    return rtns;
}

NDArray **NPH_BatchNorm_Backward(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd) {
    nph_batchnorm b;
    if (x == NULL || dy == NULL || save_mean == NULL || save_invstd == NULL) return NULL;
    if (!batchnorm_of(x, dy, gamma, NULL, save_mean, save_invstd, 1, 1, 0.0, 0.0, &b)) return NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *dx = empty_like_on_gpu(x), *dgamma = empty_on_gpu(1, &b.C), *dbeta = empty_on_gpu(1, &b.C);
    if (rtns == NULL || dx == NULL || dgamma == NULL || dbeta == NULL) return batchnorm_drop(rtns, dx, dgamma, dbeta);
    if (np_batchnorm_backward(NDArray_FDATA(x), NDArray_FDATA(dy), gamma != NULL ? NDArray_FDATA(gamma) : NULL, NDArray_FDATA(save_mean),
                              NDArray_FDATA(save_invstd), b.N, b.C, b.inner, NDArray_FDATA(dx), NDArray_FDATA(dgamma),
                              NDArray_FDATA(dbeta)) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, dx, dgamma, dbeta);
    }
    rtns[0] = dx, rtns[1] = dgamma, rtns[2] = dbeta;
    return rtns;
}


/* ---- layer and group normalization (hip_dnn.h): np_groupnorm_forward / np_groupnorm_backward ---- */

typedef struct { size_t N, G, D, inner; } nph_groupnorm;

/* a new GPU array of ndim >= 1 extents */
static NDArray *empty_of_ints_on_gpu(const int *dims, int ndim) {
    int *shape = (int *) NPH_ALLOC(sizeof(int) * (size_t) ndim);
    if (shape == NULL) return NULL;
    for (int d = 0; d < ndim; ++d) shape[d] = dims[d];
    NDArray *rtn = NDArray_Empty(shape, ndim, "float32", NDARRAY_DEVICE_GPU);
    if (NPH_SHAPE_IS_COPIED) NPH_RELEASE(shape);
    return rtn;
}

/* 1 when a has exactly the ndim extents of dims */
static int has_shape(NDArray *a, const int *dims, int ndim) {
    if (NDArray_NDIM(a) != ndim) return 0;
    for (int d = 0; d < ndim; ++d)
        if (NDArray_SHAPE(a)[d] != dims[d]) return 0;
    return 1;
}

/* the messages of one of the two layers, in the order of the checks they share */
typedef struct { const char *empty, *gamma, *beta, *saved, *gradient, *eps, *device, *cpu; } nph_norm_messages;
static const nph_norm_messages nph_ln_messages = {NPH_LN_MSG_EMPTY, NPH_LN_MSG_GAMMA, NPH_LN_MSG_BETA, NPH_LN_MSG_SAVED, NPH_LN_MSG_GRADIENT,
                                                  NPH_LN_MSG_EPS, NPH_LN_MSG_DEVICE, NPH_LN_MSG_CPU};
static const nph_norm_messages nph_gn_messages = {NPH_GN_MSG_EMPTY, NPH_GN_MSG_GAMMA, NPH_GN_MSG_BETA, NPH_GN_MSG_SAVED, NPH_GN_MSG_GRADIENT,
                                                  NPH_GN_MSG_EPS, NPH_GN_MSG_DEVICE, NPH_GN_MSG_CPU};

/* the checks both layers and both directions share once the geometry is known, in the order of hip_dnn.h: the parameters have
 * the par_ndim extents of par, the saved statistics the stat_ndim extents of stat.  Absent operands are NULL.  0 after a raised
 * error */
static int norm_operands(const nph_norm_messages *msg, NDArray *x, NDArray *dy, NDArray *gamma, NDArray *beta, NDArray *mean, NDArray *invstd,
                         const int *par, int par_ndim, const int *stat, int stat_ndim, double eps, const nph_groupnorm *b) {
    if (b->N < 1 || b->G < 1 || b->D < 1 || b->inner < 1) {
        np_ext_throw(msg->empty);
        return 0;
    }
    if (gamma != NULL && !has_shape(gamma, par, par_ndim)) {
        np_ext_throw(msg->gamma);
        return 0;
    }
    if (beta != NULL && !has_shape(beta, par, par_ndim)) {
        np_ext_throw(msg->beta);
        return 0;
    }
    if ((mean != NULL && !has_shape(mean, stat, stat_ndim)) || (invstd != NULL && !has_shape(invstd, stat, stat_ndim))) {
        np_ext_throw(msg->saved);
        return 0;
    }
    if (dy != NULL && !has_shape(dy, NDArray_SHAPE(x), NDArray_NDIM(x))) {
        np_ext_throw(msg->gradient);
        return 0;
    }
    if (!(eps >= 0.0)) {
        np_ext_throw(msg->eps);
        return 0;
    }
    NDArray *others[5] = {dy, gamma, beta, mean, invstd};
    for (int k = 0; k < 5; ++k)
        if (others[k] != NULL && NDArray_DEVICE(others[k]) != NDArray_DEVICE(x)) {
            np_ext_throw(msg->device);
            return 0;
        }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(msg->cpu);
        return 0;
    }
    return 1;
}

/* layer normalization's geometry: (M, 1, L, 1).  *stat / *stat_ndim: the leading shape ((1) when there is no leading axis) */
static int layernorm_of(NDArray *x, NDArray *dy, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *beta, NDArray *mean,
                        NDArray *invstd, double eps, nph_groupnorm *b, const int **stat, int *stat_ndim) {
    static const int one = 1;
    const int ndim = NDArray_NDIM(x), lead = ndim - normalized_ndim;
    if (normalized_shape == NULL || normalized_ndim < 1 || normalized_ndim > ndim) {
        np_ext_throw(NPH_LN_MSG_NDIM);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x);
    for (int d = 0; d < normalized_ndim; ++d)
        if (normalized_shape[d] != xs[lead + d]) {
            np_ext_throw(NPH_LN_MSG_SHAPE);
            return 0;
        }
    b->N = 1, b->G = 1, b->D = 1, b->inner = 1;
    for (int d = 0; d < lead; ++d) b->N *= (size_t) (xs[d] > 0 ? xs[d] : 0);
    for (int d = lead; d < ndim; ++d) b->D *= (size_t) (xs[d] > 0 ? xs[d] : 0);
    *stat = lead > 0 ? xs : &one, *stat_ndim = lead > 0 ? lead : 1;
    return norm_operands(&nph_ln_messages, x, dy, gamma, beta, mean, invstd, xs + lead, normalized_ndim, *stat, *stat_ndim, eps, b);
}

/* group normalization's geometry: (N, G, C / G, inner).  stat: room for the two extents (N, G) */
static int groupnorm_of(NDArray *x, NDArray *dy, int num_groups, NDArray *gamma, NDArray *beta, NDArray *mean, NDArray *invstd, double eps,
                        nph_groupnorm *b, int *stat) {
    const int ndim = NDArray_NDIM(x);
    if (ndim < 2) {
        np_ext_throw(NPH_GN_MSG_NDIM);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x);
    const int C = xs[1];
    b->inner = 1;
    for (int d = 2; d < ndim; ++d) b->inner *= (size_t) (xs[d] > 0 ? xs[d] : 0);
    if (xs[0] < 1 || C < 1 || b->inner < 1) {
        np_ext_throw(NPH_GN_MSG_EMPTY);
        return 0;
    }
    if (num_groups < 1) {
        np_ext_throw(NPH_GN_MSG_GROUPS);
        return 0;
    }
    if (C % num_groups != 0) {
        np_ext_throw(NPH_GN_MSG_DIVISIBLE);
        return 0;
    }
    b->N = (size_t) xs[0], b->G = (size_t) num_groups, b->D = (size_t) (C / num_groups);
    stat[0] = xs[0], stat[1] = num_groups;
    return norm_operands(&nph_gn_messages, x, dy, gamma, beta, mean, invstd, &C, 1, stat, 2, eps, b);
}

/* the forward call on checked operands: (y, save_mean, save_invstd), the statistics with the stat_ndim extents of stat */
static NDArray **norm_forward(NDArray *x, NDArray *gamma, NDArray *beta, double eps, const nph_groupnorm *b, const int *stat, int stat_ndim) {
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *y = empty_like_on_gpu(x), *mean = empty_of_ints_on_gpu(stat, stat_ndim), *invstd = empty_of_ints_on_gpu(stat, stat_ndim);
    if (rtns == NULL || y == NULL || mean == NULL || invstd == NULL) return batchnorm_drop(rtns, y, mean, invstd);
    if (np_groupnorm_forward(NDArray_FDATA(x), gamma != NULL ? NDArray_FDATA(gamma) : NULL, beta != NULL ? NDArray_FDATA(beta) : NULL, b->N, b->G,
                             b->D, b->inner, eps, NDArray_FDATA(y), NDArray_FDATA(mean), NDArray_FDATA(invstd)) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, y, mean, invstd);
    }
    rtns[0] = y, rtns[1] = mean, rtns[2] = invstd;
    return rtns;
}

/* the backward call on checked operands: (dx, dgamma, dbeta), the gradients with the par_ndim extents of par */
static NDArray **norm_backward(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *mean, NDArray *invstd, const nph_groupnorm *b, const int *par,
                               int par_ndim) {
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *dx = empty_like_on_gpu(x), *dgamma = empty_of_ints_on_gpu(par, par_ndim), *dbeta = empty_of_ints_on_gpu(par, par_ndim);
    if (rtns == NULL || dx == NULL || dgamma == NULL || dbeta == NULL) return batchnorm_drop(rtns, dx, dgamma, dbeta);
    if (np_groupnorm_backward(NDArray_FDATA(x), NDArray_FDATA(dy), gamma != NULL ? NDArray_FDATA(gamma) : NULL, NDArray_FDATA(mean),
                              NDArray_FDATA(invstd), b->N, b->G, b->D, b->inner, NDArray_FDATA(dx), NDArray_FDATA(dgamma),
                              NDArray_FDATA(dbeta)) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, dx, dgamma, dbeta);
    }
    rtns[0] = dx, rtns[1] = dgamma, rtns[2] = dbeta;
    return rtns;
}

NDArray **NPH_LayerNorm_Forward(NDArray *x, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *beta, double eps) {
    nph_groupnorm b;
    const int *stat;
    int stat_ndim;
    if (x == NULL || !layernorm_of(x, NULL, normalized_shape, normalized_ndim, gamma, beta, NULL, NULL, eps, &b, &stat, &stat_ndim)) return NULL;
    return norm_forward(x, gamma, beta, eps, &b, stat, stat_ndim);
}

NDArray **NPH_LayerNorm_Backward(NDArray *x, NDArray *dy, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *save_mean,
                                 NDArray *save_invstd) {
    nph_groupnorm b;
    const int *stat;
    int stat_ndim;
    if (x == NULL || dy == NULL || save_mean == NULL || save_invstd == NULL) return NULL;
    if (!layernorm_of(x, dy, normalized_shape, normalized_ndim, gamma, NULL, save_mean, save_invstd, 0.0, &b, &stat, &stat_ndim)) return NULL;
    return norm_backward(x, dy, gamma, save_mean, save_invstd, &b, NDArray_SHAPE(x) + (NDArray_NDIM(x) - normalized_ndim), normalized_ndim);
}

NDArray **NPH_GroupNorm_Forward(NDArray *x, int num_groups, NDArray *gamma, NDArray *beta, double eps) {
    nph_groupnorm b;
    int stat[2];
    if (x == NULL || !groupnorm_of(x, NULL, num_groups, gamma, beta, NULL, NULL, eps, &b, stat)) return NULL;
    return norm_forward(x, gamma, beta, eps, &b, stat, 2);
}

NDArray **NPH_GroupNorm_Backward(NDArray *x, NDArray *dy, int num_groups, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd) {
    nph_groupnorm b;
    int stat[2];
    if (x == NULL || dy == NULL || save_mean == NULL || save_invstd == NULL) return NULL;
    if (!groupnorm_of(x, dy, num_groups, gamma, NULL, save_mean, save_invstd, 0.0, &b, stat)) return NULL;
    return norm_backward(x, dy, gamma, save_mean, save_invstd, &b, &NDArray_SHAPE(x)[1], 1);
}


/* ---- scaled dot-product attention (hip_dnn.h): np_attention_forward / np_attention_backward ---- */

typedef struct { size_t BH, Sq, Sk, D; float scale; } nph_attention;

/* the checks of both directions, in the order of hip_dnn.h.  Absent operands are NULL.  0 after a raised error */
static int attention_of(NDArray *q, NDArray *k, NDArray *v, NDArray *o, NDArray *dout, NDArray *smax, NDArray *ssum, float scale, nph_attention *a) {
    const int ndim = NDArray_NDIM(q);
    if (ndim < 2 || NDArray_NDIM(k) != ndim || NDArray_NDIM(v) != ndim) {
        np_ext_throw(NPH_ATTN_MSG_NDIM);
        return 0;
    }
    const int *qs = NDArray_SHAPE(q), *ks = NDArray_SHAPE(k), *vs = NDArray_SHAPE(v);
    a->BH = 1;
    for (int d = 0; d < ndim - 2; ++d) {
        if (ks[d] != qs[d] || vs[d] != qs[d]) {
            np_ext_throw(NPH_ATTN_MSG_LEADING);
            return 0;
        }
        a->BH *= (size_t) (qs[d] > 0 ? qs[d] : 0);
    }
    if (ks[ndim - 1] != qs[ndim - 1] || vs[ndim - 1] != qs[ndim - 1]) {
        np_ext_throw(NPH_ATTN_MSG_D);
        return 0;
    }
    if (ks[ndim - 2] != vs[ndim - 2]) {
        np_ext_throw(NPH_ATTN_MSG_SK);
        return 0;
    }
    if (a->BH < 1 || qs[ndim - 2] < 1 || ks[ndim - 2] < 1 || qs[ndim - 1] < 1) {
        np_ext_throw(NPH_ATTN_MSG_EMPTY);
        return 0;
    }
    a->Sq = (size_t) qs[ndim - 2], a->Sk = (size_t) ks[ndim - 2], a->D = (size_t) qs[ndim - 1];
    if (a->D > 128) {
        np_ext_throw(NPH_ATTN_MSG_DMAX);
        return 0;
    }
    if ((o != NULL && !has_shape(o, qs, ndim)) || (dout != NULL && !has_shape(dout, qs, ndim))) {
        np_ext_throw(NPH_ATTN_MSG_OUTPUT);
        return 0;
    }
    if ((smax != NULL && !has_shape(smax, qs, ndim - 1)) || (ssum != NULL && !has_shape(ssum, qs, ndim - 1))) {
        np_ext_throw(NPH_ATTN_MSG_SAVED);
        return 0;
    }
    if (scale > 0.0f && scale - scale != 0.0f) {
        np_ext_throw(NPH_ATTN_MSG_SCALE);
        return 0;
    }
    a->scale = scale > 0.0f ? scale : 1.0f / sqrtf((float) a->D);      /* not greater than zero, or a NaN: the default */
    NDArray *others[6] = {k, v, o, dout, smax, ssum};
    for (int i = 0; i < 6; ++i)
        if (others[i] != NULL && NDArray_DEVICE(others[i]) != NDArray_DEVICE(q)) {
            np_ext_throw(NPH_ATTN_MSG_DEVICE);
            return 0;
        }
    if (NDArray_DEVICE(q) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_ATTN_MSG_CPU);
        return 0;
    }
    return 1;
}

NDArray **NPH_Attention_Forward(NDArray *q, NDArray *k, NDArray *v, int causal, float scale) {
    nph_attention a;
    if (q == NULL || k == NULL || v == NULL || !attention_of(q, k, v, NULL, NULL, NULL, NULL, scale, &a)) return NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *o = empty_like_on_gpu(q), *smax = empty_of_ints_on_gpu(NDArray_SHAPE(q), NDArray_NDIM(q) - 1);
    NDArray *ssum = empty_of_ints_on_gpu(NDArray_SHAPE(q), NDArray_NDIM(q) - 1);
    if (rtns == NULL || o == NULL || smax == NULL || ssum == NULL) return batchnorm_drop(rtns, o, smax, ssum);
    if (np_attention_forward(NDArray_FDATA(q), NDArray_FDATA(k), NDArray_FDATA(v), a.BH, a.Sq, a.Sk, a.D, causal, a.scale, NDArray_FDATA(o),
                             NDArray_FDATA(smax), NDArray_FDATA(ssum)) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, o, smax, ssum);
    }
    rtns[0] = o, rtns[1] = smax, rtns[2] = ssum;
    return rtns;
}

NDArray **NPH_Attention_Backward(NDArray *q, NDArray *k, NDArray *v, NDArray *o, NDArray *dout, NDArray *save_max, NDArray *save_sum, int causal,
                                 float scale) {
    nph_attention a;
    if (q == NULL || k == NULL || v == NULL || o == NULL || dout == NULL || save_max == NULL || save_sum == NULL) return NULL;
    if (!attention_of(q, k, v, o, dout, save_max, save_sum, scale, &a)) return NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *dq = empty_like_on_gpu(q), *dk = empty_like_on_gpu(k), *dv = empty_like_on_gpu(v);
    if (rtns == NULL || dq == NULL || dk == NULL || dv == NULL) return batchnorm_drop(rtns, dq, dk, dv);
    if (np_attention_backward(NDArray_FDATA(q), NDArray_FDATA(k), NDArray_FDATA(v), NDArray_FDATA(o), NDArray_FDATA(dout), NDArray_FDATA(save_max),
                              NDArray_FDATA(save_sum), a.BH, a.Sq, a.Sk, a.D, causal, a.scale, NDArray_FDATA(dq), NDArray_FDATA(dk),
                              NDArray_FDATA(dv)) != NP_OK) {
        np_ext_throw_last();
        return batchnorm_drop(rtns, dq, dk, dv);
    }
    rtns[0] = dq, rtns[1] = dk, rtns[2] = dv;
    return rtns;
}


/* ---- optimizer steps (hip_dnn.h): np_sgd_step / np_adam_step / np_grad_norm ---- */

/* the device pointers and element counts of a call's lists, one block that is released on every path */
typedef struct { void *block; float **p, **g, **s1, **s2; size_t *n; } nph_optim;

static void optim_release(nph_optim *o) {
    if (o->block != NULL) NPH_RELEASE(o->block);
    o->block = NULL;
}

/* the checks the three calls share, in the order of hip_dnn.h; lists[0] leads (the parameters, or the gradients of the norm), a
 * NULL list is absent; refusal: the message of the call's first bad parameter, or NULL.  Fills o.  0 after a raised error */
static int optim_of(NDArray **lists[4], const int lens[4], NDArray *grad_scale, int grad_scale_index, const char *refusal, nph_optim *o) {
    o->block = NULL;
    const int T = lens[0];
    for (int l = 1; l < 4; ++l)
        if (lists[l] != NULL && lens[l] != T) {
            np_ext_throw(NPH_OPTIM_MSG_LENGTHS);
            return 0;
        }
    for (int l = 0; l < 4; ++l)
        for (int t = 0; lists[l] != NULL && t < T; ++t)
            if (lists[l][t] == NULL) {
                np_ext_throw(NPH_OPTIM_MSG_NULL);
                return 0;
            }
    if (lists[0] == NULL || T < 1) {
        np_ext_throw(NPH_OPTIM_MSG_EMPTY_LIST);
        return 0;
    }
    for (int t = 0; t < T; ++t) {
        const long n = NDArray_NUMELEMENTS(lists[0][t]);
        if (n < 1) {
            np_ext_throw(NPH_OPTIM_MSG_EMPTY);
            return 0;
        }
        for (int l = 1; l < 4; ++l)
            if (lists[l] != NULL && NDArray_NUMELEMENTS(lists[l][t]) != n) {
                np_ext_throw(NDArray_NUMELEMENTS(lists[l][t]) < 1 ? NPH_OPTIM_MSG_EMPTY : NPH_OPTIM_MSG_COUNT);
                return 0;
            }
    }
    if (grad_scale != NULL && (grad_scale_index < 0 || (long) grad_scale_index >= NDArray_NUMELEMENTS(grad_scale))) {
        np_ext_throw(NPH_OPTIM_MSG_SCALE);
        return 0;
    }
    if (refusal != NULL) {
        np_ext_throw(refusal);
        return 0;
    }
    const int device = NDArray_DEVICE(lists[0][0]);
    for (int l = 0; l < 4; ++l)
        for (int t = 0; lists[l] != NULL && t < T; ++t)
            if (NDArray_DEVICE(lists[l][t]) != device) {
                np_ext_throw(NPH_OPTIM_MSG_DEVICE);
                return 0;
            }
    if (grad_scale != NULL && NDArray_DEVICE(grad_scale) != device) {
        np_ext_throw(NPH_OPTIM_MSG_DEVICE);
        return 0;
    }
    if (device != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_OPTIM_MSG_CPU);
        return 0;
    }
    o->block = NPH_ALLOC((size_t) T * (4 * sizeof(float *) + sizeof(size_t)));
    if (o->block == NULL) return 0;
    o->p = (float **) o->block, o->g = o->p + T, o->s1 = o->g + T, o->s2 = o->s1 + T, o->n = (size_t *) (o->s2 + T);
    float **into[4] = {o->p, o->g, o->s1, o->s2};
    for (int t = 0; t < T; ++t) {
        o->n[t] = (size_t) NDArray_NUMELEMENTS(lists[0][t]);
        for (int l = 0; l < 4; ++l) into[l][t] = lists[l] != NULL ? NDArray_FDATA(lists[l][t]) : NULL;
    }
    return 1;
}

static int optim_finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

int NPH_SGD_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **bufs, int n_bufs, double lr, double momentum,
                 double dampening, double weight_decay, int nesterov, int first_step, NDArray *grad_scale, int grad_scale_index) {
    nph_optim o;
    NDArray **lists[4] = {params, grads, bufs, NULL};
    const int lens[4] = {n_params, grads != NULL ? n_grads : -1, n_bufs, 0};
    if (momentum != 0.0 && bufs == NULL) {
        np_ext_throw(params != NULL && grads != NULL && n_params == n_grads ? NPH_OPTIM_MSG_BUFFERS : NPH_OPTIM_MSG_LENGTHS);
        return 0;
    }
    if (grads == NULL) {
        np_ext_throw(NPH_OPTIM_MSG_LENGTHS);
        return 0;
    }
    const char *msg = !optim_finite_nonneg(lr) ? NPH_OPTIM_MSG_LR
                      : !optim_finite_nonneg(weight_decay) ? NPH_OPTIM_MSG_WEIGHT_DECAY
                      : !(momentum >= 0.0 && momentum <= 1.0) ? NPH_OPTIM_MSG_MOMENTUM
                      : !(dampening >= 0.0 && dampening <= 1.0) ? NPH_OPTIM_MSG_DAMPENING
                      : (nesterov && (momentum == 0.0 || dampening != 0.0)) ? NPH_OPTIM_MSG_NESTEROV : NULL;
    if (!optim_of(lists, lens, grad_scale, grad_scale_index, msg, &o)) return 0;
    const int ok = np_sgd_step((float *const *) o.p, (const float *const *) o.g, momentum != 0.0 ? (float *const *) o.s1 : NULL, o.n, (size_t) n_params,
                               lr, momentum, dampening, weight_decay, nesterov, first_step,
                               grad_scale != NULL ? NDArray_FDATA(grad_scale) + grad_scale_index : NULL) == NP_OK;
    if (!ok) np_ext_throw_last();
    optim_release(&o);
    return ok;
}

int NPH_Adam_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **exp_avg, int n_exp_avg, NDArray **exp_avg_sq,
                  int n_exp_avg_sq, long step, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                  NDArray *grad_scale, int grad_scale_index) {
    nph_optim o;
    NDArray **lists[4] = {params, grads, exp_avg, exp_avg_sq};
    const int lens[4] = {n_params, n_grads, n_exp_avg, n_exp_avg_sq};
    if (grads == NULL || exp_avg == NULL || exp_avg_sq == NULL) {
        np_ext_throw(NPH_OPTIM_MSG_LENGTHS);
        return 0;
    }
    const char *msg = !optim_finite_nonneg(lr) ? NPH_OPTIM_MSG_LR
                      : !optim_finite_nonneg(weight_decay) ? NPH_OPTIM_MSG_WEIGHT_DECAY
                      : (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) ? NPH_OPTIM_MSG_BETAS
                      : !optim_finite_nonneg(eps) ? NPH_OPTIM_MSG_EPS
                      : step < 1 ? NPH_OPTIM_MSG_STEP : NULL;
    if (!optim_of(lists, lens, grad_scale, grad_scale_index, msg, &o)) return 0;
    const int ok = np_adam_step((float *const *) o.p, (const float *const *) o.g, (float *const *) o.s1, (float *const *) o.s2, o.n, (size_t) n_params,
                                (long long) step, lr, beta1, beta2, eps, weight_decay, decoupled,
                                grad_scale != NULL ? NDArray_FDATA(grad_scale) + grad_scale_index : NULL) == NP_OK;
    if (!ok) np_ext_throw_last();
    optim_release(&o);
    return ok;
}

NDArray *NPH_GradNorm(NDArray **grads, int n_grads, double max_norm) {
    nph_optim o;
    NDArray **lists[4] = {grads, NULL, NULL, NULL};
    const int lens[4] = {n_grads, 0, 0, 0};
    if (!optim_of(lists, lens, NULL, 0, !(max_norm >= 0.0) ? NPH_OPTIM_MSG_MAX_NORM : NULL, &o)) return NULL;
    const size_t two = 2;
    NDArray *out = empty_on_gpu(1, &two);
    if (out != NULL && np_grad_norm((const float *const *) o.p, o.n, (size_t) n_grads, max_norm, NDArray_FDATA(out)) != NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(out);
        out = NULL;
    }
    optim_release(&o);
    return out;
}


/* ---- dense layers (hip_dnn.h): np_linear_forward / np_linear_backward ---- */

typedef struct { size_t M, K, N; } nph_linear;

/* the checks of both directions, in the order of hip_dnn.h.  bias, out and dy may be NULL; out is compared only with an
 * activation.  0 after a raised error */
static int linear_of(NDArray *x, NDArray *weight, NDArray *bias, NDArray *out, NDArray *dy, int act, nph_linear *l) {
    if (act < 0) {
        np_ext_throw(NPH_LINEAR_MSG_ACTIVATION);
        return 0;
    }
    const int ndim = NDArray_NDIM(x);
    if (ndim < 1 || NDArray_NDIM(weight) != 2) {
        np_ext_throw(NPH_LINEAR_MSG_NDIM);
        return 0;
    }
    const int *xs = NDArray_SHAPE(x), *ws = NDArray_SHAPE(weight);
    if (xs[ndim - 1] != ws[1]) {
        np_ext_throw(NPH_LINEAR_MSG_FEATURES);
        return 0;
    }
    if (bias != NULL && (NDArray_NDIM(bias) != 1 || NDArray_SHAPE(bias)[0] != ws[0])) {
        np_ext_throw(NPH_LINEAR_MSG_BIAS);
        return 0;
    }
    l->M = 1;
    for (int d = 0; d < ndim - 1; ++d) l->M *= (size_t) (xs[d] > 0 ? xs[d] : 0);
    if (l->M < 1 || ws[0] < 1 || ws[1] < 1) {
        np_ext_throw(NPH_LINEAR_MSG_EMPTY);
        return 0;
    }
    l->K = (size_t) ws[1], l->N = (size_t) ws[0];
    if (dy != NULL) {
        int same = NDArray_NDIM(dy) == ndim && NDArray_SHAPE(dy)[ndim - 1] == ws[0];
        for (int d = 0; same && d < ndim - 1; ++d) same = NDArray_SHAPE(dy)[d] == xs[d];
        if (!same) {
            np_ext_throw(NPH_LINEAR_MSG_GRADIENT);
            return 0;
        }
        if (act != NP_ACT_NONE && (out == NULL || !has_shape(out, NDArray_SHAPE(dy), ndim))) {
            np_ext_throw(NPH_LINEAR_MSG_OUT);
            return 0;
        }
    }
    NDArray *others[4] = {weight, bias, act != NP_ACT_NONE ? out : NULL, dy};
    for (int i = 0; i < 4; ++i)
        if (others[i] != NULL && NDArray_DEVICE(others[i]) != NDArray_DEVICE(x)) {
            np_ext_throw(NPH_LINEAR_MSG_DEVICE);
            return 0;
        }
    if (NDArray_DEVICE(x) != NDARRAY_DEVICE_GPU) {
        np_ext_throw(NPH_LINEAR_MSG_CPU);
        return 0;
    }
    return 1;
}

NDArray *NPH_Linear_Forward(NDArray *x, NDArray *weight, NDArray *bias, char activation) {
    nph_linear l;
    const int act = activation_of(activation);
    if (x == NULL || weight == NULL || !linear_of(x, weight, bias, NULL, NULL, act, &l)) return NULL;
    const int ndim = NDArray_NDIM(x);
    int *dims = (int *) NPH_ALLOC(sizeof(int) * (size_t) ndim);
    if (dims == NULL) return NULL;
    for (int d = 0; d < ndim - 1; ++d) dims[d] = NDArray_SHAPE(x)[d];
    dims[ndim - 1] = (int) l.N;
    NDArray *y = empty_of_ints_on_gpu(dims, ndim);
    NPH_RELEASE(dims);
    if (y == NULL) return NULL;
    if (np_linear_forward(NDArray_FDATA(x), NDArray_FDATA(weight), bias != NULL ? NDArray_FDATA(bias) : NULL, l.M, l.K, l.N, act, NDArray_FDATA(y)) !=
        NP_OK) {
        np_ext_throw_last();
        NDArray_FREE(y);
        return NULL;
    }
    return y;
}

NDArray **NPH_Linear_Backward(NDArray *x, NDArray *out, NDArray *dy, NDArray *weight, char activation, int use_bias, int need_dx) {
    nph_linear l;
    const int act = activation_of(activation);
    if (x == NULL || dy == NULL || weight == NULL || !linear_of(x, weight, NULL, out, dy, act, &l)) return NULL;
    NDArray **rtns = (NDArray **) NPH_ALLOC(sizeof(NDArray *) * 3);
    NDArray *dw = empty_like_on_gpu(weight), *dx = need_dx ? empty_like_on_gpu(x) : NULL, *db = use_bias ? empty_on_gpu(1, &l.N) : NULL;
    void *dz = NULL;   /* pool scratch, only with an activation: dz = dy otherwise */
    int ok = rtns != NULL && dw != NULL && (dx != NULL || !need_dx) && (db != NULL || !use_bias);
    if (ok && act != NP_ACT_NONE && np_malloc(&dz, l.M * l.N * sizeof(float)) != NP_OK) {
        np_ext_throw_last();
        dz = NULL;
        ok = 0;
    }
    if (ok && np_linear_backward(NDArray_FDATA(x), NDArray_FDATA(weight), act != NP_ACT_NONE ? NDArray_FDATA(out) : NULL, NDArray_FDATA(dy), l.M, l.K,
                                 l.N, act, (float *) dz, dx != NULL ? NDArray_FDATA(dx) : NULL, NDArray_FDATA(dw),
                                 db != NULL ? NDArray_FDATA(db) : NULL) != NP_OK) {
        np_ext_throw_last();
        ok = 0;
    }
    if (dz != NULL) np_free(dz);   /* released on every path; the pool is stream-ordered: safe right behind the launches that read it */
    if (!ok) return batchnorm_drop(rtns, dw, dx, db);
    rtns[0] = dw, rtns[1] = dx, rtns[2] = db;
    return rtns;
}
