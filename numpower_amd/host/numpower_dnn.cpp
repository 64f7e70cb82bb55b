// NDArrayDNN_Conv2D_Forward / _Backward (dnn.c:273-368, dnn.h:7-8) on the device convolution layer (np_conv2d_forward,
// np_conv2d_backward_data, np_conv2d_backward_filter).
// The work — argument checks, this project's messages, the result arrays, the np_conv2d_* calls — is ext/hip_dnn.c, the same
// code a `--dnn` --with-hip tree reaches through the early-outs tools/apply_with_hip.py inserts at the top of the reference's
// functions; here strided views of the operands are first made contiguous (numpower_host_contiguous).  kernel_size, activation
// and use_bias are the reference's parameters and are ignored, as the reference ignores the last two on both of its paths.
// The host library has no CPU convolution: CPU operands get the glue's message.
// NDArrayDNN_Pool2D_Forward / _Backward at the end are the pooling layers (np_pool2d_forward / _backward), which
// the reference does not have; the same glue file does their work.
// A translation unit of its own: the sanitizer build of numpower_host.cpp (tests/test_host_sanitizers_cpu.py) links
// against a null device that has no convolution.
#include <deque>
#include <optional>
#include <vector>

#include "hip_dnn.h"
#include "np_ext_hooks.h"
#include "numpower_host.h"
#include "numpower_operand.h"

using numpower_host::Operand;

namespace {

// glue(a, b, c, d) for up to four operands, nullptr for one the call does not have.  CPU operands are handed on as they are:
// they only ever meet the argument checks and the device messages.  Otherwise each operand is made contiguous for the call,
// in argument order; nullptr at the first that cannot be.
template <class Glue>
auto on_contiguous(Glue glue, NDArray *a, NDArray *b, NDArray *c = nullptr, NDArray *d = nullptr) -> decltype(glue(a, b, c, d)) {
    NDArray *arr[4] = {a, b, c, d};
    for (NDArray *p : arr)
        if (p && NDArray_DEVICE(p) != NDARRAY_DEVICE_GPU) return glue(a, b, c, d);
    std::optional<Operand> held[4];
    for (int i = 0; i < 4; ++i) {
        if (!arr[i]) continue;
        arr[i] = held[i].emplace(arr[i]).arr;
        if (!arr[i]) return nullptr;
    }
    return glue(arr[0], arr[1], arr[2], arr[3]);
}

// The lists of an optimizer call, each entry made contiguous for the call (take, in argument order).  A list that is NULL or
// holds a NULL or a CPU array is handed on as it is: it only ever meets the glue's checks.  in_place: a list that the call
// updates, so an entry that had to be copied is refused.
struct OptimLists {
    std::deque<Operand> held;
    std::deque<std::vector<NDArray *>> lists;
    std::vector<NDArray **> given;

    bool take(NDArray **list, int n, bool in_place) {
        lists.emplace_back();
        given.push_back(list);
        if (!list || n < 1) return true;
        for (int i = 0; i < n; ++i)
            if (!list[i] || NDArray_DEVICE(list[i]) != NDARRAY_DEVICE_GPU) return true;
        std::vector<NDArray *> &out = lists.back();
        for (int i = 0; i < n; ++i) {
            NDArray *c = held.emplace_back(list[i]).arr;
            if (!c) return false;
            if (in_place && c != list[i]) {
                np_ext_throw(NPH_OPTIM_MSG_VIEW);
                return false;
            }
            out.push_back(c);
        }
        return true;
    }
    // list k as the glue takes it
    NDArray **at(size_t k) { return lists[k].empty() ? given[k] : lists[k].data(); }
};

}  // namespace

extern "C" {

NDArray *NDArrayDNN_Conv2D_Forward(NDArray *x, NDArray *filters, int *kernel_size, char activation, int use_bias) {
    (void) kernel_size, (void) activation, (void) use_bias;
    if (!x || !filters) return nullptr;
    return on_contiguous([](NDArray *cx, NDArray *cf, NDArray *, NDArray *) { return NPH_Conv2D_Forward(cx, cf); }, x, filters);
}

NDArray **NDArrayDNN_Conv2D_Backward(NDArray *input, NDArray *y, NDArray *filters, int kernel_size, char activation, int use_bias) {
    (void) kernel_size, (void) activation, (void) use_bias;
    if (!input || !y || !filters) return nullptr;
    return on_contiguous([](NDArray *cx, NDArray *cy, NDArray *cf, NDArray *) { return NPH_Conv2D_Backward(cx, cy, cf); }, input, y, filters);
}

// The same layer with a stride, a padding and a dilation ((rows, columns) each, nullptr: 1, 0, 1): what the reference's layer
// signature names (dnn.c:196-200) and its functions cannot express.
NDArray *NDArrayDNN_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int *stride, const int *padding, const int *dilation) {
    if (!x || !filters) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cf, NDArray *, NDArray *) { return NPH_Conv2D_ForwardEx(cx, cf, stride, padding, dilation); }, x,
                         filters);
}

NDArray **NDArrayDNN_Conv2D_BackwardEx(NDArray *input, NDArray *y, NDArray *filters, const int *stride, const int *padding, const int *dilation) {
    if (!input || !y || !filters) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cy, NDArray *cf, NDArray *) { return NPH_Conv2D_BackwardEx(cx, cy, cf, stride, padding, dilation); },
                         input, y, filters);
}

// The layer with a bias per filter (1-D (F,), or nullptr) and an activation ('r', 't', 's', 'n' or 0): what a binding with a bias
// argument calls.  The reference-signature functions at the top keep ignoring `activation` and `use_bias`.
NDArray *NDArrayDNN_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int *stride, const int *padding, const int *dilation,
                                        char activation) {
    if (!x || !filters) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cf, NDArray *cb, NDArray *) {
        return NPH_Conv2D_LayerForward(cx, cf, cb, stride, padding, dilation, activation);
    }, x, filters, bias);
}

// out: the forward result (may be nullptr without an activation); dy: its gradient.  A malloc'd vector of three: dW, dX and db
// (nullptr without use_bias).
NDArray **NDArrayDNN_Conv2D_LayerBackward(NDArray *input, NDArray *out, NDArray *dy, NDArray *filters, const int *stride, const int *padding,
                                          const int *dilation, char activation, int use_bias) {
    if (!input || !dy || !filters) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cy, NDArray *cf, NDArray *co) {
        return NPH_Conv2D_LayerBackward(cx, co, cy, cf, stride, padding, dilation, activation, use_bias);
    }, input, dy, filters, out);
}

// Pooling (np_pool2d_forward / _backward): x (N, C, H, W); kernel (kh, kw); stride nullptr: the window; padding
// nullptr: 0; mode 'm' max, 'a' average with divisor kh.kw, 'v' average over the real cells.  The reference has no pooling.
NDArray *NDArrayDNN_Pool2D_Forward(NDArray *x, const int *kernel, const int *stride, const int *padding, char mode) {
    if (!x) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *, NDArray *, NDArray *) { return NPH_Pool2D_Forward(cx, kernel, stride, padding, mode); }, x,
                         nullptr);
}

// dx (N, C, H, W) for dy = the gradient of that result; x is the layer's input (max reads it again, the averages take its shape).
NDArray *NDArrayDNN_Pool2D_Backward(NDArray *x, NDArray *dy, const int *kernel, const int *stride, const int *padding, char mode) {
    if (!x || !dy) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cy, NDArray *, NDArray *) { return NPH_Pool2D_Backward(cx, cy, kernel, stride, padding, mode); }, x,
                         dy);
}

// Softmax, log-softmax and cross-entropy (np_softmax_forward / _backward, np_cross_entropy), which the reference
// does not have either.  mode 's' softmax, 'l' log-softmax; reduction 'n', 's', 'm'.
NDArray *NDArrayDNN_Softmax_Forward(NDArray *x, int axis, char mode) {
    if (!x) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *, NDArray *, NDArray *) { return NPH_Softmax_Forward(cx, axis, mode); }, x, nullptr);
}

// dx for y = the forward result and dy = its gradient
NDArray *NDArrayDNN_Softmax_Backward(NDArray *y, NDArray *dy, int axis, char mode) {
    if (!y || !dy) return nullptr;
    return on_contiguous([=](NDArray *cy, NDArray *cg, NDArray *, NDArray *) { return NPH_Softmax_Backward(cy, cg, axis, mode); }, y, dy);
}

// the loss ((rows), or 0-dimensional); *dlogits: a new array when with_grad, nullptr after an error
NDArray *NDArrayDNN_CrossEntropy(NDArray *logits, NDArray *target, char reduction, int with_grad, NDArray **dlogits) {
    if (dlogits) *dlogits = nullptr;
    if (!logits || !target) return nullptr;
    return on_contiguous([=](NDArray *cl, NDArray *ct, NDArray *, NDArray *) { return NPH_CrossEntropy(cl, ct, reduction, with_grad, dlogits); },
                         logits, target);
}

// Batch normalization (np_batchnorm_forward / _backward), which the reference does not have either.  gamma, beta
// and, in training, the running statistics may be nullptr.  The running statistics are updated in place: one that had to be
// copied to become contiguous (a view) is refused in training.
NDArray **NDArrayDNN_BatchNorm_Forward(NDArray *x, NDArray *gamma, NDArray *beta, NDArray *running_mean, NDArray *running_var, int training,
                                       double momentum, double eps) {
    if (!x) return nullptr;
    return on_contiguous(
        [=](NDArray *cx, NDArray *cg, NDArray *cb, NDArray *) -> NDArray ** {
            return on_contiguous(
                [=](NDArray *cm, NDArray *cv, NDArray *, NDArray *) -> NDArray ** {
                    if (training && (cm != running_mean || cv != running_var)) {
                        np_ext_throw(NPH_BN_MSG_RUNNING_VIEW);
                        return nullptr;
                    }
                    return NPH_BatchNorm_Forward(cx, cg, cb, cm, cv, training, momentum, eps);
                },
                running_mean, running_var);
        },
        x, gamma, beta);
}

// (dx, dgamma, dbeta) of training mode, from the layer's input and the statistics the forward pass saved
NDArray **NDArrayDNN_BatchNorm_Backward(NDArray *x, NDArray *dy, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd) {
    if (!x || !dy || !save_mean || !save_invstd) return nullptr;
    return on_contiguous(
        [=](NDArray *cx, NDArray *cd, NDArray *cm, NDArray *cv) -> NDArray ** {
            return on_contiguous([=](NDArray *cg, NDArray *, NDArray *, NDArray *) -> NDArray ** { return NPH_BatchNorm_Backward(cx, cd, cg, cm, cv); },
                                 gamma, nullptr);
        },
        x, dy, save_mean, save_invstd);
}

// Layer and group normalization (np_groupnorm_forward / _backward), which the reference does not have either.
// normalized_shape: the normalized_ndim trailing extents of x; gamma and beta may be nullptr.
NDArray **NDArrayDNN_LayerNorm_Forward(NDArray *x, const int *normalized_shape, int normalized_ndim, NDArray *gamma, NDArray *beta, double eps) {
    if (!x) return nullptr;
    return on_contiguous(
        [=](NDArray *cx, NDArray *cg, NDArray *cb, NDArray *) -> NDArray ** {
            return NPH_LayerNorm_Forward(cx, normalized_shape, normalized_ndim, cg, cb, eps);
        },
        x, gamma, beta);
}

// (dx, dgamma, dbeta) from the layer's input and the statistics the forward pass saved
NDArray **NDArrayDNN_LayerNorm_Backward(NDArray *x, NDArray *dy, const int *normalized_shape, int normalized_ndim, NDArray *gamma,
                                        NDArray *save_mean, NDArray *save_invstd) {
    if (!x || !dy || !save_mean || !save_invstd) return nullptr;
    return on_contiguous(
        [=](NDArray *cx, NDArray *cd, NDArray *cm, NDArray *cv) -> NDArray ** {
            return on_contiguous(
                [=](NDArray *cg, NDArray *, NDArray *, NDArray *) -> NDArray ** {
                    return NPH_LayerNorm_Backward(cx, cd, normalized_shape, normalized_ndim, cg, cm, cv);
                },
                gamma, nullptr);
        },
        x, dy, save_mean, save_invstd);
}

// x (N, C, ...) in num_groups groups of C / num_groups channels; instance normalization is num_groups = C
NDArray **NDArrayDNN_GroupNorm_Forward(NDArray *x, int num_groups, NDArray *gamma, NDArray *beta, double eps) {
    if (!x) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cg, NDArray *cb, NDArray *) -> NDArray ** { return NPH_GroupNorm_Forward(cx, num_groups, cg, cb, eps); },
                         x, gamma, beta);
}

NDArray **NDArrayDNN_GroupNorm_Backward(NDArray *x, NDArray *dy, int num_groups, NDArray *gamma, NDArray *save_mean, NDArray *save_invstd) {
    if (!x || !dy || !save_mean || !save_invstd) return nullptr;
    return on_contiguous(
        [=](NDArray *cx, NDArray *cd, NDArray *cm, NDArray *cv) -> NDArray ** {
            return on_contiguous(
                [=](NDArray *cg, NDArray *, NDArray *, NDArray *) -> NDArray ** { return NPH_GroupNorm_Backward(cx, cd, num_groups, cg, cm, cv); }, gamma,
                nullptr);
        },
        x, dy, save_mean, save_invstd);
}

// Scaled dot-product attention (np_attention_forward / _backward), which the reference does not have either.
// scale: not greater than zero, or a NaN, means 1 / sqrt(D).
NDArray **NDArrayDNN_Attention_Forward(NDArray *q, NDArray *k, NDArray *v, int causal, float scale) {
    if (!q || !k || !v) return nullptr;
    return on_contiguous([=](NDArray *cq, NDArray *ck, NDArray *cv, NDArray *) -> NDArray ** { return NPH_Attention_Forward(cq, ck, cv, causal, scale); },
                         q, k, v);
}

// (dq, dk, dv) from the layer's operands, its output, the gradient of the output and the statistics the forward pass saved
NDArray **NDArrayDNN_Attention_Backward(NDArray *q, NDArray *k, NDArray *v, NDArray *o, NDArray *dout, NDArray *save_max, NDArray *save_sum,
                                        int causal, float scale) {
    if (!q || !k || !v || !o || !dout || !save_max || !save_sum) return nullptr;
    return on_contiguous(
        [=](NDArray *cq, NDArray *ck, NDArray *cv, NDArray *co) -> NDArray ** {
            return on_contiguous(
                [=](NDArray *cd, NDArray *cm, NDArray *cs, NDArray *) -> NDArray ** {
                    return NPH_Attention_Backward(cq, ck, cv, co, cd, cm, cs, causal, scale);
                },
                dout, save_max, save_sum);
        },
        q, k, v, o);
}

// Optimizer steps (np_sgd_step / np_adam_step / np_grad_norm), which the reference does not have either.  The
// lists are handed to the glue as they are when they are malformed or hold a CPU array, so that its messages speak.  Otherwise
// gradients are made contiguous for the call; a parameter or state that would have to be copied (a view) is refused.
int NDArrayDNN_SGD_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **bufs, int n_bufs, double lr, double momentum,
                        double dampening, double weight_decay, int nesterov, int first_step, NDArray *grad_scale, int grad_scale_index) {
    OptimLists l;
    if (!l.take(params, n_params, true) || !l.take(grads, n_grads, false) || !l.take(bufs, n_bufs, true) || !l.take(&grad_scale, grad_scale ? 1 : 0, false))
        return 0;
    return NPH_SGD_Step(l.at(0), n_params, l.at(1), n_grads, l.at(2), n_bufs, lr, momentum, dampening, weight_decay, nesterov, first_step,
                        grad_scale ? l.at(3)[0] : nullptr, grad_scale_index);
}

int NDArrayDNN_Adam_Step(NDArray **params, int n_params, NDArray **grads, int n_grads, NDArray **exp_avg, int n_exp_avg, NDArray **exp_avg_sq,
                         int n_exp_avg_sq, long step, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                         NDArray *grad_scale, int grad_scale_index) {
    OptimLists l;
    if (!l.take(params, n_params, true) || !l.take(grads, n_grads, false) || !l.take(exp_avg, n_exp_avg, true) ||
        !l.take(exp_avg_sq, n_exp_avg_sq, true) || !l.take(&grad_scale, grad_scale ? 1 : 0, false))
        return 0;
    return NPH_Adam_Step(l.at(0), n_params, l.at(1), n_grads, l.at(2), n_exp_avg, l.at(3), n_exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay,
                         decoupled, grad_scale ? l.at(4)[0] : nullptr, grad_scale_index);
}

// a new (2) array: the norm of the list and the clip coefficient for max_norm
NDArray *NDArrayDNN_GradNorm(NDArray **grads, int n_grads, double max_norm) {
    OptimLists l;
    if (!l.take(grads, n_grads, false)) return nullptr;
    return NPH_GradNorm(l.at(0), n_grads, max_norm);
}

// Dense layers (np_linear_forward / _backward), which the reference does not have either.  bias may be nullptr;
// out may be nullptr without an activation.
NDArray *NDArrayDNN_Linear_Forward(NDArray *x, NDArray *weight, NDArray *bias, char activation) {
    if (!x || !weight) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cw, NDArray *cb, NDArray *) { return NPH_Linear_Forward(cx, cw, cb, activation); }, x, weight, bias);
}

// a malloc'd vector of three: dW, dX (nullptr without need_dx) and db (nullptr without use_bias)
NDArray **NDArrayDNN_Linear_Backward(NDArray *x, NDArray *out, NDArray *dy, NDArray *weight, char activation, int use_bias, int need_dx) {
    if (!x || !dy || !weight) return nullptr;
    return on_contiguous([=](NDArray *cx, NDArray *cy, NDArray *cw, NDArray *co) {
        return NPH_Linear_Backward(cx, co, cy, cw, activation, use_bias, need_dx);
    }, x, dy, weight, out);
}

}  // extern "C"
