/*
 * hip_dnn.h — dnn_conv2d_forward / dnn_conv2d_backward of GPU arrays on the device convolution layer (np_conv2d_forward,
 * np_conv2d_backward_data, np_conv2d_backward_filter of include/np_hip.h).
 *
 * The reference computes these on the CPU, or through cuDNN when it is built with HAVE_CUDNN; a --with-hip tree never defines
 * that name, so for a GPU array NDArrayDNN_Conv2D_Forward / _Backward (dnn.c:273-368) throw "DNN features for GPU not enabled.
 * ..." (dnn.c:305, 361).  `tools/apply_with_hip.py --dnn` inserts one early-out at the top of each function, which replaces
 * nothing:
 *
 *     NDArrayDNN_Conv2D_Forward at the top
 *         if (NPH_DNN_TAKES(x, filters)) return NPH_Conv2D_Forward(x, filters);
 *     NDArrayDNN_Conv2D_Backward at the top, before its first allocation
 *         if (NPH_DNN_TAKES3(input, y, filters)) return NPH_Conv2D_Backward(input, y, filters);
 *
 * guarded by `#ifdef HAVE_NP_HIP`: CPU operands fall through to the reference's code, untouched; as soon as ONE operand lives on
 * the GPU the call is taken, so a mixed pair (which the reference would read blindly) is refused here with a message.
 *
 * What is computed: x (N, C, H, W), filters (F, C, kh, kw), cross-correlation, stride 1, no padding ('valid'),
 * no bias, no activation — the reference ignores `activation` and `use_bias` on both paths, and `kernel_size` is ignored here.
 * Where the reference's CPU path is inconsistent this glue defines the mathematics and does NOT follow it:
 *   - F is filters.shape[0], as the reference's backward and its cuDNN filter descriptor read it (its forward reads shape[3]);
 *   - kh != kw is allowed (the reference reads shape[2] for both);
 *   - dW comes back in the filters' own shape (F, C, kh, kw), not as the all-axes NDArray_Transpose view the reference wraps it in;
 *   - the reference's backward swaps out_w and out_h, and sizes its im2col workspace as N.C.H.W floats for a C.k^2.oh.ow matrix;
 *   - NDArray_DNN_Conv1D is a placeholder with hard-coded extents and stays out.
 *
 * Plain C over the reference's headers in a PHP build (results are the reference's own arrays and die in its NDArray_FREE), over
 * include/numpower_host.h in libnumpower_host.so, whose NDArrayDNN_Conv2D_Forward / _Backward call these functions after making
 * their operands contiguous.  Operands must be contiguous (the reference's arrays are).
 * Errors: this project's messages, the reference has none and reads blindly; NULL after a raised error.
 */
#ifndef NUMPOWER_AMD_EXT_HIP_DNN_H
#define NUMPOWER_AMD_EXT_HIP_DNN_H

#ifdef __cplusplus
extern "C" {
#endif

struct NDArray;

/* true when the early-out takes the call: at least one operand lives on the GPU */
#define NPH_DNN_TAKES(a, b) (NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU || NDArray_DEVICE(b) == NDARRAY_DEVICE_GPU)
#define NPH_DNN_TAKES3(a, b, c) (NPH_DNN_TAKES(a, b) || NDArray_DEVICE(c) == NDARRAY_DEVICE_GPU)

/* The messages, checked in this order (the fourth by NPH_Conv2D_Backward alone). */
#define NPH_DNN_MSG_NDIM "dnn_conv2d: the operands must be 4-dimensional: the input (N, C, H, W), the filters (F, C, kh, kw)"
#define NPH_DNN_MSG_CHANNELS "dnn_conv2d: the filters' second extent must equal the input's number of channels"
#define NPH_DNN_MSG_WINDOW "dnn_conv2d: the filter window must not be larger than the input (kh <= H and kw <= W)"
#define NPH_DNN_MSG_GRADIENT "dnn_conv2d_backward: the gradient must have the shape of the forward result (N, F, H - kh + 1, W - kw + 1)"
#define NPH_DNN_MSG_DEVICE "dnn_conv2d: the operands must be on the same device"
#define NPH_DNN_MSG_CPU "dnn_conv2d: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first, the CPU path is the reference's own)"

/* y (N, F, H - kh + 1, W - kw + 1), a new GPU array */
struct NDArray *NPH_Conv2D_Forward(struct NDArray *x, struct NDArray *filters);
/* y: the gradient of the forward result, of its shape.  A vector of two new GPU arrays in the reference's order, rtn[0] = dW
 * (F, C, kh, kw), rtn[1] = dX (N, C, H, W); the vector is emalloc'd in a PHP build (the reference efree's it), malloc'd in
 * libnumpower_host.so. */
struct NDArray **NPH_Conv2D_Backward(struct NDArray *x, struct NDArray *y, struct NDArray *filters);

/* ---- with a stride, a padding and a dilation (np_conv2d_*_ex of include/np_hip.h; DESIGN.md §3.14 "the general gather") ----
 * The reference's layer names strides, padding and dilation_rate (dnn.c:196-200) and then hard-wires stride 1, no padding; its
 * two functions above have no argument for them.  These two are what a binding with such arguments calls: each of stride,
 * padding, dilation is (rows, columns), NULL meaning (1, 1), (0, 0), (1, 1).  The effective window is dilation . (k - 1) + 1;
 * y (N, F, oh, ow) with oh = floor((H + 2 ph - keh) / sh) + 1.  The messages above, with these four in place of
 * NPH_DNN_MSG_WINDOW and NPH_DNN_MSG_GRADIENT, checked in this order after the channels: */
#define NPH_DNN_MSG_STRIDE "dnn_conv2d: the stride must be at least 1 along both axes"
#define NPH_DNN_MSG_DILATION "dnn_conv2d: the dilation must be at least 1 along both axes"
#define NPH_DNN_MSG_PADDING "dnn_conv2d: the padding must be at least 0 and smaller than the effective window, dilation . (k - 1) + 1"
#define NPH_DNN_MSG_EFFECTIVE "dnn_conv2d: the effective window, dilation . (k - 1) + 1, must not be larger than the padded input (H + 2 ph, W + 2 pw)"
#define NPH_DNN_MSG_STRIDED_GRADIENT "dnn_conv2d_backward: the gradient must have the shape of the forward result (N, F, (H + 2 ph - keh) / sh + 1, (W + 2 pw - kew) / sw + 1)"

struct NDArray *NPH_Conv2D_ForwardEx(struct NDArray *x, struct NDArray *filters, const int stride[2], const int padding[2], const int dilation[2]);
/* {dW (F, C, kh, kw), dX (N, C, H, W)} as NPH_Conv2D_Backward; rows and columns of x that no window reads get dX = +0 */
struct NDArray **NPH_Conv2D_BackwardEx(struct NDArray *x, struct NDArray *y, struct NDArray *filters, const int stride[2], const int padding[2],
                                       const int dilation[2]);

/* ---- the layer: a bias per filter and an activation (np_conv2d_forward_act / np_conv2d_backward_act of include/np_hip.h) ----
 * The reference's signature names `activation` and `use_bias`, has no bias operand and ignores both; the functions above keep
 * ignoring them.  These two are what a binding with a bias argument calls.  activation: 'r' relu, 't' tanh, 's' sigmoid, 'n' or 0
 * none.  y = act(conv(x, filters) + bias[f]): the bias is ONE fp32 add after the reduction, the activation runs in the forward
 * kernel's store loop.  The backward pass takes `out`, the forward RESULT (gradients are expressed through the output, a layer
 * keeps no pre-activation), and dy, the gradient of that result: dz = dy . act'(out) goes to pool scratch, is released on every
 * path, and dW and dX are the Ex gradients of dz; db[f] = sum_{n,i,j} dz.
 * The messages: these four, checked in this order BEFORE the ones above (the last needs its operands' devices): */
#define NPH_DNN_MSG_ACTIVATION "dnn_conv2d: unknown activation: 'r' (relu), 't' (tanh), 's' (sigmoid), 'n' or 0 (none)"
#define NPH_DNN_MSG_BIAS "dnn_conv2d: the bias must be 1-dimensional with one element per filter (F,)"
#define NPH_DNN_MSG_OUT "dnn_conv2d_backward: out, the forward result, must have the shape of the gradient"
#define NPH_DNN_MSG_BIAS_DEVICE "dnn_conv2d: the bias must be on the device of the input and the filters"

/* y (N, F, oh, ow), a new GPU array; bias: 1-D (F,) on the GPU, or NULL */
struct NDArray *NPH_Conv2D_LayerForward(struct NDArray *x, struct NDArray *filters, struct NDArray *bias, const int stride[2], const int padding[2],
                                        const int dilation[2], char activation);
/* A vector of THREE: rtn[0] = dW, rtn[1] = dX as NPH_Conv2D_BackwardEx, rtn[2] = db (F,), NULL without use_bias.  `out` may be
 * NULL when the activation is none. */
struct NDArray **NPH_Conv2D_LayerBackward(struct NDArray *x, struct NDArray *out, struct NDArray *dy, struct NDArray *filters, const int stride[2],
                                          const int padding[2], const int dilation[2], char activation, int use_bias);

/* ---- pooling: max and average pool2d (np_pool2d_forward / np_pool2d_backward of include/np_hip.h) ----
 * The reference has no pooling, so tools/apply_with_hip.py inserts nothing for these two; they are what a binding with a pooling
 * method calls.  x is (N, C, H, W) and is pooled as N.C planes.  kernel is (kh, kw); stride is (sh, sw), NULL meaning the window;
 * padding is (ph, pw), NULL meaning 0, with 2 ph <= kh and 2 pw <= kw.  mode: 'm' max, 'a' average with divisor kh.kw (padding
 * counts), 'v' average over the real cells.  No dilation, no ceil mode.  y (N, C, oh, ow), oh = floor((H + 2 ph - kh) / sh) + 1.
 * The backward pass keeps no state between calls: it takes the layer's input x, as the convolution's does.  For max it runs the
 * forward kernel again, y and idx both going to ONE block of pool scratch (the C ABI has no index-only call; y is a quarter of x
 * or less for a stride of 2), then gathers; the scratch is released on every path.  For the average modes x supplies the shape
 * only and is not read.
 * The messages, checked in this order (the gradient's by NPH_Pool2D_Backward alone): */
#define NPH_POOL_MSG_MODE "dnn_pool2d: unknown mode: 'm' (max), 'a' (average, padding counts), 'v' (average over the real cells)"
#define NPH_POOL_MSG_NDIM "dnn_pool2d: the input must be 4-dimensional (N, C, H, W), and so must the gradient"
#define NPH_POOL_MSG_WINDOW "dnn_pool2d: the window must be at least 1 along both axes"
#define NPH_POOL_MSG_STRIDE "dnn_pool2d: the stride must be at least 1 along both axes"
#define NPH_POOL_MSG_PADDING "dnn_pool2d: the padding must be at least 0 and at most half the window (2 ph <= kh and 2 pw <= kw)"
#define NPH_POOL_MSG_LARGER "dnn_pool2d: the window must not be larger than the padded input (H + 2 ph, W + 2 pw)"
#define NPH_POOL_MSG_GRADIENT "dnn_pool2d_backward: the gradient must have the shape of the forward result (N, C, (H + 2 ph - kh) / sh + 1, (W + 2 pw - kw) / sw + 1)"
#define NPH_POOL_MSG_DEVICE "dnn_pool2d: the operands must be on the same device"
#define NPH_POOL_MSG_CPU "dnn_pool2d: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"

/* y (N, C, oh, ow), a new GPU array */
struct NDArray *NPH_Pool2D_Forward(struct NDArray *x, const int kernel[2], const int stride[2], const int padding[2], char mode);
/* dx (N, C, H, W), a new GPU array; dy: the gradient of the forward result, of its shape.  Cells that no window covers get +0 */
struct NDArray *NPH_Pool2D_Backward(struct NDArray *x, struct NDArray *dy, const int kernel[2], const int stride[2], const int padding[2], char mode);

/* ---- softmax, log-softmax and cross-entropy (np_softmax_forward / _backward, np_cross_entropy of include/np_hip.h) ----
 * The reference has none of them, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods calls.
 * x has any ndim >= 1 and is seen as (outer, cols, inner) around `axis` (negative axes count from the end).  mode: 's' softmax,
 * 'l' log-softmax.  The backward pass works from the OUTPUT y of the forward pass and the gradient dy of that output.
 * The cross-entropy takes 2-D logits (rows, cols) and a target that is either (rows) class indices stored as fp32 or
 * (rows, cols) probabilities.  reduction: 'n' none: the (rows) losses, scale 1; 's' sum: the library's sum of those losses (np_reduce_all),
 * scale 1; 'm' mean: that sum divided once by (float) rows, scale = 1.0f / (float) rows.  With with_grad, *dlogits receives
 * (softmax - target) . scale from the same launch.  A sum or a mean is returned as a 0-dimensional array.
 * The messages, checked in this order (the gradient's by NPH_Softmax_Backward alone; the logits', target's and reduction's by
 * NPH_CrossEntropy alone): */
#define NPH_SOFTMAX_MSG_MODE "softmax: unknown mode: 's' (softmax), 'l' (log-softmax)"
#define NPH_SOFTMAX_MSG_AXIS "softmax: the axis is out of range for the operand's dimensions"
#define NPH_SOFTMAX_MSG_GRADIENT "softmax_backward: the gradient must have the shape of the output"
#define NPH_XENT_MSG_LOGITS "dnn_cross_entropy: the logits must be 2-dimensional (rows, classes)"
#define NPH_XENT_MSG_TARGET "dnn_cross_entropy: the target must be (rows) class indices or (rows, classes) probabilities"
#define NPH_XENT_MSG_REDUCTION "dnn_cross_entropy: unknown reduction: 'n' (none), 's' (sum), 'm' (mean)"
#define NPH_SOFTMAX_MSG_DEVICE "softmax: the operands must be on the same device"
#define NPH_SOFTMAX_MSG_CPU "softmax: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"
#define NPH_XENT_MSG_DEVICE "dnn_cross_entropy: the operands must be on the same device"
#define NPH_XENT_MSG_CPU "dnn_cross_entropy: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"

/* y, a new GPU array of x's shape */
struct NDArray *NPH_Softmax_Forward(struct NDArray *x, int axis, char mode);
/* dx, a new GPU array of y's shape */
struct NDArray *NPH_Softmax_Backward(struct NDArray *y, struct NDArray *dy, int axis, char mode);
/* the loss; *dlogits (when with_grad != 0 and dlogits != NULL) a new GPU array of the logits' shape, NULL after an error */
struct NDArray *NPH_CrossEntropy(struct NDArray *logits, struct NDArray *target, char reduction, int with_grad, struct NDArray **dlogits);

/* ---- batch normalization (np_batchnorm_forward / _backward of include/np_hip.h) ----
 * The reference has no normalization layer, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods
 * calls.  x has ndim >= 2 with the channel on axis 1 and is seen as (N, C, inner) = (shape[0], shape[1], the product of the rest).
 * gamma, beta, the running statistics and the saved statistics are (C) arrays; gamma, beta and, in training, the running
 * statistics may be NULL.  Training returns y, save_mean and save_invstd and updates the running statistics in place;
 * inference (training == 0) needs both running statistics and returns y alone.  The backward pass is training mode's.
 * The messages, checked in this order (the saved statistics' and the gradient's by NPH_BatchNorm_Backward alone; the running
 * statistics', eps', momentum's and the last by NPH_BatchNorm_Forward alone): */
#define NPH_BN_MSG_NDIM "dnn_batch_norm: the input must have at least 2 dimensions (N, C, ...)"
#define NPH_BN_MSG_EMPTY "dnn_batch_norm: an operand has no elements"
#define NPH_BN_MSG_GAMMA "dnn_batch_norm: gamma must be a (C) array, C = the input's shape[1]"
#define NPH_BN_MSG_BETA "dnn_batch_norm: beta must be a (C) array, C = the input's shape[1]"
#define NPH_BN_MSG_RUNNING "dnn_batch_norm: running_mean and running_var must be (C) arrays, C = the input's shape[1]"
#define NPH_BN_MSG_INFERENCE "dnn_batch_norm: inference needs both running_mean and running_var"
#define NPH_BN_MSG_SAVED "dnn_batch_norm_backward: save_mean and save_invstd must be (C) arrays, C = the input's shape[1]"
#define NPH_BN_MSG_GRADIENT "dnn_batch_norm_backward: the gradient must have the shape of the input"
#define NPH_BN_MSG_EPS "dnn_batch_norm: eps must not be negative"
#define NPH_BN_MSG_MOMENTUM "dnn_batch_norm: momentum must lie in [0, 1]"
#define NPH_BN_MSG_DEVICE "dnn_batch_norm: the operands must be on the same device"
#define NPH_BN_MSG_CPU "dnn_batch_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"
#define NPH_BN_MSG_ONE_VALUE "dnn_batch_norm: training needs more than one value per channel"
/* raised by the host library: a running statistic that had to be copied (a view) could not be updated in place */
#define NPH_BN_MSG_RUNNING_VIEW "dnn_batch_norm: the running statistics are updated in place and must be contiguous arrays"

/* a vector of three new GPU arrays: y in x's shape, save_mean (C), save_invstd (C); in inference the last two are NULL */
struct NDArray **NPH_BatchNorm_Forward(struct NDArray *x, struct NDArray *gamma, struct NDArray *beta, struct NDArray *running_mean,
                                       struct NDArray *running_var, int training, double momentum, double eps);
/* a vector of three new GPU arrays: dx in x's shape, dgamma (C), dbeta (C) */
struct NDArray **NPH_BatchNorm_Backward(struct NDArray *x, struct NDArray *dy, struct NDArray *gamma, struct NDArray *save_mean,
                                        struct NDArray *save_invstd);

/* ---- layer and group normalization (np_groupnorm_forward / _backward of include/np_hip.h) ----
 * The reference has no normalization layer, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods
 * calls.
 * Layer normalization: normalized_shape (normalized_ndim >= 1 extents) must equal x's trailing axes; x is seen as (M, L), M the
 * product of the leading axes; gamma and beta have the normalized shape or are NULL; the statistics have the leading shape ((1)
 * when the normalized shape is the whole of x).
 * Group normalization: x has ndim >= 2 with the channel on axis 1 and is seen as (N, G, C / G, inner); gamma and beta are (C)
 * arrays or NULL; the statistics are (N, G) arrays.  Instance normalization is num_groups = C.
 * The messages, checked in this order (the saved statistics' and the gradient's by the backward passes alone, eps' by the forward
 * passes alone): */
#define NPH_LN_MSG_NDIM "dnn_layer_norm: normalized_shape must have between 1 and the input's number of dimensions"
#define NPH_LN_MSG_SHAPE "dnn_layer_norm: normalized_shape must equal the input's trailing axes"
#define NPH_LN_MSG_EMPTY "dnn_layer_norm: an operand has no elements"
#define NPH_LN_MSG_GAMMA "dnn_layer_norm: gamma must have the normalized shape"
#define NPH_LN_MSG_BETA "dnn_layer_norm: beta must have the normalized shape"
#define NPH_LN_MSG_SAVED "dnn_layer_norm_backward: save_mean and save_invstd must have the shape of the input's leading axes"
#define NPH_LN_MSG_GRADIENT "dnn_layer_norm_backward: the gradient must have the shape of the input"
#define NPH_LN_MSG_EPS "dnn_layer_norm: eps must not be negative"
#define NPH_LN_MSG_DEVICE "dnn_layer_norm: the operands must be on the same device"
#define NPH_LN_MSG_CPU "dnn_layer_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"
#define NPH_GN_MSG_NDIM "dnn_group_norm: the input must have at least 2 dimensions (N, C, ...)"
#define NPH_GN_MSG_EMPTY "dnn_group_norm: an operand has no elements"
#define NPH_GN_MSG_GROUPS "dnn_group_norm: num_groups must be at least 1"
#define NPH_GN_MSG_DIVISIBLE "dnn_group_norm: C = the input's shape[1] must be divisible by num_groups"
#define NPH_GN_MSG_GAMMA "dnn_group_norm: gamma must be a (C) array, C = the input's shape[1]"
#define NPH_GN_MSG_BETA "dnn_group_norm: beta must be a (C) array, C = the input's shape[1]"
#define NPH_GN_MSG_SAVED "dnn_group_norm_backward: save_mean and save_invstd must be (N, num_groups) arrays"
#define NPH_GN_MSG_GRADIENT "dnn_group_norm_backward: the gradient must have the shape of the input"
#define NPH_GN_MSG_EPS "dnn_group_norm: eps must not be negative"
#define NPH_GN_MSG_DEVICE "dnn_group_norm: the operands must be on the same device"
#define NPH_GN_MSG_CPU "dnn_group_norm: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"

/* a vector of three new GPU arrays: y in x's shape, save_mean and save_invstd in the leading shape */
struct NDArray **NPH_LayerNorm_Forward(struct NDArray *x, const int *normalized_shape, int normalized_ndim, struct NDArray *gamma,
                                       struct NDArray *beta, double eps);
/* a vector of three new GPU arrays: dx in x's shape, dgamma and dbeta in the normalized shape */
struct NDArray **NPH_LayerNorm_Backward(struct NDArray *x, struct NDArray *dy, const int *normalized_shape, int normalized_ndim,
                                        struct NDArray *gamma, struct NDArray *save_mean, struct NDArray *save_invstd);
/* a vector of three new GPU arrays: y in x's shape, save_mean (N, num_groups), save_invstd (N, num_groups) */
struct NDArray **NPH_GroupNorm_Forward(struct NDArray *x, int num_groups, struct NDArray *gamma, struct NDArray *beta, double eps);
/* a vector of three new GPU arrays: dx in x's shape, dgamma (C), dbeta (C) */
struct NDArray **NPH_GroupNorm_Backward(struct NDArray *x, struct NDArray *dy, int num_groups, struct NDArray *gamma,
                                        struct NDArray *save_mean, struct NDArray *save_invstd);

/* ---- scaled dot-product attention (np_attention_forward / _backward of include/np_hip.h) ----
 * The reference has no attention, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods calls.
 * q is (..., Sq, D), k and v are (..., Sk, D) with ndim >= 2; the leading axes must be equal across q, k and v and are flattened to
 * BH (1 without leading axes).  o and dout have q's shape; the statistics have q's shape without its last axis.
 * scale: a value that is not greater than zero (0, a negative number, a NaN) means the default 1 / sqrt(D).
 * The messages, checked in this order (the output's, the gradient's and the statistics' by the backward pass alone): */
#define NPH_ATTN_MSG_NDIM "dnn_attention: q, k and v must have at least 2 dimensions (..., S, D) and the same number of them"
#define NPH_ATTN_MSG_LEADING "dnn_attention: the leading axes of q, k and v must be equal"
#define NPH_ATTN_MSG_D "dnn_attention: q, k and v must have the same last axis D"
#define NPH_ATTN_MSG_SK "dnn_attention: k and v must have the same number of rows Sk"
#define NPH_ATTN_MSG_EMPTY "dnn_attention: an operand has no elements"
#define NPH_ATTN_MSG_DMAX "dnn_attention: D, the last axis, must not be above 128"
#define NPH_ATTN_MSG_OUTPUT "dnn_attention_backward: o and dout must have the shape of q"
#define NPH_ATTN_MSG_SAVED "dnn_attention_backward: save_max and save_sum must have the shape of q without its last axis"
#define NPH_ATTN_MSG_SCALE "dnn_attention: scale must be finite"
#define NPH_ATTN_MSG_DEVICE "dnn_attention: the operands must be on the same device"
#define NPH_ATTN_MSG_CPU "dnn_attention: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"

/* a vector of three new GPU arrays: o in q's shape, save_max and save_sum in q's shape without its last axis */
struct NDArray **NPH_Attention_Forward(struct NDArray *q, struct NDArray *k, struct NDArray *v, int causal, float scale);
/* a vector of three new GPU arrays: dq in q's shape, dk in k's shape, dv in v's shape */
struct NDArray **NPH_Attention_Backward(struct NDArray *q, struct NDArray *k, struct NDArray *v, struct NDArray *o, struct NDArray *dout,
                                        struct NDArray *save_max, struct NDArray *save_sum, int causal, float scale);

/* ---- optimizer steps (np_sgd_step / np_adam_step / np_grad_norm of include/np_hip.h) ----
 * The reference has no optimizer, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods calls.
 * A call takes LISTS of arrays: n_params parameters, as many gradients and, where the rule has a state, as many state arrays, entry
 * t of each list belonging to tensor t.  Parameters and states are updated in place; a gradient must have as many elements as its
 * parameter (the shapes are not compared).  grad_scale, when not NULL, is a GPU array and grad_scale_index the element of it that
 * the kernel multiplies every gradient by: (the result of NPH_GradNorm, 1) clips by the norm with no host read.
 * The messages, checked in this order (the buffers', momentum's, dampening's and nesterov's by NPH_SGD_Step alone; the betas', eps'
 * and step's by NPH_Adam_Step alone; max_norm's by NPH_GradNorm alone, which has no parameters and no states): */
#define NPH_OPTIM_MSG_LENGTHS "dnn_optim: the lists of parameters, gradients and states must have the same length"
#define NPH_OPTIM_MSG_NULL "dnn_optim: a list holds an entry that is not an array"
#define NPH_OPTIM_MSG_EMPTY_LIST "dnn_optim: the list is empty"
#define NPH_OPTIM_MSG_BUFFERS "dnn_sgd_step: a momentum needs the list of buffers"
#define NPH_OPTIM_MSG_EMPTY "dnn_optim: an operand has no elements"
#define NPH_OPTIM_MSG_COUNT "dnn_optim: a gradient or a state must have as many elements as its parameter"
#define NPH_OPTIM_MSG_SCALE "dnn_optim: grad_scale must be an array and grad_scale_index an element of it"
#define NPH_OPTIM_MSG_LR "dnn_optim: lr must be finite and not negative"
#define NPH_OPTIM_MSG_WEIGHT_DECAY "dnn_optim: weight_decay must be finite and not negative"
#define NPH_OPTIM_MSG_MOMENTUM "dnn_sgd_step: momentum must lie in [0, 1]"
#define NPH_OPTIM_MSG_DAMPENING "dnn_sgd_step: dampening must lie in [0, 1]"
#define NPH_OPTIM_MSG_NESTEROV "dnn_sgd_step: nesterov needs a momentum and zero dampening"
#define NPH_OPTIM_MSG_BETAS "dnn_adam_step: the betas must lie in [0, 1)"
#define NPH_OPTIM_MSG_EPS "dnn_adam_step: eps must be finite and not negative"
#define NPH_OPTIM_MSG_STEP "dnn_adam_step: step must be at least 1"
#define NPH_OPTIM_MSG_MAX_NORM "dnn_grad_norm: max_norm must not be negative"
#define NPH_OPTIM_MSG_DEVICE "dnn_optim: the operands must be on the same device"
#define NPH_OPTIM_MSG_CPU "dnn_optim: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"
/* raised by the host library: a parameter or a state that had to be copied (a view) could not be updated in place */
#define NPH_OPTIM_MSG_VIEW "dnn_optim: parameters and states are updated in place and must be contiguous arrays"

/* 1, or 0 after a raised error (nothing was launched).  bufs may be NULL (n_bufs = 0) when momentum == 0 */
int NPH_SGD_Step(struct NDArray **params, int n_params, struct NDArray **grads, int n_grads, struct NDArray **bufs, int n_bufs, double lr,
                 double momentum, double dampening, double weight_decay, int nesterov, int first_step, struct NDArray *grad_scale,
                 int grad_scale_index);
int NPH_Adam_Step(struct NDArray **params, int n_params, struct NDArray **grads, int n_grads, struct NDArray **exp_avg, int n_exp_avg,
                  struct NDArray **exp_avg_sq, int n_exp_avg_sq, long step, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int decoupled, struct NDArray *grad_scale, int grad_scale_index);
/* a new (2) GPU array: the norm of the list and the clip coefficient for max_norm (+Inf: 1) */
struct NDArray *NPH_GradNorm(struct NDArray **grads, int n_grads, double max_norm);

/* ---- dense layers (np_linear_forward / _backward of include/np_hip.h) ----
 * The reference has no dense layer, so tools/apply_with_hip.py inserts nothing; they are what a binding with these methods calls.
 * torch's layout: x is (..., K) with ndim >= 1, its leading axes flattened to M rows (1 without one); weight is (N, K); bias is a
 * 1-D (N,) array or NULL; y and dy are x's shape with N in place of K.  activation: 'r' relu, 't' tanh, 's' sigmoid, 'n' or 0
 * none.  y = act(x . weight^T + bias[n]): the bias is ONE fp32 add after the reduction, the activation runs in the same kernel.
 * The backward pass takes `out`, the forward RESULT (gradients are expressed through the output), and dy, the gradient of that
 * result: dz = dy . act'(out) goes to pool scratch that is released on every path.
 * The messages, checked in this order (out's and the gradient's by NPH_Linear_Backward alone): */
#define NPH_LINEAR_MSG_ACTIVATION "dnn_linear: unknown activation: 'r' (relu), 't' (tanh), 's' (sigmoid), 'n' or 0 (none)"
#define NPH_LINEAR_MSG_NDIM "dnn_linear: x must have at least 1 dimension (..., K) and the weight exactly 2 (N, K)"
#define NPH_LINEAR_MSG_FEATURES "dnn_linear: the last axis of x must equal the weight's second axis K (in_features)"
#define NPH_LINEAR_MSG_BIAS "dnn_linear: the bias must be 1-dimensional with one element per output feature (N,)"
#define NPH_LINEAR_MSG_EMPTY "dnn_linear: an operand has no elements"
#define NPH_LINEAR_MSG_GRADIENT "dnn_linear_backward: the gradient must have the shape of the forward result (..., N)"
#define NPH_LINEAR_MSG_OUT "dnn_linear_backward: an activation needs out, the forward result, in the shape of the gradient"
#define NPH_LINEAR_MSG_DEVICE "dnn_linear: the operands must be on the same device"
#define NPH_LINEAR_MSG_CPU "dnn_linear: operands are on the CPU; numpower_amd only computes on the GPU (call ->gpu() first)"

/* y (..., N), a new GPU array */
struct NDArray *NPH_Linear_Forward(struct NDArray *x, struct NDArray *weight, struct NDArray *bias, char activation);
/* A vector of THREE, the conv layer's order: rtn[0] = dW (N, K), rtn[1] = dX in x's shape, NULL without need_dx (and then no
 * launch is spent on it), rtn[2] = db (N,), NULL without use_bias.  `out` may be NULL when the activation is none. */
struct NDArray **NPH_Linear_Backward(struct NDArray *x, struct NDArray *out, struct NDArray *dy, struct NDArray *weight, char activation,
                                     int use_bias, int need_dx);

#ifdef __cplusplus
}
#endif
#endif
