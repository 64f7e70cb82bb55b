// NDArrayDNN_Conv2D_Forward / _Backward (dnn.c:273-368, dnn.h:7-8) on the device convolution layer (np_conv2d_forward,
// np_conv2d_backward_data, np_conv2d_backward_filter).
// The work — argument checks, this project's messages, the result arrays, the np_conv2d_* calls — is ext/hip_dnn.c, the same
// code a `--dnn` --with-hip tree reaches through the early-outs tools/apply_with_hip.py inserts at the top of the reference's
// functions; here strided views of the operands are first made contiguous (numpower_host_contiguous).  kernel_size, activation
// and use_bias are the reference's parameters and are ignored, as the reference ignores the last two on both of its paths.
// The host library has no CPU convolution: CPU operands get the glue's message.
// A translation unit of its own: the sanitizer build of numpower_host.cpp (tests/test_host_sanitizers_cpu.py) links
// against a null device that has no convolution.
#include "hip_dnn.h"
#include "numpower_host.h"
#include "numpower_operand.h"

using numpower_host::Operand;

namespace {

bool on_gpu(NDArray *a) { return NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU; }

}  // namespace

extern "C" {

NDArray *NDArrayDNN_Conv2D_Forward(NDArray *x, NDArray *filters, int *kernel_size, char activation, int use_bias) {
    (void) kernel_size, (void) activation, (void) use_bias;
    if (!x || !filters) return nullptr;
    // CPU operands are handed on as they are: they only ever meet the argument checks and the device messages
    if (!on_gpu(x) || !on_gpu(filters)) return NPH_Conv2D_Forward(x, filters);
    Operand cx(x);
    if (!cx.arr) return nullptr;
    Operand cf(filters);
    return cf.arr ? NPH_Conv2D_Forward(cx.arr, cf.arr) : nullptr;
}

NDArray **NDArrayDNN_Conv2D_Backward(NDArray *input, NDArray *y, NDArray *filters, int kernel_size, char activation, int use_bias) {
    (void) kernel_size, (void) activation, (void) use_bias;
    if (!input || !y || !filters) return nullptr;
    if (!on_gpu(input) || !on_gpu(y) || !on_gpu(filters)) return NPH_Conv2D_Backward(input, y, filters);
    Operand cx(input);
    if (!cx.arr) return nullptr;
    Operand cy(y);
    if (!cy.arr) return nullptr;
    Operand cf(filters);
    return cf.arr ? NPH_Conv2D_Backward(cx.arr, cy.arr, cf.arr) : nullptr;
}

// The same layer with a stride, a padding and a dilation ((rows, columns) each, nullptr: 1, 0, 1): what the reference's layer
// signature names (dnn.c:196-200) and its functions cannot express.
NDArray *NDArrayDNN_Conv2D_ForwardEx(NDArray *x, NDArray *filters, const int *stride, const int *padding, const int *dilation) {
    if (!x || !filters) return nullptr;
    if (!on_gpu(x) || !on_gpu(filters)) return NPH_Conv2D_ForwardEx(x, filters, stride, padding, dilation);
    Operand cx(x);
    if (!cx.arr) return nullptr;
    Operand cf(filters);
    return cf.arr ? NPH_Conv2D_ForwardEx(cx.arr, cf.arr, stride, padding, dilation) : nullptr;
}

NDArray **NDArrayDNN_Conv2D_BackwardEx(NDArray *input, NDArray *y, NDArray *filters, const int *stride, const int *padding, const int *dilation) {
    if (!input || !y || !filters) return nullptr;
    if (!on_gpu(input) || !on_gpu(y) || !on_gpu(filters)) return NPH_Conv2D_BackwardEx(input, y, filters, stride, padding, dilation);
    Operand cx(input);
    if (!cx.arr) return nullptr;
    Operand cy(y);
    if (!cy.arr) return nullptr;
    Operand cf(filters);
    return cf.arr ? NPH_Conv2D_BackwardEx(cx.arr, cy.arr, cf.arr, stride, padding, dilation) : nullptr;
}

// The layer with a bias per filter (1-D (F,), or nullptr) and an activation ('r', 't', 's', 'n' or 0): what a binding with a bias
// argument calls.  The reference-signature functions at the top keep ignoring `activation` and `use_bias`.
NDArray *NDArrayDNN_Conv2D_LayerForward(NDArray *x, NDArray *filters, NDArray *bias, const int *stride, const int *padding, const int *dilation,
                                        char activation) {
    if (!x || !filters) return nullptr;
    if (!on_gpu(x) || !on_gpu(filters) || (bias && !on_gpu(bias))) return NPH_Conv2D_LayerForward(x, filters, bias, stride, padding, dilation, activation);
    Operand cx(x);
    if (!cx.arr) return nullptr;
    Operand cf(filters);
    if (!cf.arr) return nullptr;
    if (!bias) return NPH_Conv2D_LayerForward(cx.arr, cf.arr, nullptr, stride, padding, dilation, activation);
    Operand cb(bias);
    return cb.arr ? NPH_Conv2D_LayerForward(cx.arr, cf.arr, cb.arr, stride, padding, dilation, activation) : nullptr;
}

// out: the forward result (may be nullptr without an activation); dy: its gradient.  A malloc'd vector of three: dW, dX and db
// (nullptr without use_bias).
NDArray **NDArrayDNN_Conv2D_LayerBackward(NDArray *input, NDArray *out, NDArray *dy, NDArray *filters, const int *stride, const int *padding,
                                          const int *dilation, char activation, int use_bias) {
    if (!input || !dy || !filters) return nullptr;
    if (!on_gpu(input) || !on_gpu(dy) || !on_gpu(filters) || (out && !on_gpu(out)))
        return NPH_Conv2D_LayerBackward(input, out, dy, filters, stride, padding, dilation, activation, use_bias);
    Operand cx(input);
    if (!cx.arr) return nullptr;
    Operand cy(dy);
    if (!cy.arr) return nullptr;
    Operand cf(filters);
    if (!cf.arr) return nullptr;
    if (!out) return NPH_Conv2D_LayerBackward(cx.arr, nullptr, cy.arr, cf.arr, stride, padding, dilation, activation, use_bias);
    Operand co(out);
    return co.arr ? NPH_Conv2D_LayerBackward(cx.arr, co.arr, cy.arr, cf.arr, stride, padding, dilation, activation, use_bias) : nullptr;
}

}  // extern "C"
