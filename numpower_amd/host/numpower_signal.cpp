// NDArray_Correlate2D (signal.c:217-303) on the device stencil (np_correlate2d).
// The work — argument checks, the reference's messages, the result array, the np_correlate2d call — is ext/hip_signal.c, the
// same code a --with-hip tree reaches through the early-out tools/apply_with_hip.py inserts at the top of the reference's
// function; here strided views of either operand are first made contiguous (numpower_host_contiguous).
// A translation unit of its own: the sanitizer build of numpower_host.cpp (tests/test_host_sanitizers_cpu.py) links
// against a null device that has no stencil.
#include "hip_signal.h"
#include "numpower_host.h"
#include "numpower_operand.h"

using numpower_host::Operand;

extern "C" {

NDArray *NDArray_Correlate2D(NDArray *a, NDArray *b, int mode, int boundary, NDArray *fill_value, int flip) {
    if (!a || !b) return nullptr;
    // CPU operands are handed on as they are: they only ever meet the argument checks and the device message
    if (NDArray_DEVICE(a) != NDARRAY_DEVICE_GPU || NDArray_DEVICE(b) != NDARRAY_DEVICE_GPU)
        return NPH_Correlate2D(a, b, mode, boundary, fill_value, flip);
    Operand ca(a);
    if (!ca.arr) return nullptr;
    Operand cb(b);
    return cb.arr ? NPH_Correlate2D(ca.arr, cb.arr, mode, boundary, fill_value, flip) : nullptr;
}

}  // extern "C"
