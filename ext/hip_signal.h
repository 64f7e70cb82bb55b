/*
 * hip_signal.h — correlate2d / convolve2d of GPU arrays on the device stencil (np_correlate2d of include/np_hip.h).
 *
 * The reference computes these on the CPU alone: the first statement of its NDArray_Correlate2D (signal.c:218-222) throws
 * "correlate2d not implemented for GPU computation." when either operand is a GPU array.  tools/apply_with_hip.py inserts
 * one early-out in front of that throw, which replaces nothing:
 *
 *     NDArray_Correlate2D at the top, before its GPU throw
 *         if (NPH_SIGNAL_TAKES(a, b)) return NPH_Correlate2D(a, b, mode, boundary, fill_value, flip);
 *
 * guarded by `#ifdef HAVE_NP_HIP`: two CPU operands fall through to the reference's loop, one operand on each device falls
 * through to the reference's throw.
 *
 * The result is what scipy.signal.correlate2d / convolve2d return, which is what the reference's loop (signal.c:152-207)
 * computes.  Its wrapper departs from SciPy in three places and this function does not follow it there:
 * a 'full' result has the full shape (signal.c:275-278 allocates the shape of a), operands change places in 'valid' mode
 * and never in 'same' (signal.c:66 tests the wrong constant), and fill_value is honoured.
 *
 * Plain C over the reference's headers in a PHP build (the result is the reference's own array and dies in its
 * NDArray_FREE), over include/numpower_host.h in libnumpower_host.so, whose NDArray_Correlate2D calls this function after
 * making its operands contiguous.  Operands must be contiguous (the reference's arrays are).
 * Errors: the reference's messages (signal.c:220, 228, 235, 247, 281); NULL after a raised error.
 */
#ifndef NUMPOWER_AMD_EXT_HIP_SIGNAL_H
#define NUMPOWER_AMD_EXT_HIP_SIGNAL_H

#ifdef __cplusplus
extern "C" {
#endif

struct NDArray;

/* true when the early-out takes the call: both operands live on the GPU */
#define NPH_SIGNAL_TAKES(a, b) (NDArray_DEVICE(a) == NDARRAY_DEVICE_GPU && NDArray_DEVICE(b) == NDARRAY_DEVICE_GPU)

/* mode: 0 valid, 1 same, 2 full; boundary: 0 fill, 4 symm, 8 wrap (signal.h); flip != 0: convolution.  fill_value: NULL (0)
 * or an array with one element on either device, read only under boundary 0.  A new GPU array of SciPy's shape.
 * Checked in this order: "NDArray::correlate2d inputs must be both 2-D arrays"; "For 'valid' mode, one input must be at
 * least as large as the other in every dimension"; "fillValue must be a scalar or an array with one element."; "invalid
 * mode."; then the devices: one operand on each "correlate2d not implemented for GPU computation.", both on the CPU the
 * glue's "only computes on the GPU". */
struct NDArray *NPH_Correlate2D(struct NDArray *a, struct NDArray *b, int mode, int boundary, struct NDArray *fill_value, int flip);

#ifdef __cplusplus
}
#endif
#endif
