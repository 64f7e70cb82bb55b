// NDArray_Det / NDArray_Inverse / NDArray_LU / NDArray_Solve (linalg.c:253, 584, 620, 981) on the device LU, and
// NDArray_Cholesky (linalg.c:1056) on the device Cholesky factorization.
// The work — argument checks, the reference's messages, the np_det / np_inverse / np_lu / np_solve / np_cholesky calls — is
// ext/hip_linalg.c, the same code a --with-hip tree reaches through the early-outs tools/apply_with_hip.py inserts into
// the reference's functions; here strided views are first made contiguous (numpower_host_contiguous).
// A translation unit of its own: the sanitizer build of numpower_host.cpp (tests/test_host_sanitizers_cpu.py) links
// against a null device that has no LU.
//
// How each call sees the row-major buffers:
//   det      getrf on the buffer as LAPACK sees it (column-major: a^T, the same determinant)
//   inverse  getrf on the buffer as-is, getrs against I: (a^T)^-1 column-major, which read row-major is a^-1
//   solve    a itself is factored (a transposed copy in column-major), so x solves a x = b for any number of columns
//   lu       the same factorization of a: P a = L U with partial pivoting on the rows of a
//   cholesky row-major as it is: only the lower triangle of a is read
#include <stdlib.h>

#include "hip_linalg.h"
#include "np_ext_hooks.h"
#include "numpower_host.h"

namespace {

// an operand made contiguous for the duration of one call
struct Operand {
    NDArray *arr = nullptr;
    NDArray *owned = nullptr;
    explicit Operand(NDArray *a) { arr = numpower_host_contiguous(a, &owned); }
    ~Operand() {
        if (owned) NDArray_FREE(owned);
    }
};

}  // namespace

extern "C" {

NDArray *NDArray_Det(NDArray *a) {   // linalg.c:253-305
    if (!a) return nullptr;
    Operand ca(a);
    return ca.arr ? NPH_Det(ca.arr) : nullptr;
}

NDArray *NDArray_Inverse(NDArray *target) {   // linalg.c:574-606
    if (!target) return nullptr;
    Operand ca(target);
    return ca.arr ? NPH_Inverse(ca.arr) : nullptr;
}

NDArray **NDArray_LU(NDArray *target) {   // linalg.c:614-650: the vector is malloc'd here (the reference emallocs it)
    if (!target) return nullptr;
    Operand ca(target);
    if (!ca.arr) return nullptr;
    NDArray *p = NDArray_EmptyLike(ca.arr);
    NDArray *l = p ? NDArray_EmptyLike(ca.arr) : nullptr;
    NDArray *u = l ? NDArray_EmptyLike(ca.arr) : nullptr;
    NDArray **rtns = u ? (NDArray **)malloc(sizeof(NDArray *) * 3) : nullptr;
    if (u && !rtns) np_ext_throw("lu: out of host memory");
    if (!rtns || !NPH_LU(ca.arr, p, l, u)) {
        free(rtns);
        if (p) NDArray_FREE(p);
        if (l) NDArray_FREE(l);
        if (u) NDArray_FREE(u);
        return nullptr;
    }
    rtns[0] = p;
    rtns[1] = l;
    rtns[2] = u;
    return rtns;
}

NDArray *NDArray_Solve(NDArray *a, NDArray *b) {   // linalg.c:981-1030
    if (!a || !b) return nullptr;
    Operand ca(a);
    if (!ca.arr) return nullptr;
    Operand cb(b);
    return cb.arr ? NPH_Solve(ca.arr, cb.arr) : nullptr;
}

NDArray *NDArray_Cholesky(NDArray *a) {   // linalg.c:1056-1102
    if (!a) return nullptr;
    Operand ca(a);
    return ca.arr ? NPH_Cholesky(ca.arr) : nullptr;
}

}  // extern "C"
