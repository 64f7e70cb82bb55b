// NDArray_Det / NDArray_Inverse / NDArray_LU / NDArray_Solve (linalg.c:253, 584, 620, 981) on the device LU, and
// NDArray_Cholesky (linalg.c:1056) on the device Cholesky factorization, NDArray_SVD / NDArray_MatrixRank / NDArray_Norm /
// NDArray_Cond (linalg.c:111, 668, 402-470, 1038) on the device Jacobi SVD, NDArray_Eig (linalg.c:795) on the
// device symmetric eigensolver, NDArray_Qr / NDArray_Lstsq (linalg.c:909, 849) on the device Householder QR
// (DESIGN.md §3.13).
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
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hip_linalg.h"
#include "np_ext_hooks.h"
#include "np_hip.h"
#include "numpower_host.h"
#include "numpower_operand.h"

namespace {

using numpower_host::Operand;

// the singular values of a contiguous 2-d GPU array on the host (np_svdvals), descending; false after a raised error
bool singular_values(NDArray *a, const char *who, std::vector<float> &out) {
    char msg[160];
    if (NDArray_NDIM(a) != 2) {
        snprintf(msg, sizeof msg, "%s: the operand must be two-dimensional", who);
        np_ext_throw(msg);
        return false;
    }
    if (NDArray_DEVICE(a) != NDARRAY_DEVICE_GPU) {
        np_ext_throw("linear algebra: operand is on the CPU; numpower_amd only computes on the GPU "
                     "(call ->gpu() first, the CPU path is the reference's own)");
        return false;
    }
    const size_t m = (size_t)NDArray_SHAPE(a)[0], n = (size_t)NDArray_SHAPE(a)[1], k = m < n ? m : n;
    out.assign(k, 0.0f);
    if (k == 0) return true;
    void *s = nullptr;
    int info = 0;
    bool ok = np_malloc(&s, k * sizeof(float)) == NP_OK;
    ok = ok && np_svdvals(NDArray_FDATA(a), m, n, (float *)s, &info) == NP_OK;
    ok = ok && np_memcpy_d2h(out.data(), s, k * sizeof(float)) == NP_OK;
    if (!ok) np_ext_throw_last();
    if (s) np_free(s);
    return ok;
}

NDArray *gpu_scalar(float value) {
    NDArray *h = NDArray_CreateFromFloatScalar(value);
    if (!h) return nullptr;
    NDArray *d = NDArray_ToGPU(h);
    NDArray_FREE(h);
    return d;
}

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

NDArray **NDArray_SVD(NDArray *target) {   // linalg.c:111-209: the vector is malloc'd here (the reference emallocs it)
    if (!target) return nullptr;
    Operand ca(target);
    return ca.arr ? NPH_SVD(ca.arr) : nullptr;
}

NDArray **NDArray_Eig(NDArray *a) {   // linalg.c:795-838: the vector is malloc'd here; symmetric GPU operands only (np_eigh)
    if (!a) return nullptr;
    Operand ca(a);
    return ca.arr ? NPH_Eig(ca.arr) : nullptr;
}

NDArray **NDArray_Qr(NDArray *a) {   // linalg.c:908-970: the vector is malloc'd here; {Q (m, n) reduced, R (n, n)}, m >= n
    if (!a) return nullptr;
    Operand ca(a);
    return ca.arr ? NPH_Qr(ca.arr) : nullptr;
}

NDArray *NDArray_Lstsq(NDArray *a, NDArray *b) {   // linalg.c:848-899, m >= n
    if (!a || !b) return nullptr;
    Operand ca(a);
    if (!ca.arr) return nullptr;
    Operand cb(b);
    return cb.arr ? NPH_Lstsq(ca.arr, cb.arr) : nullptr;
}

NDArray *NDArray_MatrixRank(NDArray *target, float *tol) {   // linalg.c:668-715, on the singular values alone
    if (!target) return nullptr;
    Operand ca(target);
    std::vector<float> s;
    if (!ca.arr || !singular_values(ca.arr, "NDArray_MatrixRank", s)) return nullptr;
    float mtol = 0.0f;
    if (tol) {
        mtol = *tol;
    } else if (!s.empty()) {
        mtol = s[0] * fmaxf((float)NDArray_SHAPE(ca.arr)[0], (float)NDArray_SHAPE(ca.arr)[1]) * FLT_EPSILON;
    }
    long rank = 0;
    for (float v : s) rank += v > mtol ? 1 : 0;
    return NDArray_CreateFromLongScalar(rank);
}

NDArray *NDArray_Norm(NDArray *target, int type) {   // linalg.c:402-470
    if (!target) return nullptr;
    char msg[200];
    if (type == 1) {
        np_ext_throw("NDArray_Norm: the norm `1` is not available for GPU arrays (the reference's NDArray_L1Norm writes past its "
                     "result buffer when an array has more columns than rows)");
        return nullptr;
    }
    if (type != 2) {
        snprintf(msg, sizeof msg, "NDArray_Norm: The provided norm `%d` is invalid", type);
        np_ext_throw(msg);
        return nullptr;
    }
    Operand ca(target);
    std::vector<float> s;
    if (!ca.arr || !singular_values(ca.arr, "NDArray_Norm", s)) return nullptr;
    return gpu_scalar(s.empty() ? 0.0f : s[0]);
}

NDArray *NDArray_Cond(NDArray *a) {   // linalg.c:1038-1050: norm2(a) * norm2(inv(a)); a singular a raises NDArray_Inverse's message
    if (!a) return nullptr;
    Operand ca(a);
    if (!ca.arr) return nullptr;
    NDArray *inv = NPH_Inverse(ca.arr);
    if (!inv) return nullptr;
    std::vector<float> s, si;
    const bool ok = singular_values(ca.arr, "NDArray_Cond", s) && singular_values(inv, "NDArray_Cond", si);
    NDArray_FREE(inv);
    if (!ok) return nullptr;
    return gpu_scalar(s.empty() ? 0.0f : s[0] * si[0]);
}

}  // extern "C"
