// What more than one of the dense factorizations (np_lu.hip, np_cholesky.hip, np_jacobi.hip) needs.  Internal: not installed.
#ifndef NUMPOWER_AMD_NP_LINALG_COMMON_H
#define NUMPOWER_AMD_NP_LINALG_COMMON_H

#include "np_internal.h"

namespace np {
namespace linalg {

constexpr int kNB = 64;                  // panel width of the blocked LU and Cholesky and of the blocked triangular solves
// dynamic LDS of the one-workgroup paths (lu_small_kernel, svd_small_kernel): what hipFuncSetAttribute is asked for
constexpr int kSmallLdsBytes = 156 * 1024;
constexpr int kSmallLdsFloats = kSmallLdsBytes / 4;
constexpr size_t kMaxBlockedN = 65536;   // largest n of the blocked LU (panel_kernel holds at most 64 rows per thread) and Cholesky

inline unsigned blocks_for(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// one int from the device (an info word, a flag): the host waits for the stream
inline int read_info(const int *dev_info, int *info_host) {
    int v = 0;
    const int rc = np_memcpy_d2h(&v, dev_info, sizeof(int));
    if (rc != NP_OK) return rc;
    *info_host = v;
    return NP_OK;
}

}  // namespace linalg
}  // namespace np

#endif
