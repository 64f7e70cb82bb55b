// An operand made contiguous for the duration of one call (numpower_host_contiguous): what the host entry points that hand
// their work to the ext/ glue (numpower_linalg.cpp, numpower_signal.cpp) wrap their arguments in.
#ifndef NUMPOWER_AMD_HOST_OPERAND_H
#define NUMPOWER_AMD_HOST_OPERAND_H

#include "numpower_host.h"

namespace numpower_host {

struct Operand {
    NDArray *arr = nullptr;
    NDArray *owned = nullptr;
    explicit Operand(NDArray *a) { arr = numpower_host_contiguous(a, &owned); }
    ~Operand() {
        if (owned) NDArray_FREE(owned);
    }
    Operand(const Operand &) = delete;
    Operand &operator=(const Operand &) = delete;
};

}  // namespace numpower_host
#endif
