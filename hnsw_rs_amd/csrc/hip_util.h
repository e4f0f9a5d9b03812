// hip_util.h -- the host files' HIP error check (sets the error text and returns the status from the enclosing
// function) and RAII device buffer.
#pragma once

#include <hip/hip_runtime.h>

#include "host_index.h"

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            hx::set_error("%s failed: %s", #expr, hipGetErrorString(e_));                \
            return e_ == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP;              \
        }                                                                                \
    } while (0)

namespace hx {

struct DevBuf {  // RAII device allocation
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t n) {
        HIP_TRY(hipMalloc(&p, n ? n : 1));
        return HNSW_OK;
    }
    template <class T>
    T *as() {
        return static_cast<T *>(p);
    }
};

}  // namespace hx
