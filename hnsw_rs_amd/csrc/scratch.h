// scratch.h -- the per-call scratch of the host-pointer search paths (internal)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "hip_util.h"

namespace hx {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One device arena, one pinned host arena and a stream, kept in a pool on the handle (ScratchLease, handle.h) or in
// a coalescer batch (coalesce.h) so that a call costs no allocation, one H2D and one D2H copy.  Concurrent callers
// each take their own scratch (hnsw_search* stays re-entrant).
struct SearchScratch {
    void *dev = nullptr, *pin = nullptr;
    size_t dev_cap = 0, pin_cap = 0;
    hipStream_t stream = nullptr;
    int device = -1;
    SearchScratch() = default;
    SearchScratch(const SearchScratch &) = delete;
    SearchScratch &operator=(const SearchScratch &) = delete;
    ~SearchScratch() { release(); }
    void release() {
        if (dev) (void)hipFree(dev);
        if (pin) (void)hipHostFree(pin);
        if (stream) (void)hipStreamDestroy(stream);
        dev = pin = nullptr;
        stream = nullptr;
        dev_cap = pin_cap = 0;
    }
    // a stream on `on_device` and arenas of at least these sizes (a scratch made for another device starts over);
    // slack: a quarter more than asked for, so that calls of slowly growing sizes do not allocate every time
    int reserve(int on_device, size_t dev_bytes, size_t pin_bytes, bool slack) {
        if (device != on_device) {
            release();
            device = on_device;
        }
        if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (dev_cap < dev_bytes) {
            if (dev) (void)hipFree(dev);
            dev = nullptr;
            dev_cap = 0;
            const size_t cap = slack ? dev_bytes + dev_bytes / 4 + 4096 : dev_bytes;
            HIP_TRY(hipMalloc(&dev, cap));
            dev_cap = cap;
        }
        if (pin_cap < pin_bytes) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr;
            pin_cap = 0;
            const size_t cap = slack ? pin_bytes + pin_bytes / 4 + 4096 : pin_bytes;
            HIP_TRY(hipHostMalloc(&pin, cap, hipHostMallocDefault));
            pin_cap = cap;
        }
        return HNSW_OK;
    }
};

}  // namespace hx
