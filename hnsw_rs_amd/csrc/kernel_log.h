// Kernel launch log: a test seam (hnsw_kernel_log / hnsw_kernel_log_get, include/hnsw_mi355x.h).  Every launch site
// calls klog() with the kernel pointer it passes to hipLaunchKernelGGL.  Off, that is one relaxed load; on, the
// pointer's count goes up in a process-wide map.  Names are resolved when the log is read.
#pragma once
#include <atomic>
#include <string>

namespace hx {

extern std::atomic<int> g_klog_on;
void klog_record(const void *kern);

inline void klog(const void *kern) {
    if (g_klog_on.load(std::memory_order_relaxed)) klog_record(kern);
}

// a kernel's name as the log and the tests write it: demangled, without namespaces and parameter list, e.g.
// "hx_search_kernel<1, 64, 256, 4, false>" for _ZN2hx16hx_search_kernelILi1ELi64ELi256ELi4ELb0EEEvNS_7DevViewE...
std::string kernel_name_normalise(const char *name);

}  // namespace hx

// hipLaunchKernelGGL with the launch recorded under the kernel it is given (every launch site of the library)
#define HX_LAUNCH(kern, ...)                                    \
    do {                                                        \
        ::hx::klog(reinterpret_cast<const void *>(kern));       \
        hipLaunchKernelGGL(kern, __VA_ARGS__);                  \
    } while (0)
