// launch.h -- what the launchers in the .hip files share, and nothing else:
//   launch_checked    the one launch sequence: LDS refusal, LDS opt-in, HX_LAUNCH, hipGetLastError -> set_error
//   query_lds_bytes   the one statement of the staged query's size in LDS (kernel carve and launcher must agree)
//   VisitedSpill      the HBM level of the two-level visited set, attached for the length of a launcher
//   cu_count          compute units of the current device
// Host code apart from query_lds_bytes; include from .hip files.
#pragma once

#include <cstdlib>

#include "device_index.h"
#include "switches.h"

namespace hx {

// Bytes the staged query takes in LDS (stage_query / stage_row, search_common.h): QUANT8 keeps both half-row element
// orders dequantised, F32 the raw values; rounded up to 16 so that what follows stays 16-byte aligned.  Kernels whose
// kind is a template parameter write the same expression with KIND for v.kind (the function would cost them a select).
__host__ __device__ inline uint32_t query_lds_bytes(const DevView &v) {
    return ((v.kind == HNSW_VEC_QUANT8 ? 2u * (v.half_bytes - 8) * 4u : v.dim * 4u) + 15u) & ~15u;
}

// What a launch site says when it fails.
struct LaunchSite {
    const char *launch;            // "<launch>: <HIP's error string>" when the launch fails (null: no text, as the site had none)
    const char *refuse = nullptr;  // printf format with one %zu, the message when the kernel would need more than 160 KiB
                                   // of LDS.  Null: the site asks for a fixed or query-sized amount and has no LDS policy
                                   // of its own -- it launches as it is, without the check and without the opt-in
    size_t refuse_value = 0;       // what the %zu prints, if not the LDS bytes
};

// The launch sequence of every kernel of the library.  More than 160 KiB of dynamic LDS (a CU's whole LDS) is refused
// with HNSW_ERR_ARG before anything is launched; more than 48 KiB is opted into on every such launch; the launch goes
// through HX_LAUNCH (kernel log); a launch error becomes the site's text + HNSW_ERR_HIP.
template <class... P, class... A>
int launch_checked(const LaunchSite &site, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                   const A &...args) {
    if (site.refuse != nullptr) {
        if (lds > 160 * 1024) {
            set_error(site.refuse, site.refuse_value ? site.refuse_value : lds);
            return HNSW_ERR_ARG;
        }
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                set_error("hipFuncSetAttribute(%zu): %s", lds, hipGetErrorString(e));
                return HNSW_ERR_HIP;
            }
        }
    }
    HX_LAUNCH(kern, grid, block, lds, stream, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (site.launch != nullptr) set_error("%s: %s", site.launch, hipGetErrorString(e));
        return HNSW_ERR_HIP;
    }
    return HNSW_OK;
}

// The HBM level of the two-level visited set (hx_search_kernel, Visited::look2 of search_lean.hip): the LDS table stays
// at 32 KiB -- four waves per CU -- and 1 << spill_log2 words of stream-ordered scratch per launched query take the ids
// beyond it.  `wanted` is the caller's own threshold (list width, table size); HNSW_MI355X_VISITED_2L=0 turns the
// second level off, HNSW_MI355X_VISITED_2L_LIMIT closes the LDS level early (tests).  Without the scratch nothing is
// attached and the one-level table serves.  The scratch is freed, stream-ordered, when the launcher returns.
struct VisitedSpill {
    void *p = nullptr;
    hipStream_t st = nullptr;
    template <class Args>
    VisitedSpill(bool wanted, Args &a, uint32_t &slots_log2, uint32_t nblocks, hipStream_t stream) : st(stream) {
        if (!wanted || !sw::visited_2l()) return;
        const uint32_t glog2 = slots_log2 + 1 > 15u ? slots_log2 + 1 : 15u;
        if (hipMallocAsync(&p, ((size_t)nblocks << glog2) * 4, stream) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return;
        }
        a.spill_tab = static_cast<uint32_t *>(p);
        a.spill_log2 = glog2;
        slots_log2 = 13;
        a.lds_limit = sw::visited_2l_limit(a.lds_limit);
    }
    ~VisitedSpill() {
        if (p) (void)hipFreeAsync(p, st);
    }
    VisitedSpill(const VisitedSpill &) = delete;
    VisitedSpill &operator=(const VisitedSpill &) = delete;
};

// compute units of the current device, asked once; 256 if the runtime does not say
inline uint32_t cu_count() {
    static const uint32_t n_cu = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return (uint32_t)cus;
    }();
    return n_cu;
}

}  // namespace hx
