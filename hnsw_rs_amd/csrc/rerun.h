// rerun.h -- the re-run loop every search path ends in (search_host.cpp, filter_host.cpp, lists_host.cpp), and the
// first per-query failure of a call (internal)
#pragma once

#include <type_traits>
#include <vector>

#include "search_host.h"

namespace hx {

// A query whose visited table filled up ends with status HNSW_ERR_OVERFLOW and is run again with a table twice the
// size, until none is left or the largest table is reached.  The first launch is the caller's (perhaps in an earlier
// call); what differs from site to site comes in as
//   launch, a:   launch_search or launch_filtered_graph and its arguments (a.qsel is set to the selection);
//   fetch(st):   bring the statuses (or the whole result block) of everything launched so far back to the host,
//                synchronise, and say where they are;
//   exhausted(sel):  answer the queries that filled the largest table some other way and fetch again -- or nullptr:
//                their status stays HNSW_ERR_OVERFLOW for the caller to report.
// d_sel holds the selection on the device (room for nq ids).  n_exhausted = queries handed to `exhausted`.
template <class Args, class Fetch, class Exhausted>
int rerun_overflowed(const DevView &v, int (*launch)(const DevView &, const Args &, uint32_t, uint32_t, hipStream_t), Args &a,
                     uint64_t nq, uint32_t slots, uint32_t max_slots, uint32_t *d_sel, hipStream_t stream, Fetch fetch,
                     Exhausted exhausted, uint64_t *n_exhausted = nullptr) {
    std::vector<uint32_t> sel;
    while (true) {
        const hnsw_query_stats *st = nullptr;
        int rc = fetch(st);
        if (rc != HNSW_OK) return rc;
        sel.clear();
        for (uint64_t i = 0; i < nq; i++)
            if (st[i].status == HNSW_ERR_OVERFLOW) sel.push_back((uint32_t)i);
        if (sel.empty()) return HNSW_OK;
        if (slots >= max_slots) {
            if constexpr (std::is_same_v<Exhausted, std::nullptr_t>) {
                return HNSW_OK;
            } else {
                if (n_exhausted) *n_exhausted = sel.size();
                return exhausted(sel);
            }
        }
        HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // `sel` is reused by the next round
        a.qsel = d_sel;
        if ((rc = launch(v, a, (uint32_t)sel.size(), ++slots, stream))) return rc;
    }
}

// first per-query failure of a call, with its text
inline int first_query_error(const hnsw_query_stats *st, uint64_t nq) {
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // namespace hx
