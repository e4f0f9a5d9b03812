// search_filtered_wide.h -- wide filtered k-NN (hnsw_search_batch_filtered_wide): up to 1024 results and ef' up to 1024
// under any filter a FilterArgs block describes (search_filtered.h) and while ids are deleted.  The kernels of
// search_filtered_wide.hip and their launchers; the host driver is filter_wide_host.cpp.  gfx950 only.
//
// The kernels of search_filtered.hip keep F and R in at most four registers per lane and write results from register 0;
// these keep both lists as sorted arrays in LDS, the visited set in two levels (an LDS table, then an open-addressed
// table per launched query in HBM), and stream the results out of LDS.  The walk, the admission rule and the distance
// routine are those of hx_filt_graph_kernel, so the answers are the ones it would give if it had the room (DESIGN.md
// section 35).
#pragma once

#include "search_filtered.h"

namespace hx {

#define HX_WIDE_MAX_EF 1024       // ef' on the graph path: F and R are 8 KiB of LDS each at most
#define HX_WIDE_MAX_N 1024        // results per query (both paths)
#define HX_WIDE_LDS_LOG2_MIN 10   // option "filter_wide_lds_log2": slots of the LDS level of the visited set
#define HX_WIDE_LDS_LOG2_MAX 15
#define HX_WIDE_HBM_LOG2_MIN 10   // option "filter_wide_hbm_log2": words of the HBM level per launched query (0: none)
#define HX_WIDE_HBM_LOG2_MAX 22
#define HX_WIDE_HBM_LOG2_DEFAULT 18
#define HX_WIDE_HBM_BYTES (1ull << 30)     // the HBM level of one launch stays within this: the queries go in chunks
#define HX_WIDE_PART_BYTES (256ull << 20)  // ... and the exact path's partial lists within this
#define HX_WIDE_SEG 2048          // admissible ids per block of the exact scan: 16 KiB of keys, sorted in LDS

// The visited set of one launch of the graph kernel: 1 << lds_log2 slots in LDS, closed when it holds three quarters of
// them; then 1 << hbm_log2 words at hbm + (block << hbm_log2), closed at three quarters as well (hbm == nullptr: no
// second level).  The HBM level is cleared (HX_EMPTY_SLOT) by the launcher's caller on the stream before the launch.
// Block b serves query q_base + b (through FilterArgs::qsel when that is set).
struct WideVisited {
    uint32_t *hbm;
    uint32_t lds_log2, hbm_log2;
    uint32_t q_base;
};

// ids the two levels hold before a query ends with HNSW_ERR_OVERFLOW
inline uint64_t wide_visited_limit(uint32_t lds_log2, uint32_t hbm_log2) {
    return filt_visited_limit(lds_log2) + (hbm_log2 ? (uint64_t)filt_visited_limit(hbm_log2) : 0);
}
// the LDS level when the option leaves it to the launcher: with a second level the table that keeps four waves on a
// CU next to the lists of ef' keys, without one the largest
inline uint32_t wide_default_lds_log2(uint32_t efp, uint32_t hbm_log2) {
    return hbm_log2 == 0 ? HX_WIDE_LDS_LOG2_MAX : efp <= 256 ? 13u : 12u;
}
// keys of a list's ring in LDS: the power of two at or above ef', 64 at least
inline uint32_t wide_ring_keys(uint32_t efp) {
    uint32_t r = 64;
    while (r < efp) r <<= 1;
    return r;
}

// graph path: `nblocks` queries from vis.q_base on (a.qsel selects them when set), 1 <= a.n <= a.ef <= HX_WIDE_MAX_EF; a
// query that fills both levels of its visited set ends with status HNSW_ERR_OVERFLOW.  No list of several ranges per
// query (a.n_ranges <= 1).
int launch_filtered_wide_graph(const DevView &v, const FilterArgs &a, uint32_t nblocks, const WideVisited &vis,
                               hipStream_t stream);
// exact path: top a.n (<= HX_WIDE_MAX_N) of the `nsel` queries (a.qsel, or the first nsel) over the A listed ids, in
// nseg = wide_exact_segments(A) segments; part holds nsel x nseg x n keys of scratch, part_status nsel x nseg words.
// Writes ids, dists, counts and stats (n_dist = A, n_exp = sum_deg = 0) as launch_filtered_exact does.
inline uint32_t wide_exact_segments(uint64_t A) { return (uint32_t)((A + HX_WIDE_SEG - 1) / HX_WIDE_SEG + (A == 0)); }
int launch_filtered_wide_exact(const DevView &v, const FilterArgs &a, uint32_t nsel, const uint32_t *ids, uint32_t A,
                               unsigned long long *part, int32_t *part_status, hipStream_t stream);

}  // namespace hx
