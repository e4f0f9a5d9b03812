// search_host.h -- the host side of the search entry points (search_host.cpp): the host-pointer path, the
// filtered / deleted orchestration and the completion of a device-pointer call (internal)
#pragma once

#include <cstring>

#include "handle.h"
#include "mask_set.h"
#include "search_filtered.h"

namespace hx {

// The result block of nq queries x n results: [ids | dists | counts | stats], the same layout in the device arena
// and in pinned memory, so it comes back in ONE copy.
struct ResultBlock {
    uint64_t nq = 0;
    uint32_t n = 0;
    size_t ids = 0, dists = 0, counts = 0, stats = 0, bytes = 0;  // offsets from the block's base
    ResultBlock() = default;
    ResultBlock(uint64_t nq_, uint32_t n_) : nq(nq_), n(n_) {
        dists = ids + align256(nq * n * 4);
        counts = dists + align256(nq * n * 4);
        stats = counts + align256(nq * 4);
        bytes = stats + align256(nq * sizeof(hnsw_query_stats));
    }
    struct Ptrs {
        uint32_t *ids;
        float *dists;
        uint32_t *counts;
        hnsw_query_stats *stats;
    };
    Ptrs at(void *base) const {
        unsigned char *b = static_cast<unsigned char *>(base);
        return {reinterpret_cast<uint32_t *>(b + ids), reinterpret_cast<float *>(b + dists),
                reinterpret_cast<uint32_t *>(b + counts), reinterpret_cast<hnsw_query_stats *>(b + stats)};
    }
    template <class Args>  // SearchArgs / FilterArgs: the kernel writes the block at `base`
    void bind(Args &a, void *base) const {
        const Ptrs p = at(base);
        a.out_ids = p.ids;
        a.out_dists = p.dists;
        a.out_counts = p.counts;
        a.out_stats = p.stats;
    }
    // a block in host memory to the caller's buffers (all but o_ids optional)
    void copy_out(void *base, uint32_t *o_ids, float *o_dists, uint32_t *o_counts, hnsw_query_stats *o_stats) const {
        const Ptrs p = at(base);
        memcpy(o_ids, p.ids, nq * n * 4);
        if (o_dists) memcpy(o_dists, p.dists, nq * n * 4);
        if (o_counts) memcpy(o_counts, p.counts, nq * 4);
        if (o_stats) memcpy(o_stats, p.stats, nq * sizeof(hnsw_query_stats));
    }
};

// One search of nq queries in a scratch.  Pinned arena: [queries | result block]; device arena:
// [queries | selection | entries | result block].  The queries reach the device by a true asynchronous copy out of
// pinned memory (a hipMemcpyAsync out of pageable user memory is staged by the runtime and does not overlap anything).
struct HostSearchPlan {
    size_t o_q, o_sel, o_ent, o_out, dev_bytes;  // device arena
    ResultBlock out;
    size_t p_q, p_out, pin_bytes;  // pinned arena
};
HostSearchPlan plan_host_search(uint64_t nq, uint32_t d, uint32_t n, uint32_t n_entry);

// the arguments of hnsw_search* (template.rs:322-326: layers L-1..1 with ef = 1, then layer 0 with ef)
SearchArgs ann_args(const DevView &v, const float *dQ, uint32_t n, uint32_t ef, uint32_t *ids, float *dists,
                    uint32_t *counts, hnsw_query_stats *stats);

// text of a per-query failure on the calling thread; returns the status
int query_status_error(uint64_t i, int32_t status);

// The search itself: the queries are in s.pin + p.p_q (or, for a large call, still in the caller's memory: Q_user),
// the results are left in s.pin + p.p_out.  Queries whose visited table filled up are run again with a table twice
// the size.  Returns launch-level errors only; per-query statuses stay in the result block.
int search_staged(hnsw_index *h, SearchScratch &s, const HostSearchPlan &p, SearchArgs a_host, uint64_t nq,
                  const uint32_t *entries, const float *Q_user);

// host-pointer search (hnsw_search_batch, hnsw_search_layer): user buffers in, user buffers out
int search_host(hnsw_index *h, SearchArgs a_host, const float *Q, uint64_t nq, uint32_t *ids, float *dists,
                uint32_t *counts, hnsw_query_stats *stats, const uint32_t *entries);

// The allow-lists of a filtered call.  One mask for every query (mask_of == nullptr; masks == nullptr: every id below
// allow_bits), or n_masks rows of ceil(allow_bits / 64) words and a row (or HNSW_MASK_NONE) per query.  The rows are
// the caller's and go up with the call, or they are a resident set's (masks, allow_bits and n_masks are then the
// set's host words, mask_of is required): nothing is uploaded, the kernels read the set's HBM copy, and the admissible
// ids of a row come from the set's caches.  Or the call has no masks but a closed range [lo[i], hi[i]] per query over
// the handle's label column (hnsw_search_batch_filtered_range; allow_bits is the index length): the planner's unit is
// then a distinct (lo, hi) pair, counted with the column's sorted copy.  Or it has a resident set AND a range per query
// (hnsw_search_batch_filtered_set_range): query i is under the ids of row mask_of[i] whose label lies in [lo[i], hi[i]],
// the planner's unit is a distinct (row, lo, hi) triple, counted by walking the cheaper of the range's slice of the
// sorted copy and the row's set bits, and the set's per-row caches serve only the triples whose range is [0, UINT32_MAX].
// Or it has a LIST of n_ranges ranges per query (hnsw_search_batch_filtered_ranges; row-major, a member with lo > hi is
// empty): the planner's unit is a distinct canonical list -- empties dropped, sorted, overlapping and adjacent members
// merged -- counted exactly as the sum of its disjoint members' slices of the sorted copy.
struct MaskSpec {
    const uint64_t *masks = nullptr;
    uint64_t allow_bits = 0;
    uint32_t n_masks = 1;
    const uint32_t *mask_of = nullptr;  // nq entries
    hnsw_mask_set *set = nullptr;
    const uint32_t *lo = nullptr, *hi = nullptr;  // nq entries each (nq x n_ranges with a list per query)
    uint32_t n_ranges = 0;  // K > 0: query i is under the union of [lo[i K + j], hi[i K + j]], j < K (no masks, no set)
};

// The admissible ids of a mask: below bits = min(allow_bits, len), allowed by `allow` (nullptr: all), not deleted.
// -> A, and the admissible ids before every block of 64 words (the compaction kernel's offsets)
uint64_t count_admissible(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase);

// k-NN among the admissible ids (hnsw_search_batch_filtered's, _multi's, _set's, _range's and _set_range's contract): the
// planner runs per group -- the queries under one mask, row, range or (row, range) -- the graph path's queries of all groups share one launch and
// one re-run loop, the exact path runs group by group; queries that fill the largest visited table are answered by the
// exact path as well, each under its own filter (path 2).
// exact_only: every query by the exact path (hnsw_brute_force).  The results go to the caller's buffers (per-query
// statuses in stats: required), or, when pin_block is given, straight into that pinned ResultBlock(nq, n) and the
// buffers are not read.  Returns argument and launch errors only.
int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const MaskSpec &m,
                    bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                    uint8_t *paths, const PathCounters *ctr, void *pin_block = nullptr);
// ... with the first per-query error as the status (stats may be NULL)
int search_filtered_checked(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const MaskSpec &m,
                            bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                            uint8_t *paths, const PathCounters *ctr);

// The filter of a device-pointer call, read on the device: a row of a resident set per query (d_mask_of; nullptr: row 0),
// or a label range per query (d_lo / d_hi), or both (hnsw_search_batch_filtered_set_range_device), or neither: the
// undeleted ids, while ids are deleted.
struct DeviceFilter {
    hnsw_mask_set *set = nullptr;
    const uint32_t *d_mask_of = nullptr, *d_lo = nullptr, *d_hi = nullptr;
    uint32_t n_ranges = 0;  // K > 0: d_lo / d_hi hold nq x K members (hnsw_search_batch_filtered_ranges_device)
};

// hnsw_search_batch_device while ids are deleted, hnsw_search_batch_filtered_device, _filtered_range_device and
// _filtered_set_range_device (finish = false), and their _finish: every query by the filtered graph path under its own filter.  The deleted set and
// the set or the label column are brought up to date on a stream of the handle's own, then ONE launch goes to the
// caller's stream.  _finish waits, reads the statuses back (and with them, once, d_mask_of and d_lo / d_hi), re-runs the
// queries whose visited table filled up with larger tables, up to the graph path's largest, answers those that fill it
// by the exact path, each under its own row and range (search_filtered's path 2), and returns the first per-query error:
// a row the set does not have is HNSW_ERR_ARG.  Equals search_filtered under the same filter with filter_exact_max = -1.
int search_device_filtered(hnsw_index *h, const DeviceFilter &f, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                           uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                           hipStream_t stream, bool finish, uint8_t *paths);

// hnsw_search_batch_device_finish while nothing is deleted: waits for the stream, reads the per-query statuses,
// re-runs the queries whose visited table filled up with a table twice the size (same arithmetic, same result as
// if the larger table had been used from the start) and reports the first remaining per-query error.
int search_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                         float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream);

}  // namespace hx
