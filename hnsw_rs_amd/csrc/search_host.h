// search_host.h -- the host side of the search entry points: the host-pointer path and the completion of a
// device-pointer call (search_host.cpp), the filtered / deleted orchestration (filter_host.cpp) (internal)
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

// The filter of a call, stated once: which ROWS of mask words its queries are under, and how many label RANGES each
// query has.  The two facts are independent; the legal combinations are
//
//   rows \ K   | 0                              | 1                                    | 2 .. HNSW_RANGES_MAX
//   ALL        | the undeleted ids below len    | _filtered_range                      | _filtered_ranges
//   ONE        | _filtered (masks: one row)     | refused                              | refused
//   MANY       | _filtered_multi                | refused                              | refused
//   SET        | _filtered_set, _device         | _filtered_set_range, _device         | refused (the kernel's LDS has no room)
//
// rows: ALL -- every undeleted id below the index length; ONE -- `masks` is one row of allow_bits bits for the whole
// call; MANY -- the caller's n_masks rows of ceil(allow_bits / 64) words, and query i is under row mask_of[i] or
// HNSW_MASK_NONE; SET -- the rows are a resident hnsw_mask_set's (nothing is uploaded, the kernels read its HBM copy,
// the admissible ids of a row come from its caches), mask_of as under MANY, or nullptr in a device call: row 0.
// ranges: query i is under the union of [lo[i K + j], hi[i K + j]], j < K, over the handle's label column; a member
// with lo > hi is empty; K == 0: no label filter.  Next to a SET row a query is under the row AND its range.
struct Filter {
    // the entry points that made the call: picks the stat counters and the wording of errors, never a launch
    enum Family { DELETED, SCAN, MASK, MULTI, OF_SET, RANGE, SET_RANGE, RANGES, ONE_QUERY } family = DELETED;
    enum Rows { ALL, ONE, MANY, SET } rows = ALL;
    const uint64_t *masks = nullptr;  // ONE, MANY (host memory)
    uint64_t allow_bits = 0;          // ONE, MANY
    uint32_t n_masks = 0;             // MANY
    hnsw_mask_set *set = nullptr;     // SET
    const uint32_t *mask_of = nullptr;            // MANY, SET: nq entries
    uint32_t K = 0;                               // ranges per query
    const uint32_t *lo = nullptr, *hi = nullptr;  // nq x K entries each, row-major
    bool on_device = false;  // mask_of, lo and hi are device memory (a device-pointer call), else host memory
};

// The admissible ids of a mask: below bits = min(allow_bits, len), allowed by `allow` (nullptr: all), not deleted.
// -> A, and the admissible ids before every block of 64 words (the compaction kernel's offsets)
uint64_t count_admissible(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase);

// k-NN among the admissible ids (the contract of every hnsw_search_batch_filtered*): the planner runs per group -- the
// queries under one (row, canonical range list) -- the graph path's queries of all groups share one launch and one
// re-run loop, the exact path runs group by group; queries that fill the largest visited table are answered by the
// exact path as well, each under its own filter (path 2).
// exact_only: every query by the exact path (hnsw_brute_force).  The results go to the caller's buffers (per-query
// statuses in stats: required), or, when pin_block is given, straight into that pinned ResultBlock(nq, n) and the
// buffers are not read.  Returns argument and launch errors only.
// grouped: a call with two or more exact-path groups runs them in the grouped form, three launches for all of them
// (filter_exact.cpp, exact_grouped), and its path 2 groups in one more such pass; false: as the handle's option
// "filter_exact_grouped" says (0: group by group).  The results do not depend on it.
int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f,
                    bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                    uint8_t *paths, void *pin_block = nullptr, bool grouped = false);
// ... with the first per-query error as the status (stats may be NULL)
int search_filtered_checked(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f,
                            bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                            uint8_t *paths);

// A device-pointer call under a Filter whose mask_of / lo / hi are device memory (on_device): hnsw_search_batch_device
// while ids are deleted and every hnsw_search_batch_filtered*_device (finish = false), and their _finish: every query by
// the filtered graph path under its own filter.  The deleted set and
// the set or the label column are brought up to date on a stream of the handle's own, then ONE launch goes to the
// caller's stream.  _finish waits, reads the statuses back (and with them, once, d_mask_of and d_lo / d_hi), re-runs the
// queries whose visited table filled up with larger tables, up to the graph path's largest, answers those that fill it
// by the exact path, each under its own row and range (search_filtered's path 2), and returns the first per-query error:
// a row the set does not have is HNSW_ERR_ARG.  Equals search_filtered under the same filter with filter_exact_max = -1.
int search_device_filtered(hnsw_index *h, const Filter &f, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                           uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                           hipStream_t stream, bool finish, uint8_t *paths);

// The label column as the kernels read it, for a caller outside the filtered searches (grouped.cpp): the HBM copy is
// brought up to date on a stream of the handle's own, exactly as a range search does it (a column no label was ever
// set in gets its copy of zeros); -> the copy and the labels it holds.  The snapshot's device must be known
// (ensure_uploaded).
int labels_on_device(hnsw_index *h, const uint32_t **d_labels, uint64_t *label_len);
// ... and the deleted set as the kernels read it (FilterArgs::deny, deny_bits), for the rank fusion (hybrid.cpp): brought
// up to date the same way; nullptr and 0 while nothing is deleted
int deleted_on_device(hnsw_index *h, const uint64_t **d_deny, uint64_t *deny_bits);

// hnsw_search_batch_device_finish while nothing is deleted: waits for the stream, reads the per-query statuses,
// re-runs the queries whose visited table filled up with a table twice the size (same arithmetic, same result as
// if the larger table had been used from the start) and reports the first remaining per-query error.
int search_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                         float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream);

// The two ground-truth scans (ground_truth.cpp) behind hnsw_brute_force and hnsw_brute_force_fast, which have checked
// the handle and the arguments: every point in the reference's arithmetic (while ids are deleted, the undeleted ones);
// the screen on the matrix cores with the exact re-rank of its k + 8 survivors (k + 8 <= brute_mfma_k2())
int exact_scan(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists);
int mfma_scan(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists);

}  // namespace hx
