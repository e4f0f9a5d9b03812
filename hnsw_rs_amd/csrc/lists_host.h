// lists_host.h -- the candidate stage of the search-then-post-process entry points (grouped, radius, diverse,
// from_rows, multi, late, docs, refine, hybrid, partition .cpp): every one of them checks the call, gets candidate lists of rows x pool into
// HBM, runs ONE post-process launch, brings a column block back in one copy and scatters its columns into the caller's
// buffers.  Everything but the launch is here, once (internal; DESIGN.md, "The candidate stage")
#pragma once

#include <atomic>
#include <cassert>
#include <initializer_list>
#include <vector>

#include "handle.h"
#include "search_host.h"

namespace hx {

// ---- the checks of a call ------------------------------------------------------------------------------------------
// a status that stays with its query (in the stats column) and does not end the call
bool per_query_status(int rc);

// The skeleton of a `_device` entry point, in the order its checks fire: need_handle, nq == 0 is HNSW_OK, the feature's
// shape check, check_nq, the required pointers, check_stats_pair, ready_for_lists.  `what` prefixes the text.
int need_handle(const char *what, const hnsw_index *h);
int check_nq(const char *what, uint64_t nq);  // at most 2^31 - 1 queries
// the stats output goes with the input lists' (`whose`: "candidates'", "shards'"), both or neither
int check_stats_pair(const char *what, const char *whose, const void *d_stats_in, const void *d_stats);
// the lists are a search's: the handle has points and a complete build, and its snapshot is in HBM
int ready_for_lists(hnsw_index *h);

// the filter a composite search hands on to its candidate search: a resident mask set, a label range, both or neither
struct CandidateFilter {
    hnsw_mask_set *set = nullptr;
    const uint32_t *mask_of = nullptr, *lo = nullptr, *hi = nullptr;
    bool filtered() const { return set || lo; }
};
int check_candidate_filter(const char *what, const hnsw_index *h, const CandidateFilter &f);

// ---- candidates by the host form -----------------------------------------------------------------------------------
// Under a filter or while ids are deleted the candidates are the HOST entry point's: only it lets the planner choose
// the exact path ("filter_exact_max"), and every composite call is defined by it.
struct HostLists {
    std::vector<uint32_t> ids, counts;
    std::vector<float> dists;
    std::vector<hnsw_query_stats> stats;
};
// hnsw_search_batch (or the one of its _filtered_set_range / _set / _range forms that `f` names) over rows x pool into
// `l`; a per-query status stays in l.stats and is no error here
int host_candidates(hnsw_index *h, const float *Q, uint64_t rows, uint32_t pool, uint32_t ef, const CandidateFilter &f,
                    HostLists &l);
// the lists into a candidate block in HBM, asynchronously: `l` must outlive the stream's next synchronise.  with_dists
// false: the post-process kernel does not read the distances
int upload(const HostLists &l, const ResultBlock::Ptrs &c, hipStream_t stream, bool with_dists);

// ---- candidates on the device --------------------------------------------------------------------------------------
// the caller's queries into our own arena, once, and there to unit length in place under the cosine option: as the
// search kernel and every post-process kernel that reads queries stage them
int queries_up(const hnsw_index *h, float *d_Q, const float *Q, uint64_t rows, hipStream_t stream);
// The unfiltered search of `rows` queries already in HBM as the kernel stages them (d_Q: unit length under the cosine
// option) into the candidate block `c` of rows x n: the launch of hnsw_search_batch_device and the re-run loop of its
// _finish.  ef is the search's own, as the caller defines it; d_qsel, n_launched: only these queries are launched
// (radius's rung; `c.stats` of the others must read HNSW_OK), nullptr: all rows.  d_resel: room for `rows` ids in
// HBM; pin_stats: room for `rows` stats in pinned memory.  Per-query statuses stay in c.stats.
int device_candidates(const DevView &v, const float *d_Q, uint64_t rows, uint32_t n, uint32_t ef, const uint32_t *d_qsel,
                      uint32_t n_launched, const ResultBlock::Ptrs &c, uint32_t *d_resel, hipStream_t stream,
                      void *pin_stats);

// ---- a post-process stage two entry points launch ----------------------------------------------------------------
// late.cpp: THE LATE INTERACTION over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine
// option): the label column brought up to date, ONE launch on `stream`, "late_launches" bumped
int late_interaction_lists(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                           const float *d_Q, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                           const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels, float *d_scores, uint32_t *d_best_ids,
                           uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs, hnsw_query_stats *d_stats,
                           hipStream_t stream);

// ---- the column block a post-process launch writes -----------------------------------------------------------------
// Columns of any length, each aligned to 256 bytes, the same layout in the device arena and in pinned memory, so the
// block comes back in ONE copy.  The stats column is added last.
struct ColumnBlock {
    static constexpr uint32_t MAX_COLS = 8;
    size_t off[MAX_COLS] = {}, len[MAX_COLS] = {}, bytes = 0;
    uint32_t n_cols = 0;
    size_t add(size_t col_bytes) {  // -> the column's offset from the block's base
        assert(n_cols < MAX_COLS);
        const size_t o = bytes;
        off[n_cols] = o, len[n_cols] = col_bytes, n_cols++;
        bytes += align256(col_bytes);
        return o;
    }
};
template <class T>
T *at(void *base, size_t off) {
    return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off);
}
// The end of a call: the block at d_base back to p_base in one copy, the stream synchronised, `calls` bumped (a call
// counts once its results are on the host), every column copied to its buffer in `dst` (column order; nullptr: the
// caller does not want it), and the first per-query failure of the stats column as the status.
int bring_back(const ColumnBlock &b, const void *d_base, void *p_base, hipStream_t stream, std::atomic<uint64_t> &calls,
               std::initializer_list<void *> dst, uint64_t nq);

}  // namespace hx
