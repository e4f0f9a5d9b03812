// lists_host.cpp -- the candidate stage of the search-then-post-process entry points (lists_host.h).  Host logic only.

#include "lists_host.h"

#include <algorithm>
#include <cstring>

#include "rerun.h"

namespace hx {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

int need_handle(const char *what, const hnsw_index *h) {
    if (h) return HNSW_OK;
    set_error("%s: null handle", what);
    return HNSW_ERR_ARG;
}

int check_nq(const char *what, uint64_t nq) {
    if (nq <= 0x7FFFFFFFull) return HNSW_OK;
    set_error("%s: at most 2^31 - 1 queries", what);
    return HNSW_ERR_ARG;
}

int check_stats_pair(const char *what, const char *whose, const void *d_stats_in, const void *d_stats) {
    if ((d_stats_in != nullptr) == (d_stats != nullptr)) return HNSW_OK;
    set_error("%s: the stats output goes with the %s stats, both or neither", what, whose);
    return HNSW_ERR_ARG;
}

int ready_for_lists(hnsw_index *h) {
    const int rc = check_search_args(h, 0);
    return rc != HNSW_OK ? rc : ensure_uploaded(h);
}

int check_candidate_filter(const char *what, const hnsw_index *h, const CandidateFilter &f) {
    if (f.set && f.set->owner != h) {
        set_error("%s: the mask set belongs to another handle", what);
        return HNSW_ERR_ARG;
    }
    if (f.mask_of && !f.set) {
        set_error("%s: mask_of needs its mask set", what);
        return HNSW_ERR_ARG;
    }
    if ((f.lo != nullptr) != (f.hi != nullptr)) {
        set_error("%s: a label range needs lo and hi, both or neither", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

int host_candidates(hnsw_index *h, const float *Q, uint64_t rows, uint32_t pool, uint32_t ef, const CandidateFilter &f,
                    HostLists &l) {
    l.ids.resize(rows * pool), l.dists.resize(rows * pool), l.counts.resize(rows), l.stats.resize(rows);
    uint32_t *ids = l.ids.data(), *counts = l.counts.data();
    float *dists = l.dists.data();
    hnsw_query_stats *stats = l.stats.data();
    int rc;
    if (f.set && f.lo)
        rc = hnsw_search_batch_filtered_set_range(h, Q, rows, pool, ef, f.set, f.mask_of, f.lo, f.hi, ids, dists, counts, stats,
                                                  nullptr);
    else if (f.set)
        rc = hnsw_search_batch_filtered_set(h, Q, rows, pool, ef, f.set, f.mask_of, ids, dists, counts, stats, nullptr);
    else if (f.lo)
        rc = hnsw_search_batch_filtered_range(h, Q, rows, pool, ef, f.lo, f.hi, ids, dists, counts, stats, nullptr);
    else
        rc = hnsw_search_batch(h, Q, rows, pool, ef, ids, dists, counts, stats);
    return per_query_status(rc) ? HNSW_OK : rc;
}

int upload(const HostLists &l, const ResultBlock::Ptrs &c, hipStream_t stream, bool with_dists) {
    HIP_TRY(hipMemcpyAsync(c.ids, l.ids.data(), l.ids.size() * 4, hipMemcpyHostToDevice, stream));
    if (with_dists) HIP_TRY(hipMemcpyAsync(c.dists, l.dists.data(), l.dists.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c.counts, l.counts.data(), l.counts.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c.stats, l.stats.data(), l.stats.size() * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, stream));
    return HNSW_OK;
}

int queries_up(const hnsw_index *h, float *d_Q, const float *Q, uint64_t rows, hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(d_Q, Q, rows * h->dev.view.dim * 4, hipMemcpyHostToDevice, stream));
    return cosine_queries(h, d_Q, rows, stream);
}

int device_candidates(const DevView &v, const float *d_Q, uint64_t rows, uint32_t n, uint32_t ef, const uint32_t *d_qsel,
                      uint32_t n_launched, const ResultBlock::Ptrs &c, uint32_t *d_resel, hipStream_t stream,
                      void *pin_stats) {
    SearchArgs a = ann_args(v, d_Q, n, ef, c.ids, c.dists, c.counts, c.stats);
    a.qsel = d_qsel;
    // (the table launch_search itself picks when it is asked for none: its ef is at least 1)
    const uint32_t slots = default_slots_log2(std::max(ef, 1u), v.S0);
    if (int rc = launch_search(v, a, d_qsel ? n_launched : (uint32_t)rows, slots, stream)) return rc;
    return rerun_overflowed(
        v, launch_search, a, rows, slots, max_slots_log2(ef), d_resel, stream,
        [&](const hnsw_query_stats *&st) -> int {
            HIP_TRY(hipMemcpyAsync(pin_stats, c.stats, rows * sizeof(hnsw_query_stats), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            st = static_cast<const hnsw_query_stats *>(pin_stats);
            return HNSW_OK;
        },
        nullptr);
}

int bring_back(const ColumnBlock &b, const void *d_base, void *p_base, hipStream_t stream, std::atomic<uint64_t> &calls,
               std::initializer_list<void *> dst, uint64_t nq) {
    assert(dst.size() == b.n_cols);
    HIP_TRY(hipMemcpyAsync(p_base, d_base, b.bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    calls.fetch_add(1, std::memory_order_relaxed);
    uint32_t col = 0;
    for (void *to : dst) {
        if (to) memcpy(to, at<unsigned char>(p_base, b.off[col]), b.len[col]);
        col++;
    }
    return first_query_error(at<const hnsw_query_stats>(p_base, b.off[b.n_cols - 1]), nq);
}

}  // namespace hx
