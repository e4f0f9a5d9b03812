// diverse.cpp -- diversified search (include/hnsw_mi355x.h, "diversified search"): the re-ranking of candidate lists by
// maximal marginal relevance on the device, and a search answered as hits that are near the query and not near each
// other.  Host logic only; the selection is hx_distance_kernel's second source form (exact_scan.hip).

#include <cstring>
#include <vector>

#include "handle.h"
#include "search_filtered.h"
#include "search_host.h"

using hx::set_error;

static_assert(HX_DIVERSE_POOL_MAX == HNSW_DIVERSE_POOL_MAX, "the kernel's LDS holds the ABI's pool limit");

namespace {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

// the limits of the selection (`what`: the entry point, for the text)
int check_diverse_shape(const char *what, uint32_t pool, uint32_t n_out, float lambda) {
    if (n_out == 0 || n_out > pool || pool > HNSW_DIVERSE_POOL_MAX) {
        set_error("%s: needs 1 <= n <= pool <= %d", what, HNSW_DIVERSE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    if (!(lambda >= 0.0f && lambda <= 1.0f)) {  // (a NaN fails both compares)
        set_error("%s: lambda must lie in [0, 1]", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// The diverse block of nq queries x n: [ids | dists | gaps | counts | stats], the same layout in the device arena and in
// pinned memory, so it comes back in ONE copy (as ResultBlock, search_host.h).
struct DiverseBlock {
    size_t ids = 0, dists, gaps, counts, stats, bytes;
    DiverseBlock(uint64_t nq, uint32_t n) {
        dists = ids + hx::align256(nq * n * 4);
        gaps = dists + hx::align256(nq * n * 4);
        counts = gaps + hx::align256(nq * n * 4);
        stats = counts + hx::align256(nq * 4);
        bytes = stats + hx::align256(nq * sizeof(hnsw_query_stats));
    }
    template <class T>
    T *at(void *base, size_t off) const {
        return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off);
    }
};

// the selection over nq lists already in HBM: the one launch
int select(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_out, float lambda, const uint32_t *d_ids_in,
           const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_ids,
           float *d_dists, float *d_gaps, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::DiverseLists d{};
    d.ids = d_ids_in;
    d.dists = d_dists_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = pool;
    d.n_out = n_out;
    d.lambda = lambda;
    d.nq = (uint32_t)nq;
    d.out_ids = d_ids;
    d.out_dists = d_dists;
    d.out_gaps = d_gaps;
    d.out_counts = d_counts;
    d.out_stats = d_stats;
    if (int rc = hx::launch_diversify(h->dev.view, d, stream)) return rc;
    h->n_diverse_launches.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

}  // namespace

extern "C" {

int hnsw_diversify_device(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_out, float lambda, const uint32_t *d_ids_in,
                          const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in,
                          uint32_t *d_ids, float *d_dists, float *d_gaps, uint32_t *d_counts, hnsw_query_stats *d_stats,
                          void *stream) {
    if (!h) {
        set_error("diversify: null handle");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if (int rc = check_diverse_shape("diversify", pool, n_out, lambda)) return rc;
    if (nq > 0x7FFFFFFFull) {
        set_error("diversify: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("diversify: needs the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if ((d_stats_in != nullptr) != (d_stats != nullptr)) {
        set_error("diversify: the stats output goes with the candidates' stats, both or neither");
        return HNSW_ERR_ARG;
    }
    int rc = hx::check_search_args(h, 0);  // (the lists are a search's: the handle has points and a complete build)
    if (rc != HNSW_OK || (rc = hx::ensure_uploaded(h))) return rc;
    return select(h, nq, pool, n_out, lambda, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists, d_gaps, d_counts,
                  d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_diverse(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef, float lambda,
                              hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo, const uint32_t *hi,
                              uint32_t *ids, float *dists, float *gaps, uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (set && set->owner != h) {
        set_error("diverse search: the mask set belongs to another handle");
        return HNSW_ERR_ARG;
    }
    if (mask_of && !set) {
        set_error("diverse search: mask_of needs its mask set");
        return HNSW_ERR_ARG;
    }
    if ((lo != nullptr) != (hi != nullptr)) {
        set_error("diverse search: a label range needs lo and hi, both or neither");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if ((rc = check_diverse_shape("diverse search", pool, n, lambda))) return rc;
    const bool filtered = set || lo;
    const bool host_form = filtered || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("diverse search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || nq > 0x7FFFFFFFull) {
        set_error("diverse search: needs queries, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    const uint64_t dim = h->dev.replica ? h->dev.view.dim : h->host->dim;
    // device arena: [queries | candidate ids [nq][pool] | dists | counts | stats | diverse block], the diverse block back
    // in one copy to the pinned arena
    const size_t cand = hx::align256(nq * pool * 4);
    const size_t o_q = 0, o_ids = o_q + hx::align256(nq * dim * 4), o_dists = o_ids + cand, o_counts = o_dists + cand;
    const size_t o_stats = o_counts + hx::align256(nq * 4), o_out = o_stats + hx::align256(nq * sizeof(hnsw_query_stats));
    const DiverseBlock out(nq, n);
    // The candidates.  Under a filter or deletions they are the HOST form's: only it lets the planner choose the exact
    // path ("filter_exact_max"), and the call is defined by it (as grouped.cpp)
    std::vector<uint32_t> h_ids, h_counts;
    std::vector<float> h_dists;
    std::vector<hnsw_query_stats> h_stats;
    if (host_form) {
        h_ids.resize(nq * pool), h_dists.resize(nq * pool), h_counts.resize(nq), h_stats.resize(nq);
        if (set && lo)
            rc = hnsw_search_batch_filtered_set_range(h, Q, nq, pool, ef, set, mask_of, lo, hi, h_ids.data(), h_dists.data(),
                                                      h_counts.data(), h_stats.data(), nullptr);
        else if (set)
            rc = hnsw_search_batch_filtered_set(h, Q, nq, pool, ef, set, mask_of, h_ids.data(), h_dists.data(), h_counts.data(),
                                                h_stats.data(), nullptr);
        else if (lo)
            rc = hnsw_search_batch_filtered_range(h, Q, nq, pool, ef, lo, hi, h_ids.data(), h_dists.data(), h_counts.data(),
                                                  h_stats.data(), nullptr);
        else
            rc = hnsw_search_batch(h, Q, nq, pool, ef, h_ids.data(), h_dists.data(), h_counts.data(), h_stats.data());
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev);
    float *d_Q = reinterpret_cast<float *>(dv + o_q), *d_dists_in = reinterpret_cast<float *>(dv + o_dists);
    uint32_t *d_ids_in = reinterpret_cast<uint32_t *>(dv + o_ids), *d_counts_in = reinterpret_cast<uint32_t *>(dv + o_counts);
    hnsw_query_stats *d_stats_in = reinterpret_cast<hnsw_query_stats *>(dv + o_stats);
    if (host_form) {  // (the host vectors outlive the copies: the stream is synchronised below)
        HIP_TRY(hipMemcpyAsync(d_ids_in, h_ids.data(), nq * pool * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_dists_in, h_dists.data(), nq * pool * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_counts_in, h_counts.data(), nq * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_stats_in, h_stats.data(), nq * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, sc.stream));
    } else {  // as a caller of the device entry point would run it: launch, then _finish
        HIP_TRY(hipMemcpyAsync(d_Q, Q, nq * dim * 4, hipMemcpyHostToDevice, sc.stream));
        rc = hnsw_search_batch_device(h, d_Q, nq, pool, ef, d_ids_in, d_dists_in, d_counts_in, d_stats_in, sc.stream);
        if (rc != HNSW_OK) return rc;
        rc = hnsw_search_batch_device_finish(h, d_Q, nq, pool, ef, d_ids_in, d_dists_in, d_counts_in, d_stats_in, sc.stream);
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    rc = select(h, nq, pool, n, lambda, d_ids_in, d_dists_in, d_counts_in, d_stats_in, out.at<uint32_t>(dv + o_out, out.ids),
                out.at<float>(dv + o_out, out.dists), out.at<float>(dv + o_out, out.gaps),
                out.at<uint32_t>(dv + o_out, out.counts), out.at<hnsw_query_stats>(dv + o_out, out.stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    HIP_TRY(hipMemcpyAsync(sc.pin, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_diverse_calls.fetch_add(1, std::memory_order_relaxed);
    const size_t row = (size_t)nq * n * 4;
    memcpy(ids, out.at<uint32_t>(sc.pin, out.ids), row);
    if (dists) memcpy(dists, out.at<float>(sc.pin, out.dists), row);
    if (gaps) memcpy(gaps, out.at<float>(sc.pin, out.gaps), row);
    if (counts) memcpy(counts, out.at<uint32_t>(sc.pin, out.counts), nq * 4);
    const hnsw_query_stats *st = out.at<hnsw_query_stats>(sc.pin, out.stats);
    if (stats) memcpy(stats, st, nq * sizeof(hnsw_query_stats));
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return hx::query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // extern "C"
