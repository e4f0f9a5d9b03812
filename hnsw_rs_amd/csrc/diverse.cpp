// diverse.cpp -- diversified search (include/hnsw_mi355x.h, "diversified search"): the re-ranking of candidate lists by
// maximal marginal relevance on the device, and a search answered as hits that are near the query and not near each
// other.  Host logic only; the selection is hx_distance_kernel's second source form (exact_scan.hip), the candidate
// stage around it lists_host.h.

#include "lists_host.h"

using hx::set_error;

static_assert(HX_DIVERSE_POOL_MAX == HNSW_DIVERSE_POOL_MAX, "the kernel's LDS holds the ABI's pool limit");

namespace {

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
    if (int rc = hx::need_handle("diversify", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_diverse_shape("diversify", pool, n_out, lambda)) return rc;
    if (int rc = hx::check_nq("diversify", nq)) return rc;
    if (!d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("diversify: needs the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("diversify", "candidates'", d_stats_in, d_stats)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    return select(h, nq, pool, n_out, lambda, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists, d_gaps, d_counts,
                  d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_diverse(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef, float lambda,
                              hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo, const uint32_t *hi,
                              uint32_t *ids, float *dists, float *gaps, uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    const hx::CandidateFilter f{set, mask_of, lo, hi};
    if ((rc = hx::check_candidate_filter("diverse search", h, f))) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_diverse_shape("diverse search", pool, n, lambda))) return rc;
    const bool host_form = f.filtered() || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("diverse search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || nq > 0x7FFFFFFFull) {
        set_error("diverse search: needs queries, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, nq, pool, ef, f, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [queries | re-run selection | candidate block (nq, pool) | diverse block]; pinned arena: [the
    // candidates' stats | diverse block]
    const hx::ResultBlock cand(nq, pool);
    hx::ColumnBlock out;  // [ids | dists | gaps | counts | stats]
    const size_t c_ids = out.add(nq * n * 4), c_dists = out.add(nq * n * 4), c_gaps = out.add(nq * n * 4);
    const size_t c_counts = out.add(nq * 4), c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_resel = o_q + hx::align256(nq * v.dim * 4), o_cand = o_resel + hx::align256(nq * 4);
    const size_t o_out = o_cand + cand.bytes, p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    if (host_form) {
        rc = hx::upload(lists, c, sc.stream, true);
    } else {
        float *d_Q = hx::at<float>(dv, o_q);
        if ((rc = hx::queries_up(h, d_Q, Q, nq, sc.stream))) return rc;
        rc = hx::device_candidates(v, d_Q, nq, pool, ef, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    }
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = select(h, nq, pool, n, lambda, c.ids, c.dists, c.counts, c.stats, hx::at<uint32_t>(d_out, c_ids),
                hx::at<float>(d_out, c_dists), hx::at<float>(d_out, c_gaps), hx::at<uint32_t>(d_out, c_counts),
                hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_diverse_calls, {ids, dists, gaps, counts, stats}, nq);
}

}  // extern "C"
