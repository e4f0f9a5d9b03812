// boost.cpp -- boosted search (include/hnsw_mi355x.h, "boosted search"): a candidate list re-ranked by a weighted sum of
// its distances and of per-id attributes kept in a row table in HBM, on the device, and a search answered from the index
// and then ranked that way.  Host logic only; the boost is hx_distance_kernel's ninth source form (exact_scan.hip), the
// table row_table.h, the candidate stage around it lists_host.h.

#include <algorithm>

#include "lists_host.h"
#include "row_table.h"

using hx::set_error;

static_assert(HX_BOOST_POOL_MAX == HNSW_BOOST_POOL_MAX, "the kernel's LDS holds the ABI's pool limit");
static_assert(HX_BOOST_MAX_ATTRS == HNSW_BOOST_MAX_ATTRS, "the kernel's weight row holds the ABI's attribute limit");

namespace {

std::atomic<uint64_t> g_device_launches{0};  // hnsw_boost_device's, which has no handle to count them in

// the limits of the boost (`what`: the entry point, `n`: its name for the output length, `a`: for the attributes)
int check_boost_shape(const char *what, const char *n, const char *a, uint32_t pool, uint32_t n_out, uint32_t n_attrs,
                      uint32_t dtype) {
    if (n_out == 0 || n_out > pool || pool > HNSW_BOOST_POOL_MAX) {
        set_error("%s: needs 1 <= %s <= pool <= %d", what, n, HNSW_BOOST_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    if (n_attrs == 0 || n_attrs > HNSW_BOOST_MAX_ATTRS) {
        set_error("%s: needs 1 <= %s <= %d", what, a, HNSW_BOOST_MAX_ATTRS);
        return HNSW_ERR_ARG;
    }
    if (dtype != HNSW_ROWS_F32 && dtype != HNSW_ROWS_F16) {
        set_error("%s: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

int check_weights_rows(const char *what, uint64_t weights_rows, uint64_t nq) {
    if (weights_rows == 1 || weights_rows == nq) return HNSW_OK;
    set_error("%s: weights_rows is 1 (one row for every query) or nq", what);
    return HNSW_ERR_ARG;
}

// the boost over nq lists already in HBM: the one launch
int boost(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t n_attrs, uint32_t dtype, const void *d_table,
          uint64_t table_rows, const float *d_weights, uint64_t weights_rows, const uint32_t *d_ids_in, const float *d_dists_in,
          const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_scores, float *d_dists,
          uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::DiverseLists d{};
    d.ids = d_ids_in;
    d.dists = d_dists_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = pool;
    d.n_out = n_out;
    d.nq = (uint32_t)nq;
    d.out_ids = d_ids;
    d.out_dists = d_scores;
    d.out_gaps = d_dists;
    d.out_counts = d_counts;
    d.out_stats = d_stats;
    d.weights = d_weights;
    d.mode = weights_rows == 1 ? 0u : 1u;
    d.table = d_table;
    d.table_rows = table_rows;
    d.full_dim = n_attrs;
    d.table_dtype = dtype;
    return hx::launch_boost(d, stream);
}

}  // namespace

namespace hx {
uint64_t boost_device_launches() { return g_device_launches.load(std::memory_order_relaxed); }
}  // namespace hx

extern "C" {

int hnsw_boost_device(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t n_attrs, uint32_t dtype, const void *d_table,
                      uint64_t table_rows, const float *d_weights, uint64_t weights_rows, const uint32_t *d_ids_in,
                      const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_ids,
                      float *d_scores, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream) {
    if (nq == 0) return HNSW_OK;
    if (int rc = check_boost_shape("boost", "n_out", "n_attrs", pool, n_out, n_attrs, dtype)) return rc;
    if (int rc = hx::check_nq("boost", nq)) return rc;
    if (int rc = check_weights_rows("boost", weights_rows, nq)) return rc;
    if (!d_table || !d_weights || !d_ids_in || !d_dists_in || !d_ids || !d_scores) {
        set_error("boost: needs the table, the weights, the candidates' ids and distances and the id and score outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("boost", "candidates'", d_stats_in, d_stats)) return rc;
    const int rc = boost(nq, pool, n_out, n_attrs, dtype, d_table, table_rows, d_weights, weights_rows, d_ids_in, d_dists_in,
                         d_counts_in, d_stats_in, d_ids, d_scores, d_dists, d_counts, d_stats, static_cast<hipStream_t>(stream));
    if (rc == HNSW_OK) g_device_launches.fetch_add(1, std::memory_order_relaxed);
    return rc;
}

int hnsw_search_batch_boosted(hnsw_index *h, hnsw_row_table *t, const float *Q, uint64_t nq, uint32_t n, uint32_t pool,
                              uint32_t ef, const float *weights, uint64_t weights_rows, hnsw_mask_set *set,
                              const uint32_t *mask_of, const uint32_t *lo, const uint32_t *hi, uint32_t *ids, float *scores,
                              float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    const hx::CandidateFilter f{set, mask_of, lo, hi};
    if ((rc = hx::check_candidate_filter("boosted search", h, f))) return rc;
    if (nq == 0) return HNSW_OK;
    if (!t) {
        set_error("boosted search: needs a row table");
        return HNSW_ERR_ARG;
    }
    if (t->owner != h) {
        set_error("boosted search: the row table belongs to another handle");
        return HNSW_ERR_ARG;
    }
    const uint32_t n_attrs = t->full_dim;
    if ((rc = check_boost_shape("boosted search", "n", "the table's full_dim", pool, n, n_attrs, t->dtype))) return rc;
    const bool host_form = f.filtered() || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("boosted search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !weights || !ids || nq > 0x7FFFFFFFull) {
        set_error("boosted search: needs the queries, the weights, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if ((rc = check_weights_rows("boosted search", weights_rows, nq))) return rc;
    const uint64_t table_rows = t->rows, len = hx::index_len(h);
    if (table_rows < len) {
        set_error("boosted search: the row table has %llu rows, the index %llu", (unsigned long long)table_rows,
                  (unsigned long long)len);
        return HNSW_ERR_ARG;
    }
    const uint32_t efp = std::max(std::max(ef, pool), 1u);
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, nq, pool, efp, f, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    if (t->device != h->dev.device) {
        set_error("boosted search: the row table sits on device %d, the snapshot on device %d", t->device, h->dev.device);
        return HNSW_ERR_ARG;
    }
    // device arena: [queries | weights | re-run selection | candidate block (nq, pool) | boosted block]; pinned arena: [the
    // candidates' stats | boosted block]
    const hx::ResultBlock cand(nq, pool);
    hx::ColumnBlock out;  // [ids | scores | dists | counts | stats]
    const size_t c_ids = out.add(nq * n * 4), c_scores = out.add(nq * n * 4), c_dists = out.add(nq * n * 4);
    const size_t c_counts = out.add(nq * 4), c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t w_bytes = (size_t)weights_rows * (1 + n_attrs) * 4;
    const size_t o_q = 0, o_w = o_q + hx::align256(nq * v.dim * 4), o_resel = o_w + hx::align256(w_bytes);
    const size_t o_cand = o_resel + hx::align256(nq * 4), o_out = o_cand + cand.bytes;
    const size_t p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q), *d_w = hx::at<float>(dv, o_w);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    HIP_TRY(hipMemcpyAsync(d_w, weights, w_bytes, hipMemcpyHostToDevice, sc.stream));
    if (host_form) {
        rc = hx::upload(lists, c, sc.stream, true);  // (the distances ARE an input of the boost)
    } else {
        if ((rc = hx::queries_up(h, d_Q, Q, nq, sc.stream))) return rc;
        rc = hx::device_candidates(v, d_Q, nq, pool, efp, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    }
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = boost(nq, pool, n, n_attrs, t->dtype, t->d_rows, table_rows, d_w, weights_rows, c.ids, c.dists, c.counts, c.stats,
               hx::at<uint32_t>(d_out, c_ids), hx::at<float>(d_out, c_scores), hx::at<float>(d_out, c_dists),
               hx::at<uint32_t>(d_out, c_counts), hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    h->n_boost_launches.fetch_add(1, std::memory_order_relaxed);
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_boost_calls, {ids, scores, dists, counts, stats}, nq);
}

}  // extern "C"
