// late.cpp -- late-interaction search (include/hnsw_mi355x.h, "late-interaction search"): a query's per-vector candidate
// lists scored as documents -- the candidates that share a label -- by summed min distance on the device, and a search
// answered by its nearest documents.  Host logic only; the scoring is hx_distance_kernel's fifth source form
// (exact_scan.hip), the candidate stage around it lists_host.h.

#include <algorithm>

#include "lists_host.h"

using hx::set_error;

static_assert(HX_LATE_MAX_VECS == HNSW_LATE_MAX_VECS, "the kernel's vector limit is the ABI's");
static_assert(HX_LATE_MAX_CANDS == HNSW_LATE_MAX_CANDS, "the kernel's LDS table holds the ABI's candidate limit");
static_assert(HX_LATE_MAX_DOCS == HNSW_LATE_MAX_DOCS, "the kernel's document limit is the ABI's");

namespace {

// the limits of the late interaction (`what`: the entry point, `n`: its name for the output length, for the text)
int check_late_shape(const char *what, const char *n, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode) {
    if (n_vecs == 0 || n_vecs > HNSW_LATE_MAX_VECS) {
        set_error("%s: needs 1 <= n_vecs <= %d", what, HNSW_LATE_MAX_VECS);
        return HNSW_ERR_ARG;
    }
    const uint64_t total = (uint64_t)n_vecs * pool;
    if (n_out == 0 || n_out > total || n_out > HNSW_LATE_MAX_DOCS || total > HNSW_LATE_MAX_CANDS) {
        set_error("%s: needs n_vecs * pool <= %d and 1 <= %s <= min(n_vecs * pool, %d)", what, HNSW_LATE_MAX_CANDS, n,
                  HNSW_LATE_MAX_DOCS);
        return HNSW_ERR_ARG;
    }
    if (mode != HNSW_LATE_SUM && mode != HNSW_LATE_SUM_SQ) {
        set_error("%s: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

}  // namespace

// the late interaction over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine option): the
// label column brought up to date, then the one launch (lists_host.h: docs.cpp's composed search launches it too)
int hx::late_interaction_lists(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                               const float *d_Q, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                               const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels, float *d_scores,
                               uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs,
                               hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::DiverseLists d{};
    if (int rc = hx::labels_on_device(h, &d.labels, &d.label_len)) return rc;
    d.ids = d_ids_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = pool;
    d.n_out = n_out;
    d.nq = (uint32_t)nq;
    d.out_ids = d_doc_labels;
    d.out_dists = d_scores;
    d.out_counts = d_counts;
    d.out_stats = d_stats;
    d.n_vecs = n_vecs;
    d.mode = mode;
    d.queries = d_Q;
    d.best_out = d_best_ids;
    d.sizes_out = d_doc_sizes;
    d.n_docs_out = d_n_docs;
    if (int rc = hx::launch_late_interaction(h->dev.view, d, stream)) return rc;
    h->n_late_launches.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

extern "C" {

int hnsw_late_interaction_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                                 const float *d_Q, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                                 const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels, float *d_scores,
                                 uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs,
                                 hnsw_query_stats *d_stats, void *stream_v) {
    if (int rc = hx::need_handle("late interaction", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_late_shape("late interaction", "n_out", n_vecs, pool, n_out, mode)) return rc;
    if (int rc = hx::check_nq("late interaction", nq)) return rc;
    if (!d_Q || !d_ids_in || !d_doc_labels || !d_scores) {
        set_error("late interaction: needs the vectors, the candidates' ids and the label and score outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("late interaction", "candidates'", d_stats_in, d_stats)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    hx::DeviceQueries dq;  // the caller's vectors are const to us: the unit-length copy under the cosine option
    if (int rc = dq.prepare(h, d_Q, nq * n_vecs, stream)) return rc;
    return hx::late_interaction_lists(h, nq, n_vecs, pool, n_out, mode, dq.q, d_ids_in, d_counts_in, d_stats_in, d_doc_labels,
                                      d_scores, d_best_ids, d_doc_sizes, d_counts, d_n_docs, d_stats, stream);
}

int hnsw_search_batch_late(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_vecs, uint32_t mode, uint32_t n,
                           uint32_t pool, uint32_t ef, uint32_t *doc_labels, float *scores, uint32_t *best_ids,
                           uint32_t *doc_sizes, uint32_t *counts, uint32_t *n_docs, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_late_shape("late search", "n", n_vecs, pool, n, mode))) return rc;
    const bool host_form = h->del.count != 0;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("late search: needs pool <= %d while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !doc_labels || nq > 0x7FFFFFFFull / n_vecs) {
        set_error("late search: needs queries, a label buffer and at most 2^31 - 1 vectors in all");
        return HNSW_ERR_ARG;
    }
    const uint64_t rows = nq * n_vecs;  // the vectors, taken as one batch of queries
    const uint32_t efp = std::max(std::max(ef, pool), 1u);
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, rows, pool, efp, {}, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [vectors [rows][dim] | re-run selection | candidate block (rows, pool) | scored block];
    // pinned arena: [the candidates' stats | scored block]
    const hx::ResultBlock cand(rows, pool);
    hx::ColumnBlock out;  // [labels | scores | best ids | sizes | counts | n_docs | stats]
    const size_t c_labels = out.add(nq * n * 4), c_scores = out.add(nq * n * 4), c_best = out.add(nq * n * 4);
    const size_t c_sizes = out.add(nq * n * 4), c_counts = out.add(nq * 4), c_n_docs = out.add(nq * 4);
    const size_t c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_resel = o_q + hx::align256(rows * v.dim * 4);
    const size_t o_cand = o_resel + hx::align256(rows * 4), o_out = o_cand + cand.bytes;
    const size_t p_out = hx::align256(rows * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    // the one copy of the vectors serves the search AND the late interaction
    if ((rc = hx::queries_up(h, d_Q, Q, rows, sc.stream))) return rc;
    if (host_form)  // (the distances are not an input of the late interaction)
        rc = hx::upload(lists, c, sc.stream, false);
    else
        rc = hx::device_candidates(v, d_Q, rows, pool, efp, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = hx::late_interaction_lists(h, nq, n_vecs, pool, n, mode, d_Q, c.ids, c.counts, c.stats,
                                    hx::at<uint32_t>(d_out, c_labels), hx::at<float>(d_out, c_scores),
                                    hx::at<uint32_t>(d_out, c_best), hx::at<uint32_t>(d_out, c_sizes),
                                    hx::at<uint32_t>(d_out, c_counts), hx::at<uint32_t>(d_out, c_n_docs),
                                    hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_late_calls,
                          {doc_labels, scores, best_ids, doc_sizes, counts, n_docs, stats}, nq);
}

}  // extern "C"
