// docs.cpp -- exact document scoring (include/hnsw_mi355x.h, "exact document scoring"): the documents a list names -- the
// undeleted rows that share a label -- scored against a query's vectors by summed min distance over EVERY stored row of
// the document, and a late-interaction search whose returned documents are completed that way.  Host logic only; the
// scoring is hx_distance_kernel's seventh source form (exact_scan.hip), the document index it walks the HBM copy of
// LabelColumn::sorted (labels.h), the candidate stage around it lists_host.h.

#include <algorithm>

#include "lists_host.h"

using hx::set_error;

static_assert(HX_LATE_MAX_VECS == HNSW_LATE_MAX_VECS, "the kernel's vector limit is the ABI's");
static_assert(HX_DOCS_MAX_IN == HNSW_DOCS_MAX_IN, "the kernel's document tables hold the ABI's list length");
static_assert(HX_DOCS_MAX_ROWS == HNSW_DOCS_MAX_ROWS, "the kernel's row limit is the ABI's");
static_assert(HNSW_DOCS_MAX_IN == HNSW_LATE_MAX_DOCS, "a late interaction's whole output is a legal list");

namespace {

int check_vecs(const char *what, uint32_t n_vecs) {
    if (n_vecs >= 1 && n_vecs <= HNSW_LATE_MAX_VECS) return HNSW_OK;
    set_error("%s: needs 1 <= n_vecs <= %d", what, HNSW_LATE_MAX_VECS);
    return HNSW_ERR_ARG;
}

int check_mode(const char *what, uint32_t mode) {
    if (mode == HNSW_LATE_SUM || mode == HNSW_LATE_SUM_SQ) return HNSW_OK;
    set_error("%s: the mode is HNSW_LATE_SUM (0) or HNSW_LATE_SUM_SQ (1)", what);
    return HNSW_ERR_ARG;
}

// the limits of the document scoring
int check_docs_shape(uint32_t n_vecs, uint32_t n_in, uint32_t n_out, uint32_t rows_cap, uint32_t mode) {
    const char *what = "document scoring";
    if (int rc = check_vecs(what, n_vecs)) return rc;
    if (n_out == 0 || n_out > n_in || n_in > HNSW_DOCS_MAX_IN || rows_cap == 0 || rows_cap > HNSW_DOCS_MAX_ROWS) {
        set_error("%s: needs 1 <= n_out <= n_in <= %d and 1 <= rows_cap <= %d", what, HNSW_DOCS_MAX_IN, HNSW_DOCS_MAX_ROWS);
        return HNSW_ERR_ARG;
    }
    return check_mode(what, mode);
}

// ... and of the search completed by it
int check_exact_shape(uint32_t n_vecs, uint32_t pool, uint32_t n, uint32_t n_cand, uint32_t rows_cap, uint32_t mode) {
    const char *what = "exact late search";
    if (int rc = check_vecs(what, n_vecs)) return rc;
    const uint64_t total = (uint64_t)n_vecs * pool;
    if (n == 0 || n > n_cand || n_cand > total || n_cand > HNSW_DOCS_MAX_IN || total > HNSW_LATE_MAX_CANDS || rows_cap == 0 ||
        rows_cap > HNSW_DOCS_MAX_ROWS) {
        set_error("%s: needs n_vecs * pool <= %d, 1 <= n <= n_cand <= min(n_vecs * pool, %d) and 1 <= rows_cap <= %d", what,
                  HNSW_LATE_MAX_CANDS, HNSW_DOCS_MAX_IN, HNSW_DOCS_MAX_ROWS);
        return HNSW_ERR_ARG;
    }
    return check_mode(what, mode);
}

// The document index in HBM: LabelColumn::sorted -- the keys label << 32 | id of the undeleted ids below the index length,
// ascending -- as of this call.  The sort runs under the column's lock (a no-op while the column, the deleted set and
// the length are what it was made for); the copy is made whole, on a stream of the handle's own that is synchronised
// before returning, when it was made for another (label version, deleted version, length) or another device, and
// nothing moves otherwise.  The snapshot's device must be known (ensure_uploaded).
int doc_index_on_device(hnsw_index *h, const uint64_t **d_keys, uint64_t *n_keys) {
    std::lock_guard<std::mutex> g(h->mu);
    std::lock_guard<std::mutex> lg(h->lab.mu);
    hx::LabelColumn &lab = h->lab;
    lab.sort_for(h->del, hx::index_len(h));
    hx::DocIndex &di = lab.doc;
    const int device = h->dev.device;
    if (!(di.d_keys && di.device == device && di.version == lab.s_version && di.del == lab.s_del && di.len == lab.s_len)) {
        hx::ScratchLease lease(h);
        if (int rc = lease.prepare(device, 0, 0)) return rc;
        const uint64_t n = lab.sorted.size();
        if (!di.d_keys || di.device != device || di.cap < n) {
            di.release();
            const uint64_t cap = std::max<uint64_t>(n + n / 8, 16);  // (never empty: the kernel is handed a pointer)
            HIP_TRY(hipSetDevice(device));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&di.d_keys), cap * 8));
            di.cap = cap;
            di.device = device;
        }
        if (n) HIP_TRY(hipMemcpyAsync(di.d_keys, lab.sorted.data(), n * 8, hipMemcpyHostToDevice, lease.s->stream));
        HIP_TRY(hipStreamSynchronize(lease.s->stream));
        di.n = n;
        di.version = lab.s_version, di.del = lab.s_del, di.len = lab.s_len;
        di.uploads++;
        di.keys_uploaded += n;
    }
    *d_keys = di.d_keys;
    *n_keys = di.n;
    return HNSW_OK;
}

// the document scoring over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine option): the
// document index brought up to date, then the one launch
int score(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t n_in, uint32_t n_out, uint32_t rows_cap, uint32_t mode,
          const float *d_Q, const uint32_t *d_docs_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in,
          uint32_t *d_doc_labels, float *d_scores, uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts,
          uint32_t *d_n_docs, hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::DiverseLists d{};
    if (int rc = doc_index_on_device(h, &d.doc_keys, &d.n_doc_keys)) return rc;
    d.ids = d_docs_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = n_in;
    d.n_out = n_out;
    d.rows_cap = rows_cap;
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
    if (int rc = hx::launch_score_documents(h->dev.view, d, stream)) return rc;
    h->n_docs_launches.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

}  // namespace

extern "C" {

int hnsw_score_documents_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t n_in, uint32_t n_out, uint32_t rows_cap,
                                uint32_t mode, const float *d_Q, const uint32_t *d_docs_in, const uint32_t *d_counts_in,
                                const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels, float *d_scores,
                                uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs,
                                hnsw_query_stats *d_stats, void *stream_v) {
    if (int rc = hx::need_handle("document scoring", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_docs_shape(n_vecs, n_in, n_out, rows_cap, mode)) return rc;
    if (int rc = hx::check_nq("document scoring", nq)) return rc;
    if (!d_Q || !d_docs_in || !d_doc_labels || !d_scores) {
        set_error("document scoring: needs the vectors, the documents' labels and the label and score outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("document scoring", "documents'", d_stats_in, d_stats)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    hx::DeviceQueries dq;  // the caller's vectors are const to us: the unit-length copy under the cosine option
    if (int rc = dq.prepare(h, d_Q, nq * n_vecs, stream)) return rc;
    return score(h, nq, n_vecs, n_in, n_out, rows_cap, mode, dq.q, d_docs_in, d_counts_in, d_stats_in, d_doc_labels, d_scores,
                 d_best_ids, d_doc_sizes, d_counts, d_n_docs, d_stats, stream);
}

int hnsw_search_batch_late_exact(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_vecs, uint32_t mode, uint32_t n,
                                 uint32_t n_cand, uint32_t rows_cap, uint32_t pool, uint32_t ef, uint32_t *doc_labels,
                                 float *scores, uint32_t *best_ids, uint32_t *doc_sizes, uint32_t *counts, uint32_t *n_docs,
                                 hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_exact_shape(n_vecs, pool, n, n_cand, rows_cap, mode))) return rc;
    const bool host_form = h->del.count != 0;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("exact late search: needs pool <= %d while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !doc_labels || nq > 0x7FFFFFFFull / n_vecs) {
        set_error("exact late search: needs queries, a label buffer and at most 2^31 - 1 vectors in all");
        return HNSW_ERR_ARG;
    }
    const uint64_t rows = nq * n_vecs;  // the vectors, taken as one batch of queries
    const uint32_t efp = std::max(std::max(ef, pool), 1u);
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, rows, pool, efp, {}, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [vectors [rows][dim] | re-run selection | candidate block (rows, pool) | the late interaction's
    // documents (nq, n_cand): labels, scores, counts, stats | scored block]; pinned arena: [the candidates' stats | scored block]
    const hx::ResultBlock cand(rows, pool), mid(nq, n_cand);
    hx::ColumnBlock out;  // [labels | scores | best ids | sizes | counts | n_docs | stats]
    const size_t c_labels = out.add(nq * n * 4), c_scores = out.add(nq * n * 4), c_best = out.add(nq * n * 4);
    const size_t c_sizes = out.add(nq * n * 4), c_counts = out.add(nq * 4), c_n_docs = out.add(nq * 4);
    const size_t c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_resel = o_q + hx::align256(rows * v.dim * 4);
    const size_t o_cand = o_resel + hx::align256(rows * 4), o_mid = o_cand + cand.bytes, o_out = o_mid + mid.bytes;
    const size_t p_out = hx::align256(rows * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand), m = mid.at(dv + o_mid);
    // the one copy of the vectors serves the search, the late interaction AND the scoring
    if ((rc = hx::queries_up(h, d_Q, Q, rows, sc.stream))) return rc;
    if (host_form)  // (the distances are not an input of the late interaction)
        rc = hx::upload(lists, c, sc.stream, false);
    else
        rc = hx::device_candidates(v, d_Q, rows, pool, efp, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    if (rc != HNSW_OK) return rc;
    // the late interaction names the documents: its labels, counts and stats are the scoring's list
    rc = hx::late_interaction_lists(h, nq, n_vecs, pool, n_cand, mode, d_Q, c.ids, c.counts, c.stats, m.ids, m.dists, nullptr,
                                    nullptr, m.counts, nullptr, m.stats, sc.stream);
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = score(h, nq, n_vecs, n_cand, n, rows_cap, mode, d_Q, m.ids, m.counts, m.stats, hx::at<uint32_t>(d_out, c_labels),
               hx::at<float>(d_out, c_scores), hx::at<uint32_t>(d_out, c_best), hx::at<uint32_t>(d_out, c_sizes),
               hx::at<uint32_t>(d_out, c_counts), hx::at<uint32_t>(d_out, c_n_docs), hx::at<hnsw_query_stats>(d_out, c_stats),
               sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_docs_calls,
                          {doc_labels, scores, best_ids, doc_sizes, counts, n_docs, stats}, nq);
}

}  // extern "C"
