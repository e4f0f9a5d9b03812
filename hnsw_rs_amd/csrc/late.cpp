// late.cpp -- late-interaction search (include/hnsw_mi355x.h, "late-interaction search"): a query's per-vector candidate
// lists scored as documents -- the candidates that share a label -- by summed min distance on the device, and a search
// answered by its nearest documents.  Host logic only; the scoring is hx_distance_kernel's fifth source form
// (exact_scan.hip).

#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"
#include "rerun.h"
#include "search_filtered.h"
#include "search_host.h"

using hx::set_error;

static_assert(HX_LATE_MAX_VECS == HNSW_LATE_MAX_VECS, "the kernel's vector limit is the ABI's");
static_assert(HX_LATE_MAX_CANDS == HNSW_LATE_MAX_CANDS, "the kernel's LDS table holds the ABI's candidate limit");
static_assert(HX_LATE_MAX_DOCS == HNSW_LATE_MAX_DOCS, "the kernel's document limit is the ABI's");

namespace {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

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

// The scored block of nq queries x n: [labels | scores | best ids | sizes | counts | n_docs | stats], the same layout in
// the device arena and in pinned memory, so it comes back in ONE copy (as FusedBlock, multi.cpp).
struct LateBlock {
    size_t labels = 0, scores, best, sizes, counts, n_docs, stats, bytes;
    LateBlock(uint64_t nq, uint32_t n) {
        scores = labels + hx::align256(nq * n * 4);
        best = scores + hx::align256(nq * n * 4);
        sizes = best + hx::align256(nq * n * 4);
        counts = sizes + hx::align256(nq * n * 4);
        n_docs = counts + hx::align256(nq * 4);
        stats = n_docs + hx::align256(nq * 4);
        bytes = stats + hx::align256(nq * sizeof(hnsw_query_stats));
    }
    template <class T>
    T *at(void *base, size_t off) const {
        return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off);
    }
};

// the late interaction over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine option): the
// label column brought up to date, then the one launch
int score(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode, const float *d_Q,
          const uint32_t *d_ids_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels,
          float *d_scores, uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs,
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

}  // namespace

extern "C" {

int hnsw_late_interaction_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                                 const float *d_Q, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                                 const hnsw_query_stats *d_stats_in, uint32_t *d_doc_labels, float *d_scores,
                                 uint32_t *d_best_ids, uint32_t *d_doc_sizes, uint32_t *d_counts, uint32_t *d_n_docs,
                                 hnsw_query_stats *d_stats, void *stream_v) {
    if (!h) {
        set_error("late interaction: null handle");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if (int rc = check_late_shape("late interaction", "n_out", n_vecs, pool, n_out, mode)) return rc;
    if (nq > 0x7FFFFFFFull) {
        set_error("late interaction: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_Q || !d_ids_in || !d_doc_labels || !d_scores) {
        set_error("late interaction: needs the vectors, the candidates' ids and the label and score outputs");
        return HNSW_ERR_ARG;
    }
    if ((d_stats_in != nullptr) != (d_stats != nullptr)) {
        set_error("late interaction: the stats output goes with the candidates' stats, both or neither");
        return HNSW_ERR_ARG;
    }
    int rc = hx::check_search_args(h, 0);  // (the lists are a search's: the handle has points and a complete build)
    if (rc != HNSW_OK || (rc = hx::ensure_uploaded(h))) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    hx::DeviceQueries dq;  // the caller's vectors are const to us: the unit-length copy under the cosine option
    if ((rc = dq.prepare(h, d_Q, nq * n_vecs, stream))) return rc;
    return score(h, nq, n_vecs, pool, n_out, mode, dq.q, d_ids_in, d_counts_in, d_stats_in, d_doc_labels, d_scores, d_best_ids,
                 d_doc_sizes, d_counts, d_n_docs, d_stats, stream);
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
    // The candidates while ids are deleted are the HOST form's: only it lets the planner choose the exact path, and the
    // call is defined by it (as multi.cpp)
    std::vector<uint32_t> h_ids, h_counts;
    std::vector<float> h_dists;  // (not an input of the late interaction)
    std::vector<hnsw_query_stats> h_stats;
    if (host_form) {
        h_ids.resize(rows * pool), h_dists.resize(rows * pool), h_counts.resize(rows), h_stats.resize(rows);
        rc = hnsw_search_batch(h, Q, rows, pool, efp, h_ids.data(), h_dists.data(), h_counts.data(), h_stats.data());
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    const uint64_t dim = v.dim;
    // device arena: [vectors [rows][dim] | re-run selection | candidate block (rows, pool) | scored block];
    // pinned arena: [the candidates' stats | scored block].  The scored block comes back in one copy.
    const hx::ResultBlock cand(rows, pool);
    const LateBlock out(nq, n);
    const size_t o_q = 0, o_resel = o_q + hx::align256(rows * dim * 4);
    const size_t o_cand = o_resel + hx::align256(rows * 4), o_out = o_cand + cand.bytes;
    const size_t p_out = hx::align256(rows * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = reinterpret_cast<float *>(dv + o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    // Q goes up once; the unit-length copy of the cosine option is made once, from the caller's vectors, and serves the
    // search and the late interaction (as multi.cpp)
    HIP_TRY(hipMemcpyAsync(d_Q, Q, rows * dim * 4, hipMemcpyHostToDevice, sc.stream));
    if ((rc = hx::cosine_queries(h, d_Q, rows, sc.stream))) return rc;
    if (host_form) {  // (the host vectors outlive the copies: the stream is synchronised below)
        HIP_TRY(hipMemcpyAsync(c.ids, h_ids.data(), rows * pool * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(c.counts, h_counts.data(), rows * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(c.stats, h_stats.data(), rows * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, sc.stream));
    } else {  // the launch of hnsw_search_batch_device and the re-run loop of its _finish, over the unit copy made above
        hx::SearchArgs a = hx::ann_args(v, d_Q, pool, efp, c.ids, c.dists, c.counts, c.stats);
        const uint32_t slots = hx::default_slots_log2(efp, v.S0);
        if ((rc = hx::launch_search(v, a, (uint32_t)rows, slots, sc.stream))) return rc;
        rc = hx::rerun_overflowed(
            v, hx::launch_search, a, rows, slots, hx::max_slots_log2(efp), reinterpret_cast<uint32_t *>(dv + o_resel), sc.stream,
            [&](const hnsw_query_stats *&st) -> int {
                HIP_TRY(hipMemcpyAsync(hv, c.stats, rows * sizeof(hnsw_query_stats), hipMemcpyDeviceToHost, sc.stream));
                HIP_TRY(hipStreamSynchronize(sc.stream));
                st = reinterpret_cast<const hnsw_query_stats *>(hv);
                return HNSW_OK;
            },
            nullptr);
        if (rc != HNSW_OK) return rc;
    }
    unsigned char *d_out = dv + o_out;
    rc = score(h, nq, n_vecs, pool, n, mode, d_Q, c.ids, c.counts, c.stats, out.at<uint32_t>(d_out, out.labels),
               out.at<float>(d_out, out.scores), out.at<uint32_t>(d_out, out.best), out.at<uint32_t>(d_out, out.sizes),
               out.at<uint32_t>(d_out, out.counts), out.at<uint32_t>(d_out, out.n_docs),
               out.at<hnsw_query_stats>(d_out, out.stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hv + p_out, d_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_late_calls.fetch_add(1, std::memory_order_relaxed);
    memcpy(doc_labels, out.at<uint32_t>(hv + p_out, out.labels), nq * n * 4);
    if (scores) memcpy(scores, out.at<float>(hv + p_out, out.scores), nq * n * 4);
    if (best_ids) memcpy(best_ids, out.at<uint32_t>(hv + p_out, out.best), nq * n * 4);
    if (doc_sizes) memcpy(doc_sizes, out.at<uint32_t>(hv + p_out, out.sizes), nq * n * 4);
    if (counts) memcpy(counts, out.at<uint32_t>(hv + p_out, out.counts), nq * 4);
    if (n_docs) memcpy(n_docs, out.at<uint32_t>(hv + p_out, out.n_docs), nq * 4);
    const hnsw_query_stats *st = out.at<hnsw_query_stats>(hv + p_out, out.stats);
    if (stats) memcpy(stats, st, nq * sizeof(hnsw_query_stats));
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return hx::query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // extern "C"
