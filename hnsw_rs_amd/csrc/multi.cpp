// multi.cpp -- multi-vector search (include/hnsw_mi355x.h, "multi-vector search"): the fusion of a query's per-vector
// candidate lists on the device, and a search answered from several vectors per query.  Host logic only; the fusion is
// hx_distance_kernel's fourth source form (form_fuse_lists.inc), the candidate stage around it lists_host.h.

#include <algorithm>

#include "list_forms.h"
#include "lists_host.h"

using hx::set_error;

static_assert(HX_MULTI_MAX_VECS == HNSW_MULTI_MAX_VECS, "the kernel's vector limit is the ABI's");
static_assert(HX_DIVERSE_POOL_MAX == HNSW_FUSE_MAX_CANDS, "the kernel's LDS table holds the ABI's candidate limit");

namespace {

// the limits of the fusion (`what`: the entry point, `n`: its name for the output length, for the text)
int check_fuse_shape(const char *what, const char *n, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode) {
    if (n_vecs == 0 || n_vecs > HNSW_MULTI_MAX_VECS) {
        set_error("%s: needs 1 <= n_vecs <= %d", what, HNSW_MULTI_MAX_VECS);
        return HNSW_ERR_ARG;
    }
    if (n_out == 0 || n_out > pool || (uint64_t)n_vecs * pool > HNSW_FUSE_MAX_CANDS) {
        set_error("%s: needs 1 <= %s <= pool and n_vecs * pool <= %d", what, n, HNSW_FUSE_MAX_CANDS);
        return HNSW_ERR_ARG;
    }
    if (mode != HNSW_FUSE_SUM && mode != HNSW_FUSE_MIN) {
        set_error("%s: the mode is HNSW_FUSE_SUM (0) or HNSW_FUSE_MIN (1)", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// the fusion over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine option): the one launch
int fuse(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode, const float *d_Q,
         const float *d_weights, const uint32_t *d_ids_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in,
         uint32_t *d_ids, float *d_scores, uint32_t *d_counts, uint32_t *d_unique, hnsw_query_stats *d_stats,
         hipStream_t stream) {
    hx::DiverseLists d{};
    d.ids = d_ids_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = pool;
    d.n_out = n_out;
    d.nq = (uint32_t)nq;
    d.out_ids = d_ids;
    d.out_dists = d_scores;
    d.out_counts = d_counts;
    d.out_stats = d_stats;
    d.n_vecs = n_vecs;
    d.mode = mode;
    d.weights = d_weights;
    d.queries = d_Q;
    d.unique_out = d_unique;
    if (int rc = hx::launch_fuse_lists(h->dev.view, d, stream)) return rc;
    h->n_multi_fuse.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

}  // namespace

extern "C" {

int hnsw_fuse_lists_device(hnsw_index *h, uint64_t nq, uint32_t n_vecs, uint32_t pool, uint32_t n_out, uint32_t mode,
                           const float *d_Q, const float *d_weights, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                           const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_scores, uint32_t *d_counts,
                           uint32_t *d_unique, hnsw_query_stats *d_stats, void *stream_v) {
    if (int rc = hx::need_handle("fuse lists", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_fuse_shape("fuse lists", "n_out", n_vecs, pool, n_out, mode)) return rc;
    if (int rc = hx::check_nq("fuse lists", nq)) return rc;
    if (!d_Q || !d_ids_in || !d_ids || !d_scores) {
        set_error("fuse lists: needs the vectors, the candidates' ids and the id and score outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("fuse lists", "candidates'", d_stats_in, d_stats)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    hx::DeviceQueries dq;  // the caller's vectors are const to us: the unit-length copy under the cosine option
    if (int rc = dq.prepare(h, d_Q, nq * n_vecs, stream)) return rc;
    return fuse(h, nq, n_vecs, pool, n_out, mode, dq.q, d_weights, d_ids_in, d_counts_in, d_stats_in, d_ids, d_scores, d_counts,
                d_unique, d_stats, stream);
}

int hnsw_search_batch_multi(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_vecs, const float *weights, uint32_t mode,
                            uint32_t n, uint32_t pool, uint32_t ef, uint32_t *ids, float *scores, uint32_t *counts,
                            uint32_t *unique, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_fuse_shape("multi search", "n", n_vecs, pool, n, mode))) return rc;
    const bool host_form = h->del.count != 0;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("multi search: needs pool <= %d while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || nq > 0x7FFFFFFFull / n_vecs) {
        set_error("multi search: needs queries, an id buffer and at most 2^31 - 1 vectors in all");
        return HNSW_ERR_ARG;
    }
    const uint64_t rows = nq * n_vecs;  // the vectors, taken as one batch of queries
    const uint32_t efp = std::max(std::max(ef, pool), 1u);
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, rows, pool, efp, {}, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [vectors [rows][dim] | weights [rows] | re-run selection | candidate block (rows, pool) | fused block];
    // pinned arena: [the candidates' stats | fused block]
    const hx::ResultBlock cand(rows, pool);
    hx::ColumnBlock out;  // [ids | scores | counts | unique | stats]
    const size_t c_ids = out.add(nq * n * 4), c_scores = out.add(nq * n * 4), c_counts = out.add(nq * 4);
    const size_t c_unique = out.add(nq * 4), c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_w = o_q + hx::align256(rows * v.dim * 4), o_resel = o_w + hx::align256(rows * 4);
    const size_t o_cand = o_resel + hx::align256(rows * 4), o_out = o_cand + cand.bytes;
    const size_t p_out = hx::align256(rows * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q), *d_w = weights ? hx::at<float>(dv, o_w) : nullptr;
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    // the one copy of the vectors serves the search AND the fusion
    if ((rc = hx::queries_up(h, d_Q, Q, rows, sc.stream))) return rc;
    if (weights) HIP_TRY(hipMemcpyAsync(d_w, weights, rows * 4, hipMemcpyHostToDevice, sc.stream));
    if (host_form)  // (the distances are not an input of the fusion)
        rc = hx::upload(lists, c, sc.stream, false);
    else
        rc = hx::device_candidates(v, d_Q, rows, pool, efp, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = fuse(h, nq, n_vecs, pool, n, mode, d_Q, d_w, c.ids, c.counts, c.stats, hx::at<uint32_t>(d_out, c_ids),
              hx::at<float>(d_out, c_scores), hx::at<uint32_t>(d_out, c_counts), hx::at<uint32_t>(d_out, c_unique),
              hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_multi_calls, {ids, scores, counts, unique, stats}, nq);
}

}  // extern "C"
