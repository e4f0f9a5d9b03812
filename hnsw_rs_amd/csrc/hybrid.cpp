// hybrid.cpp -- hybrid search (include/hnsw_mi355x.h, "hybrid search"): the rank fusion of the index's own hits with
// external ranked lists on the device, under the handle's deletions, mask rows and label ranges, and a search answered by
// it.  Host logic only; the fusion is hx_distance_kernel's eighth source form (exact_scan.hip), the candidate stage around
// it lists_host.h.

#include <mutex>

#include "lists_host.h"

using hx::set_error;

static_assert(HX_HYBRID_MAX_EXT == HNSW_HYBRID_MAX_EXT, "the kernel's list limit is the ABI's");
static_assert(HX_DIVERSE_POOL_MAX == HNSW_FUSE_MAX_CANDS, "the kernel's LDS table holds the ABI's candidate limit");
static_assert(sizeof(hx::DiverseLists::absent) == HNSW_HYBRID_MAX_EXT * sizeof(float), "one absent value per external list");

namespace {

// what a call says of its lists and its mode (`what`: the entry point, `n`: its name for the output length, for the text)
struct HybridShape {
    uint32_t mode, rank_constant, n_out, pool, n_ext, ext_width;
    bool dense, ext_ids, ext_scores, have_q, want_dists;
};
int check_hybrid_shape(const char *what, const char *n, const HybridShape &s) {
    if (s.n_ext > HNSW_HYBRID_MAX_EXT) {
        set_error("%s: needs n_ext <= %d", what, HNSW_HYBRID_MAX_EXT);
        return HNSW_ERR_ARG;
    }
    const uint64_t total = (s.dense ? (uint64_t)s.pool : 0) + (uint64_t)s.n_ext * s.ext_width;
    if (total == 0) {
        set_error("%s: needs at least one list: the dense one or an external one", what);
        return HNSW_ERR_ARG;
    }
    if (total > HNSW_FUSE_MAX_CANDS || s.n_out == 0 || s.n_out > total) {
        set_error("%s: needs pool + n_ext * ext_width <= %d and 1 <= %s <= that total", what, HNSW_FUSE_MAX_CANDS, n);
        return HNSW_ERR_ARG;
    }
    if (s.mode != HNSW_HYBRID_RRF && s.mode != HNSW_HYBRID_LINEAR) {
        set_error("%s: the mode is HNSW_HYBRID_RRF (0) or HNSW_HYBRID_LINEAR (1)", what);
        return HNSW_ERR_ARG;
    }
    if (s.mode == HNSW_HYBRID_RRF && (s.rank_constant == 0 || s.rank_constant > (1u << 20))) {
        set_error("%s: reciprocal rank fusion needs 1 <= rank_constant <= 2^20", what);
        return HNSW_ERR_ARG;
    }
    if (s.n_ext != 0 && !s.ext_ids) {
        set_error("%s: needs the external lists' ids", what);
        return HNSW_ERR_ARG;
    }
    if (s.mode == HNSW_HYBRID_LINEAR && s.n_ext != 0 && !s.ext_scores) {
        set_error("%s: the linear mode needs the external lists' scores", what);
        return HNSW_ERR_ARG;
    }
    if (s.mode == HNSW_HYBRID_LINEAR && s.n_ext == 0 && !s.have_q) {
        set_error("%s: the linear mode needs the queries or an external list", what);
        return HNSW_ERR_ARG;
    }
    if (s.want_dists && !s.have_q) {
        set_error("%s: the distance output needs the queries", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// the filter's own argument errors, and a set whose row 0 every query would name without there being one
int check_hybrid_filter(const char *what, const hnsw_index *h, const hx::CandidateFilter &f) {
    if (int rc = hx::check_candidate_filter(what, h, f)) return rc;
    if (f.set && !f.mask_of && f.set->n_masks == 0) {
        set_error("%s: every query names row 0 of a set without rows", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// the lists of a call, all in HBM but `absent`
struct RankedLists {
    uint32_t pool, n_ext, ext_width;
    const uint32_t *ids0, *counts0;
    const hnsw_query_stats *stats0;
    const uint32_t *ext_ids;
    const float *ext_scores;
    const uint32_t *ext_counts;
    const float *weights, *absent /* host */;
};
struct RankedOut {
    uint32_t *ids;
    float *scores, *dists;
    uint32_t *counts, *unique, *dropped;
    hnsw_query_stats *stats;
};

// THE RANK FUSION over lists already in HBM, d_Q as the kernel stages it (unit length under the cosine option; nullptr:
// none), the filter's arrays in HBM too: the deleted mask, the label column and the set's words brought up to date as the
// call needs them, then the one launch
int fuse_ranked(hnsw_index *h, uint64_t nq, uint32_t mode, uint32_t rank_constant, uint32_t n_out, const RankedLists &l,
                const float *d_Q, const hx::CandidateFilter &f, const RankedOut &o, hipStream_t stream) {
    hx::DiverseLists d{};
    if (int rc = hx::deleted_on_device(h, &d.deny, &d.deny_bits)) return rc;
    if (f.lo) {
        if (int rc = hx::labels_on_device(h, &d.labels, &d.label_len)) return rc;
    }
    if (f.set) {
        std::lock_guard<std::mutex> g(f.set->mu);
        if (int rc = f.set->sync(h)) return rc;
        d.rowed = 1;
        d.allow = f.set->d_rows();
        d.allow_bits = f.set->allow_bits;
        d.mask_words = f.set->W;
        d.n_masks = f.set->n_masks;
        d.mask_of = f.mask_of;
    }
    d.range_lo = f.lo;
    d.range_hi = f.hi;
    d.ids = l.ids0;
    d.counts = l.ids0 ? l.counts0 : nullptr;
    d.stats = l.stats0;
    d.pool = l.ids0 ? l.pool : 0;
    d.n_out = n_out;
    d.nq = (uint32_t)nq;
    d.mode = mode;
    d.rank_constant = rank_constant;
    d.n_ext = l.n_ext;
    d.ext_width = l.ext_width;
    d.ext_ids = l.ext_ids;
    d.ext_scores = l.ext_scores;
    d.ext_counts = l.ext_counts;
    d.weights = l.weights;
    for (uint32_t e = 0; e < l.n_ext; e++) d.absent[e] = l.absent ? l.absent[e] : 0.0f;
    d.queries = d_Q;
    d.out_ids = o.ids;
    d.out_dists = o.scores;
    d.out_gaps = o.dists;
    d.out_counts = o.counts;
    d.unique_out = o.unique;
    d.dropped_out = o.dropped;
    d.out_stats = o.stats;
    if (int rc = hx::launch_fuse_ranked(h->dev.view, d, stream)) return rc;
    h->n_hybrid_fuse.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

}  // namespace

extern "C" {

int hnsw_fuse_ranked_device(hnsw_index *h, uint64_t nq, uint32_t mode, uint32_t rank_constant, uint32_t n_out, uint32_t pool,
                            const uint32_t *d_ids0, const uint32_t *d_counts0, const hnsw_query_stats *d_stats0, uint32_t n_ext,
                            uint32_t ext_width, const uint32_t *d_ext_ids, const float *d_ext_scores,
                            const uint32_t *d_ext_counts, const float *d_weights, const float *absent, const float *d_Q,
                            hnsw_mask_set *set, const uint32_t *d_mask_of, const uint32_t *d_lo, const uint32_t *d_hi,
                            uint32_t *d_ids, float *d_scores, float *d_dists, uint32_t *d_counts, uint32_t *d_unique,
                            uint32_t *d_dropped, hnsw_query_stats *d_stats, void *stream_v) {
    if (int rc = hx::need_handle("fuse ranked", h)) return rc;
    if (nq == 0) return HNSW_OK;
    const HybridShape shape{mode,           rank_constant,           n_out,          pool,           n_ext, ext_width, d_ids0 != nullptr,
                            d_ext_ids != nullptr, d_ext_scores != nullptr, d_Q != nullptr, d_dists != nullptr};
    if (int rc = check_hybrid_shape("fuse ranked", "n_out", shape)) return rc;
    if (int rc = hx::check_nq("fuse ranked", nq)) return rc;
    if (!d_ids || !d_scores) {
        set_error("fuse ranked: needs the id and score outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("fuse ranked", "dense list's", d_stats0, d_stats)) return rc;
    const hx::CandidateFilter f{set, d_mask_of, d_lo, d_hi};
    if (int rc = check_hybrid_filter("fuse ranked", h, f)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    hx::DeviceQueries dq;  // the caller's rows are const to us: the unit-length copy under the cosine option
    if (d_Q) {
        if (int rc = dq.prepare(h, d_Q, nq, stream)) return rc;
    }
    const RankedLists l{pool, n_ext, ext_width, d_ids0, d_counts0, d_stats0, d_ext_ids, d_ext_scores, d_ext_counts, d_weights, absent};
    return fuse_ranked(h, nq, mode, rank_constant, n_out, l, dq.q, f, {d_ids, d_scores, d_dists, d_counts, d_unique, d_dropped, d_stats},
                       stream);
}

int hnsw_search_batch_hybrid(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t pool, uint32_t ef, uint32_t mode,
                             uint32_t rank_constant, uint32_t n_ext, uint32_t ext_width, const uint32_t *ext_ids,
                             const float *ext_scores, const uint32_t *ext_counts, const float *weights, const float *absent,
                             hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo, const uint32_t *hi, uint32_t *ids,
                             float *scores, float *dists, uint32_t *counts, uint32_t *unique, uint32_t *dropped,
                             hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    const hx::CandidateFilter f{set, mask_of, lo, hi};
    if ((rc = check_hybrid_filter("hybrid search", h, f))) return rc;
    if (nq == 0) return HNSW_OK;
    if (pool == 0) {
        set_error("hybrid search: needs pool >= 1");
        return HNSW_ERR_ARG;
    }
    const HybridShape shape{mode, rank_constant, n, pool, n_ext, ext_width, true, ext_ids != nullptr, ext_scores != nullptr, true, false};
    if ((rc = check_hybrid_shape("hybrid search", "n", shape))) return rc;
    const bool host_form = f.filtered() || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("hybrid search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || nq > 0x7FFFFFFFull) {
        set_error("hybrid search: needs queries, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, nq, pool, ef, f, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [queries | re-run selection | external ids | external scores | external counts | weights | mask_of |
    // lo | hi | candidate block (nq, pool) | fused block]; pinned arena: [the candidates' stats | fused block]
    const hx::ResultBlock cand(nq, pool);
    hx::ColumnBlock out;  // [ids | scores | dists | counts | unique | dropped | stats]
    const size_t c_ids = out.add(nq * n * 4), c_scores = out.add(nq * n * 4), c_dists = out.add(nq * n * 4);
    const size_t c_counts = out.add(nq * 4), c_unique = out.add(nq * 4), c_dropped = out.add(nq * 4);
    const size_t c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t ext_bytes = nq * n_ext * ext_width * 4;
    const size_t o_q = 0, o_resel = o_q + hx::align256(nq * v.dim * 4), o_eids = o_resel + hx::align256(nq * 4);
    const size_t o_esc = o_eids + hx::align256(ext_bytes), o_ecnt = o_esc + hx::align256(ext_bytes);
    const size_t o_w = o_ecnt + hx::align256(nq * n_ext * 4), o_mof = o_w + hx::align256(nq * (1 + n_ext) * 4);
    const size_t o_lo = o_mof + hx::align256(nq * 4), o_hi = o_lo + hx::align256(nq * 4), o_cand = o_hi + hx::align256(nq * 4);
    const size_t o_out = o_cand + cand.bytes, p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    // the one copy of the queries serves the search AND the fusion
    if ((rc = hx::queries_up(h, d_Q, Q, nq, sc.stream))) return rc;
    auto up = [&](size_t off, const void *src, size_t bytes) -> const void * {  // a host array of the call into the arena
        if (!src || bytes == 0) return nullptr;
        if (hipMemcpyAsync(dv + off, src, bytes, hipMemcpyHostToDevice, sc.stream) != hipSuccess) rc = HNSW_ERR_HIP;
        return dv + off;
    };
    RankedLists l{pool, n_ext, ext_width, c.ids, c.counts, c.stats, nullptr, nullptr, nullptr, nullptr, absent};
    l.ext_ids = static_cast<const uint32_t *>(up(o_eids, ext_ids, ext_bytes));
    l.ext_scores = static_cast<const float *>(up(o_esc, ext_scores, ext_bytes));
    l.ext_counts = static_cast<const uint32_t *>(up(o_ecnt, ext_counts, nq * n_ext * 4));
    l.weights = static_cast<const float *>(up(o_w, weights, nq * (1 + n_ext) * 4));
    hx::CandidateFilter df{set, nullptr, nullptr, nullptr};  // the filter's arrays as the kernel reads them
    df.mask_of = static_cast<const uint32_t *>(up(o_mof, mask_of, nq * 4));
    df.lo = static_cast<const uint32_t *>(up(o_lo, lo, nq * 4));
    df.hi = static_cast<const uint32_t *>(up(o_hi, hi, nq * 4));
    if (rc != HNSW_OK) {
        set_error("hybrid search: copying the external lists to the device failed");
        return rc;
    }
    if (host_form)  // (the distances are not an input of the fusion)
        rc = hx::upload(lists, c, sc.stream, false);
    else
        rc = hx::device_candidates(v, d_Q, nq, pool, ef, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = fuse_ranked(h, nq, mode, rank_constant, n, l, d_Q, df,
                     {hx::at<uint32_t>(d_out, c_ids), hx::at<float>(d_out, c_scores), dists ? hx::at<float>(d_out, c_dists) : nullptr,
                      hx::at<uint32_t>(d_out, c_counts), hx::at<uint32_t>(d_out, c_unique), hx::at<uint32_t>(d_out, c_dropped),
                      hx::at<hnsw_query_stats>(d_out, c_stats)},
                     sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_hybrid_calls, {ids, scores, dists, counts, unique, dropped, stats},
                          nq);
}

}  // extern "C"
