// from_rows.cpp -- search from stored rows (include/hnsw_mi355x.h, "search from stored rows"): query rows composed out
// of stored rows on the device, the sources taken back out of the result lists there, and a search answered from ids and
// weighted ids.  Host logic only; the compose is hx_distance_kernel's third source form (exact_scan.hip), the drop
// hx_filt_merge_kernel's fifth (search_filtered.hip), the candidate stage between them lists_host.h.

#include "lists_host.h"
#include "rerun.h"

using hx::set_error;

static_assert(HX_FROM_ROWS_MAX_TERMS == HNSW_FROM_ROWS_MAX_TERMS, "the compose form's lanes are the ABI's slot limit");
static_assert(HX_DROP_MAX_WIDTH == HNSW_FROM_ROWS_MAX_TERMS, "the drop form's lanes are the ABI's slot limit");
static_assert(HX_RADIUS_MAX_N == HNSW_DROP_MAX_N, "the drop form's list limit is the ABI's");

namespace {

int check_width(const char *what, uint32_t width) {
    if (width == 0 || width > HNSW_FROM_ROWS_MAX_TERMS) {
        set_error("%s: needs 1 <= width <= %d", what, HNSW_FROM_ROWS_MAX_TERMS);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// one compose launch: nq queries of `width` slots into d_rows [nq][dim]
int compose(hnsw_index *h, uint64_t nq, uint32_t width, const uint32_t *d_src_ids, const float *d_weights, float *d_rows,
            int32_t *d_status, hipStream_t stream) {
    if (int rc = hx::launch_compose_rows(h->dev.view, (uint32_t)nq, width, d_src_ids, d_weights, d_rows, d_status, stream))
        return rc;
    h->n_from_rows_compose.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

// one drop launch over nq lists of n_in entries into rows of n_out
int drop(uint64_t nq, uint32_t n_in, uint32_t n_out, uint32_t width, const uint32_t *d_ex, const int32_t *d_src_status,
         const uint32_t *d_ids_in, const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in,
         uint32_t *d_ids, float *d_dists, uint32_t *d_counts, uint32_t *d_dropped, hnsw_query_stats *d_stats,
         hipStream_t stream) {
    hx::MergeLists m{};
    m.ids = d_ids_in;
    m.dists = d_dists_in;
    m.counts = d_counts_in;
    m.stats = d_stats_in;
    m.nq = (uint32_t)nq;
    m.pool = n_in;
    m.drop_out = n_out;
    m.ex = d_ex;
    m.ex_width = width;
    m.src_status = d_src_status;
    m.dropped = d_dropped;
    return hx::launch_drop_ids(m, nullptr, 0, d_ids, d_dists, d_counts, d_stats, stream);
}

}  // namespace

extern "C" {

int hnsw_compose_rows_device(hnsw_index *h, uint64_t nq, uint32_t width, const uint32_t *d_src_ids, const float *d_weights,
                             float *d_Q, int32_t *d_status, void *stream) {
    if (int rc = hx::need_handle("compose rows", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_width("compose rows", width)) return rc;
    if (int rc = hx::check_nq("compose rows", nq)) return rc;
    if (!d_src_ids || !d_Q) {
        set_error("compose rows: needs the source ids and the query rows");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::ready_for_lists(h)) return rc;  // (the rows are a search's queries)
    return compose(h, nq, width, d_src_ids, d_weights, d_Q, d_status, static_cast<hipStream_t>(stream));
}

int hnsw_drop_ids_device(uint64_t nq, uint32_t n_in, uint32_t n_out, uint32_t width, const uint32_t *d_ex,
                         const int32_t *d_src_status, const uint32_t *d_ids_in, const float *d_dists_in,
                         const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_dists,
                         uint32_t *d_counts, uint32_t *d_dropped, hnsw_query_stats *d_stats, void *stream) {
    if (nq == 0) return HNSW_OK;
    if (n_out == 0 || n_out > n_in || n_in > HNSW_DROP_MAX_N) {
        set_error("drop ids: needs 1 <= n_out <= n_in <= %d", HNSW_DROP_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (int rc = check_width("drop ids", width)) return rc;
    if (int rc = hx::check_nq("drop ids", nq)) return rc;
    if (!d_ex || !d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("drop ids: needs the exclusion ids, the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("drop ids", "candidates'", d_stats_in, d_stats)) return rc;
    return drop(nq, n_in, n_out, width, d_ex, d_src_status, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
                d_counts, d_dropped, d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_from_rows(hnsw_index *h, const uint32_t *src_ids, const float *weights, uint64_t nq, uint32_t width,
                                uint32_t n, uint32_t ef, int exclude, uint32_t *ids, float *dists, uint32_t *counts,
                                hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_width("search from rows", width))) return rc;
    if (n == 0 || (uint64_t)n + width > HNSW_DROP_MAX_N) {
        set_error("search from rows: needs n >= 1 and n + width <= %d", HNSW_DROP_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!src_ids || !ids || nq > 0x7FFFFFFFull) {
        set_error("search from rows: needs source ids, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    const uint32_t n_cand = exclude ? n + width : n;
    const bool host_form = h->del.count != 0;
    if (host_form && n + width > HX_FILT_MAX_N) {
        set_error("search from rows: needs n + width <= %d while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    const uint64_t len = hx::index_len(h);
    for (uint64_t q = 0; q < nq; q++) {  // all arrays are the host's: a bad query fails the whole call, here
        bool any = false;
        for (uint32_t s = 0; s < width; s++) {
            const uint32_t id = src_ids[q * width + s];
            if (id == UINT32_MAX) continue;
            any = true;
            if (id >= len) {
                set_error("search from rows: query %llu names source id %u, the index has %llu points", (unsigned long long)q, id,
                          (unsigned long long)len);
                return HNSW_ERR_ARG;
            }
        }
        if (!any) {
            set_error("search from rows: query %llu has no source", (unsigned long long)q);
            return HNSW_ERR_ARG;
        }
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [source ids [nq][width] | weights | query rows [nq][dim] | re-run selection | candidate block (nq,
    // n_cand) | result block (nq, n)]; without the drop the search writes the result block itself.  Pinned arena: [the
    // candidates' stats | result block]
    const hx::ResultBlock cand(nq, n_cand), out(nq, n);
    const size_t o_src = 0, o_w = o_src + hx::align256(nq * width * 4), o_q = o_w + hx::align256(nq * width * 4);
    const size_t o_resel = o_q + hx::align256(nq * v.dim * 4), o_cand = o_resel + hx::align256(nq * 4);
    const size_t o_out = exclude ? o_cand + cand.bytes : o_cand, p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    uint32_t *d_src = hx::at<uint32_t>(dv, o_src);
    float *d_w = weights ? hx::at<float>(dv, o_w) : nullptr, *d_Q = hx::at<float>(dv, o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand), o = out.at(dv + o_out);
    HIP_TRY(hipMemcpyAsync(d_src, src_ids, nq * width * 4, hipMemcpyHostToDevice, sc.stream));
    if (weights) HIP_TRY(hipMemcpyAsync(d_w, weights, nq * width * 4, hipMemcpyHostToDevice, sc.stream));
    if ((rc = compose(h, nq, width, d_src, d_w, d_Q, nullptr, sc.stream))) return rc;
    std::vector<float> h_Q;
    hx::HostLists lists;
    if (host_form) {
        // over the composed rows copied back, RAW: hnsw_search_batch makes their unit-length copy itself, and a row
        // normalised twice is not the row normalised once
        h_Q.resize(nq * v.dim);
        HIP_TRY(hipMemcpyAsync(h_Q.data(), d_Q, nq * v.dim * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(hipStreamSynchronize(sc.stream));
        if ((rc = hx::host_candidates(h, h_Q.data(), nq, n_cand, ef, {}, lists))) return rc;
        rc = hx::upload(lists, c, sc.stream, true);
    } else {  // the composed rows to unit length in place under the cosine option: nothing else reads them
        if ((rc = hx::cosine_queries(h, d_Q, nq, sc.stream))) return rc;
        rc = hx::device_candidates(v, d_Q, nq, n_cand, ef, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    }
    if (rc != HNSW_OK) return rc;
    if (exclude) {
        rc = drop(nq, n_cand, n, width, d_src, nullptr, c.ids, c.dists, c.counts, c.stats, o.ids, o.dists, o.counts, nullptr,
                  o.stats, sc.stream);
        if (rc != HNSW_OK) return rc;
        h->n_from_rows_drop.fetch_add(1, std::memory_order_relaxed);
    }
    HIP_TRY(hipMemcpyAsync(hv + p_out, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_from_rows_calls.fetch_add(1, std::memory_order_relaxed);
    out.copy_out(hv + p_out, ids, dists, counts, stats);
    return hx::first_query_error(out.at(hv + p_out).stats, nq);
}

int hnsw_search_batch_by_id(hnsw_index *h, const uint32_t *src_ids, uint64_t nq, uint32_t n, uint32_t ef, int exclude_self,
                            uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    return hnsw_search_batch_from_rows(h, src_ids, nullptr, nq, 1, n, ef, exclude_self, ids, dists, counts, stats);
}

}  // extern "C"
