// from_rows.cpp -- search from stored rows (include/hnsw_mi355x.h, "search from stored rows"): query rows composed out
// of stored rows on the device, the sources taken back out of the result lists there, and a search answered from ids and
// weighted ids.  Host logic only; the compose is hx_distance_kernel's third source form (exact_scan.hip), the drop
// hx_filt_merge_kernel's fifth (search_filtered.hip).

#include <cstring>
#include <vector>

#include "handle.h"
#include "search_filtered.h"
#include "search_host.h"

using hx::set_error;

static_assert(HX_FROM_ROWS_MAX_TERMS == HNSW_FROM_ROWS_MAX_TERMS, "the compose form's lanes are the ABI's slot limit");
static_assert(HX_DROP_MAX_WIDTH == HNSW_FROM_ROWS_MAX_TERMS, "the drop form's lanes are the ABI's slot limit");
static_assert(HX_RADIUS_MAX_N == HNSW_DROP_MAX_N, "the drop form's list limit is the ABI's");

namespace {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

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
    if (!h) {
        set_error("compose rows: null handle");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if (int rc = check_width("compose rows", width)) return rc;
    if (nq > 0x7FFFFFFFull) {
        set_error("compose rows: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_src_ids || !d_Q) {
        set_error("compose rows: needs the source ids and the query rows");
        return HNSW_ERR_ARG;
    }
    int rc = hx::check_search_args(h, 0);  // (the rows are a search's queries: the handle has points and a complete build)
    if (rc != HNSW_OK || (rc = hx::ensure_uploaded(h))) return rc;
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
    if (nq > 0x7FFFFFFFull) {
        set_error("drop ids: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_ex || !d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("drop ids: needs the exclusion ids, the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if ((d_stats_in != nullptr) != (d_stats != nullptr)) {
        set_error("drop ids: the stats output goes with the candidates' stats, both or neither");
        return HNSW_ERR_ARG;
    }
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
    const uint64_t dim = h->dev.replica ? h->dev.view.dim : h->host->dim;
    // device arena: [source ids [nq][width] | weights | query rows [nq][dim] | candidate block (nq, n_cand) | result block
    // (nq, n)]; without the drop the search writes the result block itself.  The result block comes back in one copy.
    const hx::ResultBlock cand(nq, n_cand), out(nq, n);
    const size_t o_src = 0, o_w = o_src + hx::align256(nq * width * 4), o_q = o_w + hx::align256(nq * width * 4);
    const size_t o_cand = o_q + hx::align256(nq * dim * 4), o_out = exclude ? o_cand + cand.bytes : o_cand;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev);
    uint32_t *d_src = reinterpret_cast<uint32_t *>(dv + o_src);
    float *d_w = weights ? reinterpret_cast<float *>(dv + o_w) : nullptr, *d_Q = reinterpret_cast<float *>(dv + o_q);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand), o = out.at(dv + o_out);
    HIP_TRY(hipMemcpyAsync(d_src, src_ids, nq * width * 4, hipMemcpyHostToDevice, sc.stream));
    if (weights) HIP_TRY(hipMemcpyAsync(d_w, weights, nq * width * 4, hipMemcpyHostToDevice, sc.stream));
    if ((rc = compose(h, nq, width, d_src, d_w, d_Q, nullptr, sc.stream))) return rc;
    // The candidates.  While ids are deleted they are the HOST form's, over the composed rows copied back: only it lets
    // the planner choose the exact path, and the call is defined by it (as diverse.cpp)
    std::vector<float> h_Q, h_dists;
    std::vector<uint32_t> h_ids, h_counts;
    std::vector<hnsw_query_stats> h_stats;
    if (host_form) {
        h_Q.resize(nq * dim), h_ids.resize(nq * n_cand), h_dists.resize(nq * n_cand), h_counts.resize(nq), h_stats.resize(nq);
        HIP_TRY(hipMemcpyAsync(h_Q.data(), d_Q, nq * dim * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(hipStreamSynchronize(sc.stream));
        rc = hnsw_search_batch(h, h_Q.data(), nq, n_cand, ef, h_ids.data(), h_dists.data(), h_counts.data(), h_stats.data());
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
        // (the host vectors outlive the copies: the stream is synchronised below)
        HIP_TRY(hipMemcpyAsync(c.ids, h_ids.data(), nq * n_cand * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(c.dists, h_dists.data(), nq * n_cand * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(c.counts, h_counts.data(), nq * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(c.stats, h_stats.data(), nq * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, sc.stream));
    } else {  // as a caller of the device entry point would run it: launch, then _finish
        rc = hnsw_search_batch_device(h, d_Q, nq, n_cand, ef, c.ids, c.dists, c.counts, c.stats, sc.stream);
        if (rc != HNSW_OK) return rc;
        rc = hnsw_search_batch_device_finish(h, d_Q, nq, n_cand, ef, c.ids, c.dists, c.counts, c.stats, sc.stream);
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    if (exclude) {
        rc = drop(nq, n_cand, n, width, d_src, nullptr, c.ids, c.dists, c.counts, c.stats, o.ids, o.dists, o.counts, nullptr,
                  o.stats, sc.stream);
        if (rc != HNSW_OK) return rc;
        h->n_from_rows_drop.fetch_add(1, std::memory_order_relaxed);
    }
    HIP_TRY(hipMemcpyAsync(sc.pin, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_from_rows_calls.fetch_add(1, std::memory_order_relaxed);
    out.copy_out(sc.pin, ids, dists, counts, stats);
    const hnsw_query_stats *st = out.at(sc.pin).stats;
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return hx::query_status_error(i, st[i].status);
    return HNSW_OK;
}

int hnsw_search_batch_by_id(hnsw_index *h, const uint32_t *src_ids, uint64_t nq, uint32_t n, uint32_t ef, int exclude_self,
                            uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    return hnsw_search_batch_from_rows(h, src_ids, nullptr, nq, 1, n, ef, exclude_self, ids, dists, counts, stats);
}

}  // extern "C"
