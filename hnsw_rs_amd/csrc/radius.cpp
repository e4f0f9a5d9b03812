// radius.cpp -- radius search (include/hnsw_mi355x.h, "radius search"): the cut of candidate lists at a radius on the
// device, and a search answered as everything within a distance, found by a ladder of searches of doubling n.  Host
// logic only; the cut is hx_filt_merge_kernel's fourth source form (search_filtered.hip), the candidate stage of every
// rung lists_host.h.

#include <algorithm>
#include <cstring>

#include "lists_host.h"

using hx::set_error;

static_assert(HX_RADIUS_MAX_N == HNSW_RADIUS_MAX_N, "the kernel's limit is the ABI's");
static_assert(HX_RADIUS_MORE == HNSW_RADIUS_MORE, "the kernel's flag is the ABI's");

namespace {

// one cut launch: lists of n_in entries into rows of n_out, for the queries of d_sel (nullptr: all)
int cut(uint64_t nq, uint32_t n_in, uint32_t n_out, const float *d_radius, const uint32_t *d_sel, uint32_t n_sel,
        const uint32_t *d_ids_in, const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in,
        uint32_t *d_ids, float *d_dists, uint32_t *d_counts, uint32_t *d_flags, hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::MergeLists m{};
    m.ids = d_ids_in;
    m.dists = d_dists_in;
    m.counts = d_counts_in;
    m.stats = d_stats_in;
    m.nq = (uint32_t)nq;
    m.pool = n_in;
    m.cut_out = n_out;
    m.radius = d_radius;
    m.flags = d_flags;
    return hx::launch_radius_cut(m, d_sel, n_sel, d_ids, d_dists, d_counts, d_stats, stream);
}

}  // namespace

extern "C" {

int hnsw_radius_cut_device(uint64_t nq, uint32_t n_in, uint32_t n_out, const float *d_radius, const uint32_t *d_sel,
                           uint64_t n_sel, const uint32_t *d_ids_in, const float *d_dists_in, const uint32_t *d_counts_in,
                           const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                           uint32_t *d_flags, hnsw_query_stats *d_stats, void *stream) {
    if (nq == 0) return HNSW_OK;
    if (n_in == 0 || n_in > n_out || n_out > HNSW_RADIUS_MAX_N) {
        set_error("radius cut: needs 1 <= n_in <= n_out <= %d", HNSW_RADIUS_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_nq("radius cut", nq)) return rc;
    if (!d_radius || !d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("radius cut: needs the radii, the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (d_sel && n_sel > nq) {
        set_error("radius cut: the selection names more queries than the call has");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("radius cut", "candidates'", d_stats_in, d_stats)) return rc;
    if (d_sel && n_sel == 0) return HNSW_OK;
    return cut(nq, n_in, n_out, d_radius, d_sel, (uint32_t)n_sel, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
               d_counts, d_flags, d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_radius(hnsw_index *h, const float *Q, uint64_t nq, const float *radius, uint32_t n_first,
                             uint32_t max_n, uint32_t ef, uint32_t *ids, float *dists, uint32_t *counts, uint32_t *flags,
                             uint32_t *rungs, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if (n_first == 0 || n_first > max_n || max_n > HNSW_RADIUS_MAX_N) {
        set_error("radius search: needs 1 <= n_first <= max_n <= %d", HNSW_RADIUS_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !radius || !ids || nq > 0x7FFFFFFFull) {
        set_error("radius search: needs queries, the radius of every query, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    for (uint64_t i = 0; i < nq; i++) {
        if (!(radius[i] >= 0.0f)) {  // (a NaN fails every compare)
            set_error("radius search: the radius of query %llu is negative or NaN", (unsigned long long)i);
            return HNSW_ERR_ARG;
        }
    }
    const bool host_form = h->del.count != 0;
    if (host_form && max_n > HX_FILT_MAX_N) {
        set_error("radius search: needs max_n <= %d while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    const uint64_t dim = v.dim;
    // device arena: [queries | selection | re-run selection | radii | rung block (laid out per rung, room for n = max_n) |
    // final block]; pinned arena: [flags or a rung's stats | final block]
    const hx::ResultBlock widest(nq, max_n);
    hx::ColumnBlock out;  // [ids | dists | counts | flags | stats]
    const size_t c_ids = out.add(nq * max_n * 4), c_dists = out.add(nq * max_n * 4), c_counts = out.add(nq * 4);
    const size_t c_flags = out.add(nq * 4), c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_sel = o_q + hx::align256(nq * dim * 4), o_resel = o_sel + hx::align256(nq * 4);
    const size_t o_rad = o_resel + hx::align256(nq * 4), o_rung = o_rad + hx::align256(nq * 4), o_out = o_rung + widest.bytes;
    const size_t p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin), *d_out = dv + o_out;
    float *d_Q = hx::at<float>(dv, o_q), *d_radius = hx::at<float>(dv, o_rad);
    uint32_t *d_sel = hx::at<uint32_t>(dv, o_sel), *d_flags = hx::at<uint32_t>(d_out, c_flags);
    const uint32_t *p_flags = reinterpret_cast<const uint32_t *>(hv);
    HIP_TRY(hipMemcpyAsync(d_radius, radius, nq * 4, hipMemcpyHostToDevice, sc.stream));
    if (!host_form && (rc = hx::queries_up(h, d_Q, Q, nq, sc.stream))) return rc;  // once, for every rung
    std::vector<uint32_t> sel(nq), next, h_rungs(nq, 0);
    for (uint64_t i = 0; i < nq; i++) sel[i] = (uint32_t)i;
    // the host form's lists of a rung: the selected queries' as searched, and every query's at its own index
    std::vector<float> q_sub;
    hx::HostLists sub, full;
    for (uint32_t k = 0;; k++) {
        const uint32_t n_k = (uint32_t)std::min<uint64_t>((uint64_t)n_first << k, max_n), ef_k = std::max(ef, n_k);
        const uint32_t n_sel = (uint32_t)sel.size();
        const bool all = n_sel == nq;  // (rung 0: no selection travels)
        const hx::ResultBlock rung(nq, n_k);
        const hx::ResultBlock::Ptrs in = rung.at(dv + o_rung);
        if (!all) HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), (size_t)n_sel * 4, hipMemcpyHostToDevice, sc.stream));
        if (host_form) {
            q_sub.resize((size_t)n_sel * dim);
            for (uint32_t b = 0; b < n_sel; b++) memcpy(&q_sub[(size_t)b * dim], Q + (size_t)sel[b] * dim, dim * 4);
            if ((rc = hx::host_candidates(h, q_sub.data(), n_sel, n_k, ef_k, {}, sub))) return rc;
            // (`full` outlives its copies: the stream is synchronised before the next rung)
            full.ids.assign((size_t)nq * n_k, UINT32_MAX), full.dists.assign((size_t)nq * n_k, 0.0f);
            full.counts.assign(nq, 0), full.stats.assign(nq, hnsw_query_stats{});
            for (uint32_t b = 0; b < n_sel; b++) {
                memcpy(&full.ids[(size_t)sel[b] * n_k], &sub.ids[(size_t)b * n_k], (size_t)n_k * 4);
                memcpy(&full.dists[(size_t)sel[b] * n_k], &sub.dists[(size_t)b * n_k], (size_t)n_k * 4);
                full.counts[sel[b]] = sub.counts[b];
                full.stats[sel[b]] = sub.stats[b];
            }
            rc = hx::upload(full, in, sc.stream, true);
        } else {
            // The rung block's layout changes with n_k: the stats of the queries outside the selection would be stale
            // bytes to the re-run loop, which scans all nq.  Cleared: their status reads HNSW_OK.
            if (!all) HIP_TRY(hipMemsetAsync(in.stats, 0, nq * sizeof(hnsw_query_stats), sc.stream));
            rc = hx::device_candidates(v, d_Q, nq, n_k, ef_k, all ? nullptr : d_sel, n_sel, in, hx::at<uint32_t>(dv, o_resel),
                                       sc.stream, hv);
        }
        if (rc != HNSW_OK) return rc;
        h->n_radius_rungs.fetch_add(1, std::memory_order_relaxed);
        rc = cut(nq, n_k, max_n, d_radius, all ? nullptr : d_sel, n_sel, in.ids, in.dists, in.counts, in.stats,
                 hx::at<uint32_t>(d_out, c_ids), hx::at<float>(d_out, c_dists), hx::at<uint32_t>(d_out, c_counts), d_flags,
                 hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
        if (rc != HNSW_OK) return rc;
        h->n_radius_launches.fetch_add(1, std::memory_order_relaxed);
        for (uint32_t q : sel) h_rungs[q] = k + 1;
        if (n_k == max_n) break;  // the flag stays: truncated at max_n
        // only the flag words come back; the next selection, ascending
        HIP_TRY(hipMemcpyAsync(hv, d_flags, nq * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(hipStreamSynchronize(sc.stream));
        next.clear();
        for (uint32_t q : sel)
            if (p_flags[q] & HNSW_RADIUS_MORE) next.push_back(q);
        if (next.empty()) break;
        sel.swap(next);
    }
    if (rungs) memcpy(rungs, h_rungs.data(), nq * 4);
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_radius_calls, {ids, dists, counts, flags, stats}, nq);
}

}  // extern "C"
