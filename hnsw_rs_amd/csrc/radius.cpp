// radius.cpp -- radius search (include/hnsw_mi355x.h, "radius search"): the cut of candidate lists at a radius on the
// device, and a search answered as everything within a distance, found by a ladder of searches of doubling n.  Host
// logic only; the cut is hx_filt_merge_kernel's fourth source form (search_filtered.hip).

#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"
#include "rerun.h"

using hx::set_error;

static_assert(HX_RADIUS_MAX_N == HNSW_RADIUS_MAX_N, "the kernel's limit is the ABI's");
static_assert(HX_RADIUS_MORE == HNSW_RADIUS_MORE, "the kernel's flag is the ABI's");

namespace {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

// The final block of nq queries x max_n: [ids | dists | counts | flags | stats], the same layout in the device arena and
// in pinned memory, so it comes back in ONE copy (as ResultBlock, search_host.h).
struct RadiusBlock {
    size_t ids = 0, dists, counts, flags, stats, bytes;
    RadiusBlock(uint64_t nq, uint32_t max_n) {
        dists = ids + hx::align256(nq * max_n * 4);
        counts = dists + hx::align256(nq * max_n * 4);
        flags = counts + hx::align256(nq * 4);
        stats = flags + hx::align256(nq * 4);
        bytes = stats + hx::align256(nq * sizeof(hnsw_query_stats));
    }
    template <class T>
    T *at(void *base, size_t off) const {
        return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off);
    }
};

// one cut launch: the lists of a rung [nq][n_in] into the final block's rows of max_n, for the queries of d_sel
// (nullptr: all)
int cut(hnsw_index *h, uint64_t nq, uint32_t n_in, uint32_t max_n, const float *d_radius, const uint32_t *d_sel,
        uint32_t n_sel, const hx::ResultBlock::Ptrs &in, const RadiusBlock &out, void *out_base, hipStream_t stream) {
    hx::MergeLists m{};
    m.ids = in.ids;
    m.dists = in.dists;
    m.counts = in.counts;
    m.stats = in.stats;
    m.nq = (uint32_t)nq;
    m.pool = n_in;
    m.cut_out = max_n;
    m.radius = d_radius;
    m.flags = out.at<uint32_t>(out_base, out.flags);
    if (int rc = hx::launch_radius_cut(m, d_sel, n_sel, out.at<uint32_t>(out_base, out.ids), out.at<float>(out_base, out.dists),
                                       out.at<uint32_t>(out_base, out.counts),
                                       out.at<hnsw_query_stats>(out_base, out.stats), stream))
        return rc;
    h->n_radius_launches.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
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
    if (nq > 0x7FFFFFFFull) {
        set_error("radius cut: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_radius || !d_ids_in || !d_dists_in || !d_ids || !d_dists) {
        set_error("radius cut: needs the radii, the candidates' ids and distances and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (d_sel && n_sel > nq) {
        set_error("radius cut: the selection names more queries than the call has");
        return HNSW_ERR_ARG;
    }
    if ((d_stats_in != nullptr) != (d_stats != nullptr)) {
        set_error("radius cut: the stats output goes with the candidates' stats, both or neither");
        return HNSW_ERR_ARG;
    }
    if (d_sel && n_sel == 0) return HNSW_OK;
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
    return hx::launch_radius_cut(m, d_sel, (uint32_t)n_sel, d_ids, d_dists, d_counts, d_stats, static_cast<hipStream_t>(stream));
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
    const RadiusBlock out(nq, max_n);
    const size_t o_q = 0, o_sel = o_q + hx::align256(nq * dim * 4), o_resel = o_sel + hx::align256(nq * 4);
    const size_t o_rad = o_resel + hx::align256(nq * 4), o_rung = o_rad + hx::align256(nq * 4), o_out = o_rung + widest.bytes;
    const size_t p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = reinterpret_cast<float *>(dv + o_q), *d_radius = reinterpret_cast<float *>(dv + o_rad);
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + o_sel), *d_resel = reinterpret_cast<uint32_t *>(dv + o_resel);
    const uint32_t *p_flags = reinterpret_cast<const uint32_t *>(hv);
    HIP_TRY(hipMemcpyAsync(d_radius, radius, nq * 4, hipMemcpyHostToDevice, sc.stream));
    if (!host_form) {  // Q goes up once; the unit-length copy of the cosine option is made once, from the caller's queries
        HIP_TRY(hipMemcpyAsync(d_Q, Q, nq * dim * 4, hipMemcpyHostToDevice, sc.stream));
        if ((rc = hx::cosine_queries(h, d_Q, nq, sc.stream))) return rc;
    }
    std::vector<uint32_t> sel(nq), next, h_rungs(nq, 0);
    for (uint64_t i = 0; i < nq; i++) sel[i] = (uint32_t)i;
    // the host form's lists of a rung, every selected query's at its own index
    std::vector<float> q_sub, l_dists, s_dists;
    std::vector<uint32_t> l_ids, l_counts, s_ids, s_counts;
    std::vector<hnsw_query_stats> l_stats, s_stats;
    for (uint32_t k = 0;; k++) {
        const uint32_t n_k = (uint32_t)std::min<uint64_t>((uint64_t)n_first << k, max_n), ef_k = std::max(ef, n_k);
        const uint32_t n_sel = (uint32_t)sel.size();
        const bool all = n_sel == nq;  // (rung 0: no selection travels)
        const hx::ResultBlock rung(nq, n_k);
        const hx::ResultBlock::Ptrs in = rung.at(dv + o_rung);
        if (!all) HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), (size_t)n_sel * 4, hipMemcpyHostToDevice, sc.stream));
        if (host_form) {
            // only the host form lets the planner choose the exact path, and the call is defined by it (as grouped.cpp)
            q_sub.resize((size_t)n_sel * dim);
            for (uint32_t b = 0; b < n_sel; b++) memcpy(&q_sub[(size_t)b * dim], Q + (size_t)sel[b] * dim, dim * 4);
            s_ids.resize((size_t)n_sel * n_k), s_dists.resize((size_t)n_sel * n_k), s_counts.resize(n_sel), s_stats.resize(n_sel);
            rc = hnsw_search_batch(h, q_sub.data(), n_sel, n_k, ef_k, s_ids.data(), s_dists.data(), s_counts.data(), s_stats.data());
            if (rc != HNSW_OK && !per_query_status(rc)) return rc;
            l_ids.assign((size_t)nq * n_k, UINT32_MAX), l_dists.assign((size_t)nq * n_k, 0.0f), l_counts.assign(nq, 0);
            l_stats.assign(nq, hnsw_query_stats{});
            for (uint32_t b = 0; b < n_sel; b++) {
                memcpy(&l_ids[(size_t)sel[b] * n_k], &s_ids[(size_t)b * n_k], (size_t)n_k * 4);
                memcpy(&l_dists[(size_t)sel[b] * n_k], &s_dists[(size_t)b * n_k], (size_t)n_k * 4);
                l_counts[sel[b]] = s_counts[b];
                l_stats[sel[b]] = s_stats[b];
            }
            HIP_TRY(hipMemcpyAsync(in.ids, l_ids.data(), (size_t)nq * n_k * 4, hipMemcpyHostToDevice, sc.stream));
            HIP_TRY(hipMemcpyAsync(in.dists, l_dists.data(), (size_t)nq * n_k * 4, hipMemcpyHostToDevice, sc.stream));
            HIP_TRY(hipMemcpyAsync(in.counts, l_counts.data(), nq * 4, hipMemcpyHostToDevice, sc.stream));
            HIP_TRY(hipMemcpyAsync(in.stats, l_stats.data(), nq * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, sc.stream));
        } else {
            // The rung block's layout changes with n_k: the stats of the queries outside the selection would be stale
            // bytes to the re-run loop, which scans all nq.  Cleared: their status reads HNSW_OK.
            if (!all) HIP_TRY(hipMemsetAsync(in.stats, 0, nq * sizeof(hnsw_query_stats), sc.stream));
            hx::SearchArgs a = hx::ann_args(v, d_Q, n_k, ef_k, in.ids, in.dists, in.counts, in.stats);
            a.qsel = all ? nullptr : d_sel;
            const uint32_t slots = hx::default_slots_log2(ef_k, v.S0);
            if ((rc = hx::launch_search(v, a, n_sel, slots, sc.stream))) return rc;
            rc = hx::rerun_overflowed(
                v, hx::launch_search, a, nq, slots, hx::max_slots_log2(ef_k), d_resel, sc.stream,
                [&](const hnsw_query_stats *&st) -> int {
                    HIP_TRY(hipMemcpyAsync(hv, in.stats, nq * sizeof(hnsw_query_stats), hipMemcpyDeviceToHost, sc.stream));
                    HIP_TRY(hipStreamSynchronize(sc.stream));
                    st = reinterpret_cast<const hnsw_query_stats *>(hv);
                    return HNSW_OK;
                },
                nullptr);
            if (rc != HNSW_OK) return rc;
        }
        h->n_radius_rungs.fetch_add(1, std::memory_order_relaxed);
        if ((rc = cut(h, nq, n_k, max_n, d_radius, all ? nullptr : d_sel, n_sel, in, out, dv + o_out, sc.stream))) return rc;
        for (uint32_t q : sel) h_rungs[q] = k + 1;
        if (n_k == max_n) break;  // the flag stays: truncated at max_n
        // only the flag words come back; the next selection, ascending (the host vectors above outlive their copies)
        HIP_TRY(hipMemcpyAsync(hv, out.at<uint32_t>(dv + o_out, out.flags), nq * 4, hipMemcpyDeviceToHost, sc.stream));
        HIP_TRY(hipStreamSynchronize(sc.stream));
        next.clear();
        for (uint32_t q : sel)
            if (p_flags[q] & HNSW_RADIUS_MORE) next.push_back(q);
        if (next.empty()) break;
        sel.swap(next);
    }
    HIP_TRY(hipMemcpyAsync(hv + p_out, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_radius_calls.fetch_add(1, std::memory_order_relaxed);
    memcpy(ids, out.at<uint32_t>(hv + p_out, out.ids), nq * max_n * 4);
    if (dists) memcpy(dists, out.at<float>(hv + p_out, out.dists), nq * max_n * 4);
    if (counts) memcpy(counts, out.at<uint32_t>(hv + p_out, out.counts), nq * 4);
    if (flags) memcpy(flags, out.at<uint32_t>(hv + p_out, out.flags), nq * 4);
    if (rungs) memcpy(rungs, h_rungs.data(), nq * 4);
    const hnsw_query_stats *st = out.at<hnsw_query_stats>(hv + p_out, out.stats);
    if (stats) memcpy(stats, st, nq * sizeof(hnsw_query_stats));
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return hx::query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // extern "C"
