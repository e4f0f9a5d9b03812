// filter_wide_host.cpp -- the orchestrator of hnsw_search_batch_filtered_wide: the host-pointer filtered search for
// n and ef' up to 1024 (search_filtered_wide.h).  It checks, plans with filter_host.cpp's planner
// (filter_plan.cpp: the same groups, the same choice of path from "filter_exact_max"), launches the wide graph kernel
// in chunks that keep the HBM level of the visited set within 1 GiB, runs the wide exact path group by group in chunks
// that keep the partial lists within 256 MiB, and ends in the re-run loop (rerun.h), whose one step here is path 2: the
// visited set has a second level instead of a larger table to try.

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "filter_plan.h"
#include "rerun.h"
#include "search_filtered_wide.h"

namespace hx {

namespace {

// The device arena of a call: [queries | row of every query | lo | hi | the graph path's selection | the exact path's
// selection | word offsets | admissible ids | partial keys | partial statuses | the HBM level of the visited set |
// result block].  The arena is the lease's: it stays with the handle between calls, the HBM level included.
struct WideArena {
    size_t o_q, o_mof, o_lo, o_hi, o_sel, o_xsel, o_wb, o_ids, o_part, o_pst, o_hbm, o_out;
    uint64_t part_rows;  // partial lists (n keys each) the exact path's room holds: the queries of a launch x its segments
    uint64_t gchunk;     // queries per launch of the graph kernel
    ResultBlock out;
    size_t bytes() const { return o_out + out.bytes; }
    // n_wb: word offsets in all; A_max: the longest list of admissible ids; x_queries: queries the exact path's room is
    // sized for; hbm_log2: 0 without a second level
    WideArena(uint64_t nq, uint32_t d, uint32_t n, bool rowed, bool ranged, size_t n_wb, uint64_t A_max, uint64_t x_queries,
              uint64_t n_graph, uint32_t hbm_log2)
        : out(nq, n) {
        const uint64_t nseg = wide_exact_segments(A_max), per_query = nseg * n * 8;
        const uint64_t xq = std::max<uint64_t>(1, std::min<uint64_t>({x_queries, 65535, HX_WIDE_PART_BYTES / per_query}));
        part_rows = xq * nseg;
        gchunk = hbm_log2 ? std::max<uint64_t>(1, std::min<uint64_t>(n_graph, HX_WIDE_HBM_BYTES >> (hbm_log2 + 2))) : n_graph;
        o_q = 0;
        o_mof = o_q + align256(nq * d * 4);
        o_lo = o_mof + (rowed ? align256(nq * 4) : 0);
        o_hi = o_lo + (ranged ? align256(nq * 4) : 0);
        o_sel = o_hi + (ranged ? align256(nq * 4) : 0);
        o_xsel = o_sel + align256(nq * 4);
        o_wb = o_xsel + align256(nq * 4);
        o_ids = o_wb + align256(n_wb * 4);
        o_part = o_ids + align256(A_max * 4);
        o_pst = o_part + align256(part_rows * n * 8);
        o_hbm = o_pst + align256(part_rows * 4);
        o_out = o_hbm + (hbm_log2 && n_graph ? align256((gchunk << hbm_log2) * 4) : 0);
    }
};

// The wide exact path for the g.nq queries of one group: those of d_sel, or the first g.nq of the call.  One compaction
// of the group's admissible ids (the kernel and the offsets of exact_group, filter_exact.cpp), then scan and merge, as
// many queries per launch as the partial lists' room takes
int wide_exact_group(const FilterSource &src, const Group &g, const uint32_t *d_sel, const WideArena &ar, unsigned char *dv,
                     hipStream_t stream) {
    const DevView &v = src.h->dev.view;
    const FilterArgs a = src.args(g);
    if (g.off.send) {
        HIP_TRY(hipMemcpyAsync(g.off.dev, g.off.host, g.off.n * 4, hipMemcpyHostToDevice, stream));
        src.count_compaction(g);
    }
    const RangeList ranges = src.range_list(g);
    uint32_t *d_ids = reinterpret_cast<uint32_t *>(dv + ar.o_ids);
    int r = launch_filter_compact(a, (a.allow_bits + 63) / 64, g.off.dev, d_ids, stream, &ranges);
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(65535, ar.part_rows / wide_exact_segments(g.A)));
    for (uint64_t c = 0; r == HNSW_OK && c < g.nq; c += chunk) {
        FilterArgs ac = a;
        if (d_sel) {
            ac.qsel = d_sel + c;
        } else {
            ac.qsel = nullptr;
            ac.Q += c * v.dim;
            ac.out_ids += c * a.n;
            ac.out_dists += c * a.n;
            ac.out_counts += c;
            ac.out_stats += c;
        }
        r = launch_filtered_wide_exact(v, ac, (uint32_t)std::min<uint64_t>(chunk, g.nq - c), d_ids, (uint32_t)g.A,
                                       reinterpret_cast<unsigned long long *>(dv + ar.o_part),
                                       reinterpret_cast<int32_t *>(dv + ar.o_pst), stream);
    }
    return r;
}

// (the re-run loop's launch: never reached, the loop starts at its largest table)
int no_larger_table(const DevView &, const FilterArgs &, uint32_t, uint32_t, hipStream_t) {
    set_error("wide filtered search: the visited set has no larger table");
    return HNSW_ERR_OVERFLOW;
}

}  // namespace

int search_filtered_wide(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f, uint32_t *ids,
                         float *dists, uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    // ---- check: everything outside the limits before any GPU work ----
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK || (rc = check_filter(f))) return rc;
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n == 0 || n > HX_WIDE_MAX_N || efp > HX_WIDE_MAX_EF || (f.lo == nullptr) != (f.hi == nullptr)) {
        set_error("wide filtered search: needs 1 <= n <= %d, ef' = max(ef, n) <= %d, and lo and hi together", HX_WIDE_MAX_N,
                  HX_WIDE_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if (!Q || !ids || nq > 0x7FFFFFFFull) {
        set_error("wide filtered search: needs queries, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    std::vector<hnsw_query_stats> local;
    if (!stats) {
        local.resize(nq);
        stats = local.data();
    }
    FilterSource src(h, f);
    if ((rc = src.check_rows(nq, f.allow_bits))) return rc;
    if (src.K) src.intern(nq);
    hnsw_mask_set *const set = src.set;
    const bool rowed = src.rowed, ranged = src.K != 0, multi = rowed || ranged;
    const uint32_t hbm_log2 = (uint32_t)h->filter_wide_hbm_log2;
    const uint32_t lds_log2 = h->filter_wide_lds_log2 ? (uint32_t)h->filter_wide_lds_log2 : wide_default_lds_log2(efp, hbm_log2);
    // ---- plan, per group, as search_filtered does: its admissible ids decide its queries' path ----
    std::vector<uint32_t> order;
    std::vector<Group> groups(1);
    groups[0].nq = nq;
    if (multi) {
        order.resize(nq);
        for (uint64_t i = 0; i < nq; i++) order[i] = (uint32_t)i;
        groups = group_by_key(order, src);
    }
    std::vector<uint32_t> wb_all;
    uint64_t A_max = 0, n_graph = 0, n_exact = 0;
    FilterSource::Locks lock = src.lock();
    for (Group &g : groups) {
        src.resolve(g, h->filter_exact_max, wb_all);
        g.d_list = nullptr;  // (a set's cached lists are the small kernels': every exact-path group is compacted here)
        A_max = std::max(A_max, g.A == UNCOUNTED ? g.A_ub : g.A);
        (g.exact ? n_exact : n_graph) += g.nq;
    }
    if (ranged) lock.lab.unlock();
    std::vector<uint32_t> gsel;
    std::vector<uint8_t> path(nq, groups[0].exact ? 1 : 0);
    if (multi) {
        for (const Group &g : groups)
            for (size_t i = g.q0; i < g.q0 + g.nq; i++) path[order[i]] = g.exact ? 1 : 0;
        if (n_graph && n_exact)
            for (uint64_t i = 0; i < nq; i++)
                if (!path[i]) gsel.push_back((uint32_t)i);
    }
    FilterArgs probe{};  // (the column and the deleted set go up as a range search's do; what they are is bound below)
    uint64_t unused = 0;
    if ((rc = ensure_uploaded(h)) || (rc = deleted_on_device(h, &probe.deny, &unused)) || (set && (rc = set->sync(h))) ||
        (ranged && (rc = labels_on_device(h, &probe.labels, &unused))))
        return rc;
    if (set) lock.set.unlock();
    const DevView &v = h->dev.view;
    // ---- lay out: a late group (a range planned on the graph path that reaches path 2) brings one more set of offsets ----
    const size_t wb_late_room = ranged ? ((src.len + 63) / 64 + 63) / 64 + 1 : 0;
    const WideArena ar(nq, v.dim, n, rowed, ranged, wb_all.size() + wb_late_room, A_max, n_exact ? nq : 16, n_graph, hbm_log2);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, ar.bytes(), ar.out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(s.dev);
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + ar.o_sel), *d_xsel = reinterpret_cast<uint32_t *>(dv + ar.o_xsel);
    uint32_t *d_mof = reinterpret_cast<uint32_t *>(dv + ar.o_mof), *d_lo = reinterpret_cast<uint32_t *>(dv + ar.o_lo),
             *d_hi = reinterpret_cast<uint32_t *>(dv + ar.o_hi), *d_wb = reinterpret_cast<uint32_t *>(dv + ar.o_wb);
    for (Group &g : groups)
        if (g.off.counted()) g.off.bind(wb_all.data(), d_wb + g.off.at, set != nullptr);
    // ---- upload ----
    HIP_TRY(hipMemcpyAsync(dv + ar.o_q, Q, nq * v.dim * 4, hipMemcpyHostToDevice, s.stream));
    if ((rc = cosine_queries(h, dv + ar.o_q, nq, s.stream))) return rc;
    if (!set && !wb_all.empty()) HIP_TRY(hipMemcpyAsync(d_wb, wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (ranged) {
        HIP_TRY(hipMemcpyAsync(d_lo, src.lo, nq * 4, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(d_hi, src.hi, nq * 4, hipMemcpyHostToDevice, s.stream));
    }
    if (rowed) HIP_TRY(hipMemcpyAsync(d_mof, src.mask_of, nq * 4, hipMemcpyHostToDevice, s.stream));
    if (!gsel.empty()) HIP_TRY(hipMemcpyAsync(d_sel, gsel.data(), gsel.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (multi && n_exact) HIP_TRY(hipMemcpyAsync(d_xsel, order.data(), nq * 4, hipMemcpyHostToDevice, s.stream));
    src.bind(reinterpret_cast<const float *>(dv + ar.o_q), set ? set->d_rows() : nullptr, rowed ? d_mof : nullptr,
             ranged ? d_lo : nullptr, ranged ? d_hi : nullptr, n, efp);
    FilterArgs &a = src.base;
    a.qsel = gsel.empty() ? nullptr : d_sel;
    ar.out.bind(a, dv + ar.o_out);
    const hnsw_query_stats *st = nullptr;
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        HIP_TRY(hipMemcpyAsync(s.pin, dv + ar.o_out, ar.out.bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        out = st = ar.out.at(s.pin).stats;
        return HNSW_OK;
    };
    // ---- launch: the graph path's queries of every group, a chunk at a time, each chunk's HBM level cleared on the
    // stream before its launch; then the exact path group by group ----
    WideVisited vis{hbm_log2 ? reinterpret_cast<uint32_t *>(dv + ar.o_hbm) : nullptr, lds_log2, hbm_log2, 0};
    for (uint64_t c = 0; c < n_graph; c += ar.gchunk) {
        const uint64_t cnt = std::min<uint64_t>(ar.gchunk, n_graph - c);
        if (vis.hbm) HIP_TRY(hipMemsetAsync(vis.hbm, 0xFF, (cnt << hbm_log2) * 4, s.stream));
        vis.q_base = (uint32_t)c;
        if ((rc = launch_filtered_wide_graph(v, a, (uint32_t)cnt, vis, s.stream))) return rc;
    }
    for (const Group &g : groups)
        if (g.exact && (rc = wide_exact_group(src, g, multi ? d_xsel + g.q0 : nullptr, ar, dv, s.stream))) return rc;
    // ---- path 2: the queries that filled both levels of their visited set, by the exact path, each under its own filter ----
    uint64_t n2 = 0;
    if (!n_graph) {
        if ((rc = fetch(st))) return rc;
    } else {
        rc = rerun_overflowed(
            v, no_larger_table, a, nq, 0, 0, d_sel, s.stream, fetch,
            [&](const std::vector<uint32_t> &sel) -> int {
                std::vector<uint32_t> sel2 = sel, wb_late;
                std::vector<Group> runs = group_by_key(sel2, src);
                for (uint32_t i : sel) path[i] = 2;
                FilterSource::Locks late;  // (a set's rows and the column's sorted copy, while a late group is counted)
                for (Group &g : runs) {
                    const Group &p = *std::lower_bound(groups.begin(), groups.end(), g, [](const Group &x, const Group &y) {
                        return group_before(x, y.key, y.list);
                    });
                    g.A = p.A, g.off = p.off;
                    if (g.off.counted()) continue;
                    if (!late.held()) late = src.lock();
                    src.resolve(g, INT64_MAX, wb_late);
                    g.d_list = nullptr;
                    g.off.late = true;
                }
                for (Group &g : runs)  // (wb_late is final; the one room is reused in stream order)
                    if (g.off.late) g.off.bind(wb_late.data(), d_wb + wb_all.size(), true);
                HIP_TRY(hipMemcpyAsync(d_sel, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, s.stream));
                for (const Group &g : runs)
                    if (int r = wide_exact_group(src, g, d_sel + g.q0, ar, dv, s.stream)) return r;
                return fetch(st);  // (synchronises: sel2 and wb_late live until then)
            },
            &n2);
        if (rc != HNSW_OK) return rc;
    }
    // ---- count ----
    h->n_wide_calls.fetch_add(1, std::memory_order_relaxed);
    h->n_wide_graph.fetch_add(n_graph - n2, std::memory_order_relaxed);
    h->n_wide_exact.fetch_add(n_exact, std::memory_order_relaxed);
    h->n_wide_overflow.fetch_add(n2, std::memory_order_relaxed);
    ar.out.copy_out(s.pin, ids, dists, counts, stats);
    if (paths) memcpy(paths, path.data(), nq);
    return first_query_error(stats, nq);
}

}  // namespace hx
