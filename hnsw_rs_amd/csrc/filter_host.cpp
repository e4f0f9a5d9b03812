// filter_host.cpp -- the two orchestrators of filtered search: the host-pointer call (every hnsw_search_batch_filtered*,
// and the unfiltered entry points while ids are deleted) and the device-pointer call with its _finish.  Each checks,
// plans (filter_plan.cpp), launches the graph path once, runs the exact path (filter_exact.cpp) and ends in the re-run
// loop (rerun.h), whose last resort is path 2.

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "filter_exact.h"
#include "rerun.h"

namespace hx {

namespace {

// brings the deleted set's HBM copy up to date on the snapshot's device (on a stream of the handle's own, so that a
// caller's stream is not synchronised); a no-op while nothing is deleted
int sync_deleted(hnsw_index *h) {
    if (h->del.count == 0) return HNSW_OK;
    std::lock_guard<std::mutex> g(h->mu);
    // (a mark or unmark that changed no id still grows the host words to the index length: a copy they have outgrown is
    // made afresh even with no word listed, as the label column's is -- the kernels read deny_bits = all host words)
    if (h->del.current(h->dev.device) && h->del.words.size() <= h->del.d_cap) return HNSW_OK;
    ScratchLease lease(h);
    int rc = lease.prepare(h->dev.device, 0, 0);
    if (rc != HNSW_OK) return rc;
    return h->del.sync(h->dev.device, lease.s->stream);
}

// ... and the label column's, for a range search.  (A column no label was ever set in gets a copy too: the kernels
// take the pointer as "this call has a label range" and read nothing beyond label_len.)
int sync_labels(hnsw_index *h) {
    std::lock_guard<std::mutex> g(h->mu);
    {  // the mirror, and so the copy, covers every id of the index: the points inserted since have label 0
        std::lock_guard<std::mutex> lg(h->lab.mu);
        h->lab.cover(index_len(h));
    }
    if (h->lab.current(h->dev.device) && h->lab.n_words() <= h->lab.d_cap) return HNSW_OK;
    ScratchLease lease(h);
    int rc = lease.prepare(h->dev.device, 0, 0);
    if (rc != HNSW_OK) return rc;
    return h->lab.sync(h->dev.device, lease.s->stream);
}

// The device arena of a host-pointer call: [queries | masks | row of every query | lo | hi | selection | the exact
// path's selection | the exact path's scratch | result block]: the caller's masks when it brought any (all n_masks rows
// in one copy; a one-mask call sends the words below `bits` only; a set's rows are in HBM already), the rows with a row
// per query, lo and hi with ranges -- and then the word offsets have room for one more group, that of a path 2 group,
// counted when a query gets there.  The result block comes back in one copy to pinned memory: the caller's block, or
// the scratch's and from there to the caller's buffers
struct FilteredArena {
    size_t o_q, o_mask, o_mof, o_lo, o_hi, o_sel, o_xsel;
    ExactScratch x;
    size_t o_out;
    ResultBlock out;
    size_t bytes() const { return o_out + out.bytes; }
    // up_words: mask words the caller brought; rk: ranges per query (0: none); n_wbase, ids_grouped: ExactScratch's
    FilteredArena(uint64_t nq, uint32_t d, uint32_t n, uint64_t up_words, bool rowed, uint64_t rk, uint64_t A_max,
                  size_t n_wbase, uint64_t ids_grouped)
        : out(nq, n) {
        o_q = 0;
        o_mask = o_q + align256(nq * d * 4);
        o_mof = o_mask + align256(up_words * 8);
        o_lo = o_mof + (rowed ? align256(nq * 4) : 0);
        o_hi = o_lo + align256(nq * rk * 4);
        o_sel = o_hi + align256(nq * rk * 4);
        o_xsel = o_sel + align256(nq * 4);
        x = ExactScratch(o_xsel + align256(rowed || rk ? nq * 4 : 0), nq, n, A_max, n_wbase, ids_grouped);
        o_out = x.end;
    }
};

}  // namespace

int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f,
                    bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                    uint8_t *paths, void *pin_block, bool grouped) {
    // ---- check ----
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK || (rc = check_filter(f))) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || (!ids && !pin_block) || nq > 0x7FFFFFFFull || n > HX_FILT_MAX_N) {
        set_error("filtered search: needs queries, an id buffer, a mask when allow_bits > 0 and n <= %d",
                  HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    // (the entry points see to lo and hi with K, and to mask_of with rows per query)
    FilterSource src(h, f);
    if ((rc = src.check_rows(nq, f.allow_bits))) return rc;
    if (n == 0) {  // nothing returned, nothing launched
        if (counts) memset(counts, 0, nq * 4);
        return HNSW_OK;
    }
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (src.K) src.intern(nq);
    hnsw_mask_set *const set = src.set;
    // The two facts the layout, the uploads and the kernels' arguments follow from: the call has a row per query; it has
    // a label column, with rk ranges per query.  With neither it has one group and no use for an order of its queries
    const bool rowed = src.rowed, ranged = src.K != 0, multi = rowed || ranged;
    const uint64_t rk = ranged ? src.K : 1, bits = src.bits;
    // ---- plan, per group: its admissible ids decide its queries' path.  A set stays locked until its HBM copy
    // is up to date and the lists this call needs are made; the label column only while the ranges are counted ----
    std::vector<uint32_t> order;  // the queries, group by group; a one-mask call has one group and no use for it
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
        src.resolve(g, exact_only ? INT64_MAX : h->filter_exact_max, wb_all);
        A_max = std::max(A_max, g.A == UNCOUNTED ? g.A_ub : g.A);  // (the scratch of a path 2 group is sized by it)
        (g.exact ? n_exact : n_graph) += g.nq;
    }
    if (ranged) lock.lab.unlock();
    if (n_graph && efp > HX_FILT_MAX_EF) {
        set_error("filtered search: ef' = max(ef, n) = %u is above the graph path's maximum of %d", efp, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    // the selections: the graph path's queries in one list (none when every query takes it), the exact path's group by
    // group (order itself when every query takes it)
    std::vector<uint32_t> gsel;
    std::vector<uint8_t> path(nq, groups[0].exact ? 1 : 0);
    if (multi) {
        for (const Group &g : groups)
            for (size_t i = g.q0; i < g.q0 + g.nq; i++) path[order[i]] = g.exact ? 1 : 0;
        if (n_graph && n_exact) {
            for (uint64_t i = 0; i < nq; i++)
                if (!path[i]) gsel.push_back((uint32_t)i);
        }
    }
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h)) || (set && (rc = set->sync(h))) ||
        (ranged && (rc = sync_labels(h))))
        return rc;
    const DevView &v = h->dev.view;
    // ---- lay out ----
    // The grouped form of the exact path (exact_grouped): the lists of a pass's groups lie one behind the other, so the
    // ids' room is that of the planned pass, and of a path 2 pass up to 4 Mi ids (one that needs more is cut); the late
    // offsets of a path 2 pass lie one behind the other as well, a group's worth for every group not counted yet
    const bool grouping = multi && groups.size() > 1 && (grouped || h->filter_exact_grouped);
    uint64_t ids_grouped = 0, ids_late = 0, n_late = 0, n_exact_groups = 0;
    for (const Group &g : groups) {
        if (g.exact) ids_grouped += g.A, n_exact_groups++;
        if (!g.exact) ids_late += g.A == UNCOUNTED ? g.A_ub : g.A;
        if (!g.off.counted()) n_late++;
    }
    ids_grouped = grouping ? std::max<uint64_t>({ids_grouped, std::min<uint64_t>(ids_late, 4u << 20), 1}) : 0;
    const size_t wb_lazy = ranged ? std::max<uint64_t>(1, ((src.len + 63) / 64 + 63) / 64) * (grouping ? std::max<uint64_t>(1, n_late) : 1) : 0;
    const uint64_t up_words = !src.masks ? 0 : rowed ? (uint64_t)src.n_masks * src.row_words : (bits + 63) / 64;
    const FilteredArena ar(nq, v.dim, n, up_words, rowed, ranged ? rk : 0, A_max, wb_all.size() + wb_lazy, ids_grouped);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, ar.bytes(), pin_block ? 0 : ar.out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(s.dev);
    void *hv = pin_block ? pin_block : s.pin;
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + ar.o_sel), *d_xsel = reinterpret_cast<uint32_t *>(dv + ar.o_xsel);
    uint32_t *d_mof = reinterpret_cast<uint32_t *>(dv + ar.o_mof), *d_lo = reinterpret_cast<uint32_t *>(dv + ar.o_lo),
             *d_hi = reinterpret_cast<uint32_t *>(dv + ar.o_hi);
    const ExactPlace at{dv, ar.x, s.stream};
    // (the planner's list is final: under a set the word offsets of a group go up only when a compaction of it runs)
    for (Group &g : groups)
        if (g.off.counted()) g.off.bind(wb_all.data(), ar.x.d_wb(dv) + g.off.at, set != nullptr);
    // ---- upload ----
    HIP_TRY(hipMemcpyAsync(dv + ar.o_q, Q, nq * v.dim * 4, hipMemcpyHostToDevice, s.stream));
    if ((rc = cosine_queries(h, dv + ar.o_q, nq, s.stream))) return rc;
    if (up_words) HIP_TRY(hipMemcpyAsync(dv + ar.o_mask, src.masks, up_words * 8, hipMemcpyHostToDevice, s.stream));
    if (!set && (bits || multi) && !wb_all.empty())
        HIP_TRY(hipMemcpyAsync(ar.x.d_wb(dv), wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (ranged) {
        HIP_TRY(hipMemcpyAsync(d_lo, src.lo, nq * rk * 4, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(d_hi, src.hi, nq * rk * 4, hipMemcpyHostToDevice, s.stream));
    }
    if (rowed) HIP_TRY(hipMemcpyAsync(d_mof, src.mask_of, nq * 4, hipMemcpyHostToDevice, s.stream));
    if (!gsel.empty()) HIP_TRY(hipMemcpyAsync(d_sel, gsel.data(), gsel.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (multi && n_exact) HIP_TRY(hipMemcpyAsync(d_xsel, order.data(), nq * 4, hipMemcpyHostToDevice, s.stream));
    src.bind(reinterpret_cast<const float *>(dv + ar.o_q),
             set ? set->d_rows() : up_words ? reinterpret_cast<const uint64_t *>(dv + ar.o_mask) : nullptr,
             rowed ? d_mof : nullptr, ranged ? d_lo : nullptr, ranged ? d_hi : nullptr, n, efp);
    FilterArgs &a = src.base;
    a.qsel = gsel.empty() ? nullptr : d_sel;
    ar.out.bind(a, dv + ar.o_out);
    if (set) {
        // the lists of the rows planned on the exact path: a valid one is used as it is, the others are compacted
        // into the set (while its budget lasts) here, once, for this call and the ones after it
        const uint64_t budget = h->mask_set_cache_mb > 0 ? (uint64_t)h->mask_set_cache_mb << 20 : 0;
        std::vector<hnsw_mask_set::Row *> made;
        for (Group &g : groups) {
            if (!src.has_words(g.key) || src.ranged(g)) continue;  // (a row AND a range: compacted in the scratch, not the row's list)
            hnsw_mask_set::Row &r = set->rows[(size_t)g.key];
            if (!r.list_valid && g.exact && set->reserve_list(r, budget)) {
                HIP_TRY(hipMemcpyAsync(g.off.dev, g.off.host, g.off.n * 4, hipMemcpyHostToDevice, s.stream));
                if ((rc = launch_filter_compact(src.args(g), (bits + 63) / 64, g.off.dev, r.d_ids, s.stream))) return rc;
                src.count_compaction(g);
                made.push_back(&r);
            }
            g.d_list = r.list_valid || (!made.empty() && made.back() == &r) ? r.d_ids : nullptr;
        }
        if (!made.empty()) {  // (searches on other streams read the lists next)
            HIP_TRY(hipStreamSynchronize(s.stream));
            for (hnsw_mask_set::Row *r : made) r->list_valid = true;
        }
        lock.set.unlock();
    }
    auto fetch = [&](const hnsw_query_stats *&st) -> int {
        HIP_TRY(hipMemcpyAsync(hv, dv + ar.o_out, ar.out.bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        st = ar.out.at(hv).stats;
        return HNSW_OK;
    };
    // ---- launch: ONE launch of the graph path for the queries of every group planned on it, then the exact path group
    // by group (its scratch reused in stream order), then the result block in one copy ----
    const uint32_t range_lds = filt_range_lds(ranged, (uint32_t)rk);
    const uint32_t slots = filt_first_slots_log2(v, efp, range_lds);
    if (n_graph && (rc = launch_filtered_graph(v, a, (uint32_t)n_graph, slots, s.stream))) return rc;
    std::vector<std::vector<unsigned char>> keep;  // (the tables of the grouped passes, until the fetch has synchronised)
    if (grouping && n_exact_groups > 1) {
        std::vector<PassItem> items;
        for (const Group &g : groups)
            if (g.exact) items.push_back({g, order.data() + g.q0, d_xsel + g.q0});
        if ((rc = exact_grouped(src, items, at, keep))) return rc;
    } else {
        for (const Group &g : groups)
            if (g.exact && (rc = exact_group(src, g, multi ? d_xsel + g.q0 : nullptr, g.nq, at))) return rc;
    }
    // ---- re-run ----
    uint64_t n2 = 0;
    const hnsw_query_stats *st;
    if (!n_graph) {
        if ((rc = fetch(st))) return rc;
    } else {
        // queries whose visited table filled up run again with a table twice the size, all groups together, and those
        // that fill the largest one take path 2: in this arena, its late offsets behind the planner's
        rc = rerun_overflowed(
            v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v, range_lds), d_sel, s.stream, fetch,
            [&](const std::vector<uint32_t> &sel) -> int {
                return path2(
                    src, sel, path, &groups, multi ? 0 : nq, grouping,
                    [&](const Path2Need &, Path2Place &p) {
                        p = {at, d_sel, ar.x.d_wb(dv) + wb_all.size()};
                        return (int)HNSW_OK;
                    },
                    [&] { return fetch(st); });
            },
            &n2);
        if (rc != HNSW_OK) return rc;
    }
    // ---- count ----
    count_call(h, src.family, n_graph - n2, n_exact, n2, groups.size());
    if (!pin_block) ar.out.copy_out(hv, ids, dists, counts, stats);
    if (paths) memcpy(paths, path.data(), nq);
    return HNSW_OK;
}

int labels_on_device(hnsw_index *h, const uint32_t **d_labels, uint64_t *label_len) {
    if (int rc = sync_labels(h)) return rc;
    FilterArgs a{};
    bind_labels(h, a);
    *d_labels = a.labels;
    *label_len = a.label_len;
    return HNSW_OK;
}

int deleted_on_device(hnsw_index *h, const uint64_t **d_deny, uint64_t *deny_bits) {
    if (int rc = sync_deleted(h)) return rc;
    *d_deny = h->del.count ? h->del.d_words : nullptr;
    *deny_bits = h->del.count ? h->del.deny_bits() : 0;
    return HNSW_OK;
}

int search_filtered_checked(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f,
                            bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                            uint8_t *paths) {
    std::vector<hnsw_query_stats> local;
    if (!stats && nq <= 0x7FFFFFFFull) {  // (more queries are refused below, before anything is allocated for them)
        local.resize(nq);
        stats = local.data();
    }
    int rc = search_filtered(h, Q, nq, n, ef, f, exact_only, ids, dists, counts, stats, paths);
    if (rc != HNSW_OK || n == 0) return rc;
    return first_query_error(stats, nq);
}

int search_device_filtered(hnsw_index *h, const Filter &f, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                           uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                           hipStream_t stream, bool finish, uint8_t *paths) {
    int rc = check_filter(f);
    if (rc != HNSW_OK) return rc;
    hnsw_mask_set *const set = f.rows == Filter::SET ? f.set : nullptr;
    const bool ranged = f.K != 0, keyed = f.mask_of || ranged;  // keyed: the queries name rows or ranges the host has not seen
    const uint64_t rk = ranged ? f.K : 1;                       // ranges per query
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n > HX_FILT_MAX_N || efp > HX_FILT_MAX_EF) {
        set_error("%s: needs n <= %d and ef' = max(ef, n) <= %d",
                  f.family == Filter::DELETED ? "search with deleted ids" : "filtered device search", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if (set && !f.mask_of && set->n_masks == 0) {
        set_error("filtered device search: every query names row 0 of a set without rows");
        return HNSW_ERR_ARG;
    }
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h)) || (ranged && (rc = sync_labels(h)))) return rc;
    if (set) {
        std::lock_guard<std::mutex> g(set->mu);
        if ((rc = set->sync(h))) return rc;
    }
    const DevView &v = h->dev.view;
    DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    StreamTmp t_dists, t_counts;  // the kernels write distances and counts: stand-ins for the optional outputs
    if (!d_dists && (rc = t_dists.alloc(nq * n * 4, stream))) return rc;
    if (!d_counts && (rc = t_counts.alloc(nq * 4, stream))) return rc;
    if (!d_dists) d_dists = static_cast<float *>(t_dists.p);
    if (!d_counts) d_counts = static_cast<uint32_t *>(t_counts.p);
    FilterSource src(h, f);
    src.bind(dq.q, set ? set->d_rows() : nullptr, f.mask_of, f.lo, f.hi, n, efp);
    FilterArgs &a = src.base;
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    const uint32_t range_lds = filt_range_lds(ranged, (uint32_t)rk);
    const uint32_t slots = filt_first_slots_log2(v, efp, range_lds);
    if (!finish) return launch_filtered_graph(v, a, (uint32_t)nq, slots, stream);

    // scratch: the selection on the device; the statuses and the keys of the queries (the rows and ranges they name:
    // [rows | lo | hi]) on the host; the exact path's part ([selection | its scratch]) is sized only when a query reaches it
    const size_t st_bytes = nq * sizeof(hnsw_query_stats), o_keys = align256(st_bytes), r_bytes = align256(nq * rk * 4);
    const size_t pin_bytes = keyed ? o_keys + 3 * r_bytes : st_bytes;
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), pin_bytes))) return rc;
    const hnsw_query_stats *st = nullptr;
    bool have_keys = false;  // they come back once, with the first fetch
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        unsigned char *pin = static_cast<unsigned char *>(lease.s->pin);
        uint32_t *k0 = reinterpret_cast<uint32_t *>(pin + o_keys), *k1 = reinterpret_cast<uint32_t *>(pin + o_keys + r_bytes),
                 *k2 = reinterpret_cast<uint32_t *>(pin + o_keys + 2 * r_bytes);
        HIP_TRY(hipMemcpyAsync(pin, d_stats, st_bytes, hipMemcpyDeviceToHost, stream));
        if (f.mask_of && !have_keys) HIP_TRY(hipMemcpyAsync(k0, f.mask_of, nq * 4, hipMemcpyDeviceToHost, stream));
        if (ranged && !have_keys) {
            HIP_TRY(hipMemcpyAsync(k1, f.lo, nq * rk * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(k2, f.hi, nq * rk * 4, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        out = st = reinterpret_cast<const hnsw_query_stats *>(pin);
        if (f.mask_of) src.mask_of = k0;
        if (ranged) src.lo = k1, src.hi = k2;
        // (the ranges are seen here for the first time.  Without a row per query their table is also the count of the
        // call's groups and is made now; with one the groups are counted from the pairs, and the table waits for path 2)
        if (ranged && !f.mask_of && !have_keys) src.intern(nq);
        have_keys = true;
        return HNSW_OK;
    };
    std::vector<uint8_t> path(nq, 0);
    uint64_t n2 = 0;
    rc = rerun_overflowed(
        v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v, range_lds), static_cast<uint32_t *>(lease.s->dev), stream,
        fetch,
        [&](const std::vector<uint32_t> &sel) -> int {
            // (a query that names no row of the set ended with HNSW_ERR_ARG, not with an overflow: every row here exists)
            if (ranged && !src.interned()) src.intern(nq);
            return path2(
                src, sel, path, nullptr, 0, h->filter_exact_grouped != 0,
                [&](const Path2Need &need, Path2Place &p) {  // [selection | exact scratch], in the lease, only now
                    p.at = {nullptr,
                            ExactScratch(align256(need.nsel * 4), need.nsel, n, need.A_max, need.grouping ? need.n_wb_late : need.n_wb,
                                         need.grouping ? std::max<uint64_t>(need.A_sum, 1) : 0),
                            stream};
                    int r = lease.prepare(h->dev.device, p.at.x.end, pin_bytes);
                    if (r != HNSW_OK) return r;
                    p.at.dv = static_cast<unsigned char *>(lease.s->dev);
                    p.d_sel = reinterpret_cast<uint32_t *>(p.at.dv);
                    p.d_late = p.at.x.d_wb(p.at.dv);
                    return (int)HNSW_OK;
                },
                [&] {
                    const hnsw_query_stats *unused;
                    return fetch(unused);
                });
        },
        &n2);
    if (rc != HNSW_OK) return rc;
    count_call(h, src.family, nq - n2, 0, n2, ranged ? src.n_groups(nq) : 0);
    if (paths) memcpy(paths, path.data(), nq);
    for (uint64_t i = 0; i < nq; i++)
        if (set && st[i].status == HNSW_ERR_ARG) {  // (the kernel's check of d_mask_of)
            set_error("filtered device search: query %llu names mask %u of %u", (unsigned long long)i,
                      (uint32_t)src.key((uint32_t)i), set->n_masks);
            return HNSW_ERR_ARG;
        } else if (st[i].status != HNSW_OK) {
            return query_status_error(i, st[i].status);
        }
    return HNSW_OK;
}

}  // namespace hx
