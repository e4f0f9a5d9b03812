// search_host.cpp -- the host side of the search entry points: the host-pointer path, the filtered / deleted
// orchestration and the completion of a device-pointer call, around one re-run loop.  Host logic only; the kernels
// are search_kernels.hip, search_lean.hip and search_filtered.hip.

#include "search_host.h"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace hx {

namespace {

// ---- the re-run loop ---------------------------------------------------------------------------------------------
// A query whose visited table filled up ends with status HNSW_ERR_OVERFLOW and is run again with a table twice the
// size, until none is left or the largest table is reached.  The first launch is the caller's (perhaps in an earlier
// call); what differs from site to site comes in as
//   launch, a:   launch_search or launch_filtered_graph and its arguments (a.qsel is set to the selection);
//   fetch(st):   bring the statuses (or the whole result block) of everything launched so far back to the host,
//                synchronise, and say where they are;
//   exhausted(sel):  answer the queries that filled the largest table some other way and fetch again -- or nullptr:
//                their status stays HNSW_ERR_OVERFLOW for the caller to report.
// d_sel holds the selection on the device (room for nq ids).  n_exhausted = queries handed to `exhausted`.
template <class Args, class Fetch, class Exhausted>
int rerun_overflowed(const DevView &v, int (*launch)(const DevView &, const Args &, uint32_t, uint32_t, hipStream_t), Args &a,
                     uint64_t nq, uint32_t slots, uint32_t max_slots, uint32_t *d_sel, hipStream_t stream, Fetch fetch,
                     Exhausted exhausted, uint64_t *n_exhausted = nullptr) {
    std::vector<uint32_t> sel;
    while (true) {
        const hnsw_query_stats *st = nullptr;
        int rc = fetch(st);
        if (rc != HNSW_OK) return rc;
        sel.clear();
        for (uint64_t i = 0; i < nq; i++)
            if (st[i].status == HNSW_ERR_OVERFLOW) sel.push_back((uint32_t)i);
        if (sel.empty()) return HNSW_OK;
        if (slots >= max_slots) {
            if constexpr (std::is_same_v<Exhausted, std::nullptr_t>) {
                return HNSW_OK;
            } else {
                if (n_exhausted) *n_exhausted = sel.size();
                return exhausted(sel);
            }
        }
        HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // `sel` is reused by the next round
        a.qsel = d_sel;
        if ((rc = launch(v, a, (uint32_t)sel.size(), ++slots, stream))) return rc;
    }
}

// first per-query failure of a call, with its text
int first_query_error(const hnsw_query_stats *st, uint64_t nq) {
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // namespace

// ---- the host-pointer search path --------------------------------------------------------------------------
HostSearchPlan plan_host_search(uint64_t nq, uint32_t d, uint32_t n, uint32_t n_entry) {
    HostSearchPlan p{};
    p.o_q = 0;
    p.o_sel = p.o_q + align256(nq * d * 4);
    p.o_ent = p.o_sel + align256(nq * 4);
    p.o_out = p.o_ent + align256((size_t)n_entry * 4);
    p.out = ResultBlock(nq, n);
    p.dev_bytes = p.o_out + p.out.bytes;
    p.p_q = 0;
    p.p_out = align256(nq * d * 4);
    p.pin_bytes = p.p_out + p.out.bytes;
    return p;
}

SearchArgs ann_args(const DevView &v, const float *dQ, uint32_t n, uint32_t ef, uint32_t *ids, float *dists,
                    uint32_t *counts, hnsw_query_stats *stats) {
    SearchArgs a{};
    a.Q = dQ;
    a.qsel = nullptr;
    a.entries = nullptr;
    a.n_entry = 1;
    a.layer_hi = (int32_t)v.nb_layers - 1;  // template.rs:322-326: layers L-1..1 with ef = 1,
    a.layer_lo = 0;                         // then layer 0 with ef
    a.ef_upper = 1;
    a.ef_bottom = ef;
    a.n = n;
    a.out_ids = ids;
    a.out_dists = dists;
    a.out_counts = counts;
    a.out_stats = stats;
    return a;
}

int query_status_error(uint64_t i, int32_t status) {
    switch (status) {
        case HNSW_OK:
            break;
        case HNSW_ERR_NAN_INPUT:
            set_error("query %llu: NaN in the query or in a distance", (unsigned long long)i);
            break;
        case HNSW_ERR_NODE_NOT_IN_GRAPH:
            set_error("Error in search_layer: node not in Graph (query %llu)", (unsigned long long)i);
            break;
        case HNSW_ERR_OVERFLOW:
            set_error("query %llu: visited table exhausted at its largest size", (unsigned long long)i);
            break;
        default:
            set_error("query %llu failed with status %d", (unsigned long long)i, status);
    }
    return status;
}

int search_staged(hnsw_index *h, SearchScratch &s, const HostSearchPlan &p, SearchArgs a_host, uint64_t nq,
                  const uint32_t *entries, const float *Q_user) {
    const DevView &v = h->dev.view;
    unsigned char *dv = static_cast<unsigned char *>(s.dev), *hv = static_cast<unsigned char *>(s.pin);
    int rc;
    // Small calls skip both copies: pinned host memory is mapped into the device's address space, the kernel reads
    // each query once (400 B per wave over the link) and writes its few result words straight into the pinned
    // result block.  Measured on the 1M x 100d index: a lone 1024-query call 225 us against 232 us with the copies, but
    // 2 / 3 concurrent 1024-query callers 5.2 / 7.5 M q/s against 5.9 / 8.0 M (the copy engines overlap with the other
    // caller's kernel, reads over the link from a busy kernel do not) -- so calls of up to 512 queries (every coalesced
    // batch of up to 512 callers) go without copies, larger ones, and calls whose queries are normalised on the
    // device first (the cosine option), keep them.
    static const bool zc_allowed = !(getenv("HNSW_MI355X_ZERO_COPY") && atoi(getenv("HNSW_MI355X_ZERO_COPY")) == 0);
    static const uint64_t zc_max = getenv("HNSW_MI355X_ZERO_COPY_MAX") ? strtoull(getenv("HNSW_MI355X_ZERO_COPY_MAX"), nullptr, 0) : 512;
    const bool zc = zc_allowed && !Q_user && !h->cosine && nq <= zc_max;
    SearchArgs a = a_host;
    if (zc) {
        a.Q = reinterpret_cast<const float *>(hv + p.p_q);
    } else {
        HIP_TRY(hipMemcpyAsync(dv + p.o_q, Q_user ? (const void *)Q_user : (const void *)(hv + p.p_q), nq * v.dim * 4,
                               hipMemcpyHostToDevice, s.stream));
        if ((rc = cosine_queries(h, dv + p.o_q, nq, s.stream))) return rc;
        a.Q = reinterpret_cast<const float *>(dv + p.o_q);
    }
    p.out.bind(a, zc ? hv + p.p_out : dv + p.o_out);  // where the kernel writes the result block
    if (entries) {
        HIP_TRY(hipMemcpyAsync(dv + p.o_ent, entries, (size_t)a.n_entry * 4, hipMemcpyHostToDevice, s.stream));
        a.entries = reinterpret_cast<const uint32_t *>(dv + p.o_ent);
    }
    const uint32_t ef_max = std::max(a.ef_bottom, a.ef_upper);
    const uint32_t slots = default_slots_log2(ef_max, v.S0);
    if ((rc = launch_search(v, a, (uint32_t)nq, slots, s.stream))) return rc;
    return rerun_overflowed(
        v, launch_search, a, nq, slots, max_slots_log2(ef_max), reinterpret_cast<uint32_t *>(dv + p.o_sel), s.stream,
        [&](const hnsw_query_stats *&st) -> int {
            if (!zc) HIP_TRY(hipMemcpyAsync(hv + p.p_out, dv + p.o_out, p.out.bytes, hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
            st = p.out.at(hv + p.p_out).stats;
            return HNSW_OK;
        },
        nullptr);
}

int search_host(hnsw_index *h, SearchArgs a_host, const float *Q, uint64_t nq, uint32_t *ids, float *dists,
                uint32_t *counts, hnsw_query_stats *stats, const uint32_t *entries) {
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const uint32_t d = h->dev.view.dim;
    HostSearchPlan p = plan_host_search(nq, d, a_host.n, entries ? a_host.n_entry : 0);
    // queries go through the pinned arena up to 8 MiB (a batch of 1024 x 100d is 400 KB); beyond that the
    // runtime's own pageable staging serves, and the pinned arena holds the result block only
    const bool stage_q = nq * (size_t)d * 4 <= (8u << 20);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, p.dev_bytes, stage_q ? p.pin_bytes : p.out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    if (!stage_q) p.p_out = 0;
    unsigned char *hv = static_cast<unsigned char *>(s.pin);
    if (stage_q) memcpy(hv + p.p_q, Q, nq * (size_t)d * 4);
    if ((rc = search_staged(h, s, p, a_host, nq, entries, stage_q ? nullptr : Q))) return rc;
    p.out.copy_out(hv + p.p_out, ids, dists, counts, stats);
    return first_query_error(p.out.at(hv + p.p_out).stats, nq);
}

// ---- filtered search, and the unfiltered entry points while ids are deleted --------------------------------------
uint64_t count_admissible(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase) {
    const uint64_t n_words = (bits + 63) / 64, n_wblk = (n_words + 63) / 64;
    const std::vector<uint64_t> &deny = h->del.words;
    const bool denies = h->del.count > 0;
    wbase.assign(std::max<uint64_t>(1, n_wblk), 0);
    uint64_t A = 0;
    for (uint64_t w = 0; w < n_words; w++) {
        if (w % 64 == 0) wbase[w / 64] = (uint32_t)A;
        uint64_t x = allow ? allow[w] : ~0ull;
        if (w == n_words - 1 && bits % 64) x &= (1ull << (bits % 64)) - 1;
        if (denies && w < deny.size()) x &= ~deny[w];
        A += (uint64_t)__builtin_popcountll(x);
    }
    return A;
}

namespace {

// brings the deleted set's HBM copy up to date on the snapshot's device (on a stream of the handle's own, so that a
// caller's stream is not synchronised); a no-op while nothing is deleted
int sync_deleted(hnsw_index *h) {
    if (h->del.count == 0) return HNSW_OK;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->del.d_words && h->del.d_device == h->dev.device && h->del.dirty.empty()) return HNSW_OK;
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

// the column as the kernels see it (after sync_labels: at least the index length; never more than the copy holds)
void bind_labels(const hnsw_index *h, FilterArgs &a) {
    a.labels = h->lab.d_labels();
    a.label_len = std::min<uint64_t>(h->lab.labels.size(), 2 * h->lab.d_cap);
}

// The exact path's scratch from `base` in a device arena: [word offsets | admissible ids | partial keys | partial
// statuses], for launches of up to nsel_max queries over up to A_max admissible ids (n_wbase word offsets in all)
struct ExactScratch {
    size_t o_wb, o_ids, o_part, o_pst, end;
    ExactScratch(size_t base, uint64_t nsel_max, uint32_t n, uint64_t A_max, size_t n_wbase) {
        // chunk x nseg of any launch within those limits (filt_exact_segments: at most 256 segments, and at most
        // 262144 blocks unless the queries alone are more)
        const uint64_t N = std::min<uint64_t>(nsel_max, 65535), s = filt_exact_segments(A_max, 1);
        const uint64_t rows = std::min<uint64_t>(N * s, std::max<uint64_t>(262144, N));
        o_wb = base;
        o_ids = o_wb + align256(n_wbase * 4);
        o_part = o_ids + align256(A_max * 4);
        o_pst = o_part + align256((size_t)rows * n * 8);
        end = o_pst + align256((size_t)rows * 4);
    }
};

// the exact path for nsel queries under ONE mask (a.allow, a.allow_bits; a.mask_of is not read): those of d_sel, or
// the first nsel of the call; the mask's word offsets are at d_wb.  shape_nsel: the query count the launch shape
// (queries per launch, segments) is chosen for.  d_list: the mask's admissible ids, already compacted (a resident
// set's cached list) -- no compaction is launched and d_wb is not read; nullptr: compacted into the scratch
int filtered_exact(const DevView &v, const FilterArgs &a, uint64_t nsel, const uint32_t *d_sel, uint64_t A,
                   const uint32_t *d_wb, uint64_t shape_nsel, const ExactScratch &x, unsigned char *dv,
                   hipStream_t stream, const uint32_t *d_list = nullptr) {
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(shape_nsel, 65535), nseg = filt_exact_segments(A, chunk);
    const uint32_t *d_ids = d_list;
    int r = HNSW_OK;
    if (!d_list) {
        uint32_t *d_scratch_ids = reinterpret_cast<uint32_t *>(dv + x.o_ids);
        r = launch_filter_compact(a, (a.allow_bits + 63) / 64, d_wb, d_scratch_ids, stream);
        d_ids = d_scratch_ids;
    }
    for (uint64_t c = 0; r == HNSW_OK && c < nsel; c += chunk) {
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
        r = launch_filtered_exact(v, ac, (uint32_t)std::min<uint64_t>(chunk, nsel - c), d_ids, (uint32_t)A, nseg,
                                  reinterpret_cast<unsigned long long *>(dv + x.o_part),
                                  reinterpret_cast<int32_t *>(dv + x.o_pst), stream);
    }
    return r;
}

// One referenced allow-list of a call: the planner's unit.  A call with one mask has one group and every query in it.
struct MaskGroup {
    const uint64_t *allow;  // the caller's words (nullptr: every id below bits)
    uint64_t row;           // first word of the mask in the call's uploaded masks
    uint64_t bits;          // its id bound: min(allow_bits, len), or len without a mask
    uint64_t A = 0;         // admissible ids
    bool exact = false;     // A <= filter_exact_max
    size_t wb = 0;            // its word offsets in the call's list: from wb_all[wb]
    size_t q0 = 0, nq = 0;    // its queries: order[q0 .. q0 + nq)
    int64_t srow = -1;        // its row of the call's resident set (-1: the call has none, or HNSW_MASK_NONE)
    uint32_t lo = 0, hi = 0;  // a range call: the group is the queries under [lo, hi] of the label column
    bool lazy_wb = false;     // ... planned on the graph path: its word offsets are counted only if a query reaches path 2
    const uint32_t *d_list = nullptr;  // ... and that row's cached list of admissible ids in HBM, when it is valid
};

}  // namespace

int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const MaskSpec &m,
                    bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                    uint8_t *paths, const PathCounters *ctr, void *pin_block) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || (!ids && !pin_block) || nq > 0x7FFFFFFFull || n > HX_FILT_MAX_N) {
        set_error("filtered search: needs queries, an id buffer, a mask when allow_bits > 0 and n <= %d",
                  HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    const bool ranged = m.lo != nullptr;  // (the entry point sees to hi)
    const bool multi = m.mask_of != nullptr || ranged;
    hnsw_mask_set *const set = m.set;  // (a call under a set is a multi call: the entry point sees to mask_of)
    if (m.mask_of) {
        bool masked = false;
        for (uint64_t i = 0; i < nq; i++) {
            if (m.mask_of[i] == HNSW_MASK_NONE) continue;
            if (m.mask_of[i] >= m.n_masks) {
                set_error("filtered search: query %llu names mask %u of %u", (unsigned long long)i, m.mask_of[i], m.n_masks);
                return HNSW_ERR_ARG;
            }
            masked = true;
        }
        if (masked && !m.masks && m.allow_bits != 0) {
            set_error("filtered search: needs the masks its queries name when allow_bits > 0");
            return HNSW_ERR_ARG;
        }
    }
    if (n == 0) {  // nothing returned, nothing launched
        if (counts) memset(counts, 0, nq * 4);
        return HNSW_OK;
    }
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    const uint64_t len = index_len(h), bits = std::min<uint64_t>(m.allow_bits, len);
    const uint64_t row_words = (m.allow_bits + 63) / 64;  // a row of the caller's masks
    // ---- the planner, per referenced mask: its admissible ids decide its queries' path ----
    std::vector<uint32_t> order;  // the queries, mask by mask (HNSW_MASK_NONE last); a one-mask call has no use for it
    std::vector<MaskGroup> groups;
    if (!multi) {
        groups.push_back(MaskGroup{m.masks, 0, bits});
        groups[0].nq = nq;
    } else if (ranged) {  // the queries range by range: a group per distinct (lo, hi) pair
        order.resize(nq);
        for (uint64_t i = 0; i < nq; i++) order[i] = (uint32_t)i;
        auto key = [&](uint32_t i) { return ((uint64_t)m.lo[i] << 32) | m.hi[i]; };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) { return key(i) < key(j); });
        for (uint64_t i = 0; i < nq; i++) {
            if (i == 0 || key(order[i]) != key(order[i - 1])) {
                groups.push_back(MaskGroup{nullptr, 0, len});
                groups.back().lo = m.lo[order[i]];
                groups.back().hi = m.hi[order[i]];
                groups.back().q0 = i;
            }
            groups.back().nq++;
        }
    } else {
        order.resize(nq);
        for (uint64_t i = 0; i < nq; i++) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) { return m.mask_of[i] < m.mask_of[j]; });
        for (uint64_t i = 0; i < nq; i++) {
            const uint32_t g = m.mask_of[order[i]];
            if (i == 0 || g != m.mask_of[order[i - 1]]) {
                if (g == HNSW_MASK_NONE)
                    groups.push_back(MaskGroup{nullptr, 0, len});
                else  // (masks may be NULL when allow_bits is 0: nothing is allowed, no word is read)
                    groups.push_back(MaskGroup{m.masks ? m.masks + g * row_words : nullptr, g * row_words, bits});
                if (set && g != HNSW_MASK_NONE && groups.back().allow) groups.back().srow = g;
                groups.back().q0 = i;
            }
            groups.back().nq++;
        }
    }
    std::vector<uint32_t> wb_all, wb;
    uint64_t A_max = 0, n_graph = 0, n_exact = 0;
    // under a set the counts come from its caches (a row is counted when it, the deleted set or the length changed);
    // the set stays locked until its HBM copy is up to date and the lists this call needs are made
    std::unique_lock<std::mutex> set_lock;
    if (set) set_lock = std::unique_lock<std::mutex>(set->mu);
    // a range's admissible ids are a slice of the label column's sorted copy (made here when the column, the deleted
    // set or the length changed): two binary searches per range, and the word offsets only for an exact-path range
    std::unique_lock<std::mutex> lab_lock;
    if (ranged) {
        lab_lock = std::unique_lock<std::mutex>(h->lab.mu);
        h->lab.sort_for(h->del, len);
    }
    for (MaskGroup &g : groups) {
        if (ranged) {
            uint64_t first;
            g.A = h->lab.count(g.lo, g.hi, &first);
            wb.clear();
            if (exact_only || (int64_t)g.A <= h->filter_exact_max) h->lab.word_base(first, g.A, len, wb);
            else g.lazy_wb = true;
        } else if (g.srow >= 0) {
            const hnsw_mask_set::Row &r = set->counted(h, (uint32_t)g.srow);
            g.A = r.A;
            wb = r.wbase;
        } else {
            g.A = count_admissible(h, g.allow, g.bits, wb);
        }
        g.exact = exact_only || (int64_t)g.A <= h->filter_exact_max;
        g.wb = wb_all.size();
        wb_all.insert(wb_all.end(), wb.begin(), wb.end());
        A_max = std::max(A_max, g.A);
        (g.exact ? n_exact : n_graph) += g.nq;
    }
    if (ranged) lab_lock.unlock();
    if (n_graph && efp > HX_FILT_MAX_EF) {
        set_error("filtered search: ef' = max(ef, n) = %u is above the graph path's maximum of %d", efp, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    // the selections: the graph path's queries in one list (none when every query takes it), the exact path's mask by
    // mask (order itself when every query takes it)
    std::vector<uint32_t> gsel, group_of;
    std::vector<uint8_t> path(nq, groups[0].exact ? 1 : 0);
    if (multi) {
        group_of.resize(nq);
        for (size_t k = 0; k < groups.size(); k++)
            for (size_t i = groups[k].q0; i < groups[k].q0 + groups[k].nq; i++) {
                group_of[order[i]] = (uint32_t)k;
                path[order[i]] = groups[k].exact ? 1 : 0;
            }
        if (n_graph && n_exact) {
            for (uint64_t i = 0; i < nq; i++)
                if (!groups[group_of[i]].exact) gsel.push_back((uint32_t)i);
        }
    }
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h)) || (set && (rc = set->sync(h))) ||
        (ranged && (rc = sync_labels(h))))
        return rc;
    const DevView &v = h->dev.view;
    const uint32_t d = v.dim;
    // device arena: [queries | masks | mask of every query | selection | the exact path's selection | the exact path's
    // scratch | result block].  All n_masks rows go up in one copy (a one-mask call sends the words below `bits` only).
    // The result block comes back in one copy to pinned memory: the caller's block, or the scratch's and from there to
    // the caller's buffers
    // (a set's rows are in HBM already: nothing goes up, and the arena has no masks; a range call has no masks
    // either: its "mask of every query" is the two arrays lo and hi, and its word offsets have room for one more range,
    // that of a path 2 group, counted when a query gets there)
    const uint64_t up_words = !m.masks || set ? 0 : multi ? (uint64_t)m.n_masks * row_words : (bits + 63) / 64;
    const size_t o_q = 0, o_mask = o_q + align256(nq * d * 4), o_mof = o_mask + align256(up_words * 8);
    const size_t o_sel = o_mof + (ranged ? 2 : 1) * align256(multi ? nq * 4 : 0), o_xsel = o_sel + align256(nq * 4);
    const size_t wb_lazy = ranged ? std::max<uint64_t>(1, ((len + 63) / 64 + 63) / 64) : 0;
    const ExactScratch x(o_xsel + align256(multi ? nq * 4 : 0), nq, n, A_max, wb_all.size() + wb_lazy);
    const size_t o_out = x.end;
    const ResultBlock out(nq, n);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, pin_block ? 0 : out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(s.dev);
    void *hv = pin_block ? pin_block : s.pin;
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + o_sel), *d_xsel = reinterpret_cast<uint32_t *>(dv + o_xsel);
    const uint64_t *d_masks = set ? set->d_rows() : up_words ? reinterpret_cast<const uint64_t *>(dv + o_mask) : nullptr;
    const uint32_t *d_wb = reinterpret_cast<const uint32_t *>(dv + x.o_wb);
    HIP_TRY(hipMemcpyAsync(dv + o_q, Q, nq * d * 4, hipMemcpyHostToDevice, s.stream));
    if ((rc = cosine_queries(h, dv + o_q, nq, s.stream))) return rc;
    if (up_words) HIP_TRY(hipMemcpyAsync(dv + o_mask, m.masks, up_words * 8, hipMemcpyHostToDevice, s.stream));
    // (under a set the word offsets of a mask go up only when a compaction of it runs)
    auto upload_wb = [&](const MaskGroup &g) -> int {
        const size_t n_wb = (&g == &groups.back() ? wb_all.size() : (&g)[1].wb) - g.wb;
        HIP_TRY(hipMemcpyAsync(dv + x.o_wb + g.wb * 4, wb_all.data() + g.wb, n_wb * 4, hipMemcpyHostToDevice, s.stream));
        return HNSW_OK;
    };
    if (!set && (bits || multi) && !wb_all.empty())
        HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (multi) {
        if (ranged) {
            HIP_TRY(hipMemcpyAsync(dv + o_mof, m.lo, nq * 4, hipMemcpyHostToDevice, s.stream));
            HIP_TRY(hipMemcpyAsync(dv + o_mof + align256(nq * 4), m.hi, nq * 4, hipMemcpyHostToDevice, s.stream));
        } else {
            HIP_TRY(hipMemcpyAsync(dv + o_mof, m.mask_of, nq * 4, hipMemcpyHostToDevice, s.stream));
        }
        if (!gsel.empty()) HIP_TRY(hipMemcpyAsync(d_sel, gsel.data(), gsel.size() * 4, hipMemcpyHostToDevice, s.stream));
        if (n_exact) HIP_TRY(hipMemcpyAsync(d_xsel, order.data(), nq * 4, hipMemcpyHostToDevice, s.stream));
    }
    FilterArgs a{};  // the graph path's arguments: every mask, the wave picks its query's
    a.Q = reinterpret_cast<const float *>(dv + o_q);
    a.qsel = gsel.empty() ? nullptr : d_sel;
    a.allow = d_masks;
    a.allow_bits = bits;
    a.mask_of = multi && !ranged ? reinterpret_cast<const uint32_t *>(dv + o_mof) : nullptr;
    if (ranged) {  // the label column and every query's range, the wave picks its own
        bind_labels(h, a);
        a.range_lo = reinterpret_cast<const uint32_t *>(dv + o_mof);
        a.range_hi = reinterpret_cast<const uint32_t *>(dv + o_mof + align256(nq * 4));
    }
    a.mask_words = row_words;
    a.none_bits = len;
    a.deny = h->del.count ? h->del.d_words : nullptr;
    a.deny_bits = h->del.count ? h->del.deny_bits() : 0;
    a.n = n;
    a.ef = efp;
    a.n_masks = m.n_masks;  // (every mask_of entry was checked against it above)
    out.bind(a, dv + o_out);
    auto group_args = [&](const MaskGroup &g) {
        FilterArgs ax = a;
        ax.mask_of = nullptr;
        ax.allow = g.allow ? d_masks + g.row : nullptr;
        ax.allow_bits = g.bits;
        ax.range_lo = ax.range_hi = nullptr;  // (a range call: the group's range as scalars)
        ax.lo = g.lo;
        ax.hi = g.hi;
        return ax;
    };
    if (set) {
        // the lists of the rows planned on the exact path: a valid one is used as it is, the others are compacted
        // into the set (while its budget lasts) here, once, for this call and the ones after it
        const uint64_t budget = h->mask_set_cache_mb > 0 ? (uint64_t)h->mask_set_cache_mb << 20 : 0;
        std::vector<hnsw_mask_set::Row *> made;
        for (MaskGroup &g : groups) {
            if (g.srow < 0) continue;
            hnsw_mask_set::Row &r = set->rows[(size_t)g.srow];
            if (!r.list_valid && g.exact && set->reserve_list(r, budget)) {
                if ((rc = upload_wb(g)) ||
                    (rc = launch_filter_compact(group_args(g), (g.bits + 63) / 64, d_wb + g.wb, r.d_ids, s.stream)))
                    return rc;
                h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
                made.push_back(&r);
            }
            if (r.list_valid || (!made.empty() && made.back() == &r)) g.d_list = r.d_ids;
        }
        if (!made.empty()) {  // (searches on other streams read the lists next)
            HIP_TRY(hipStreamSynchronize(s.stream));
            for (hnsw_mask_set::Row *r : made) r->list_valid = true;
        }
        set_lock.unlock();
    }
    // the exact path for nsel queries of one mask (sel on the device; nullptr: the first nsel of the call)
    std::vector<std::vector<uint32_t>> wb_kept;  // the word offsets of path 2 ranges, alive until the stream is waited for
    auto exact = [&](const MaskGroup &g, uint64_t nsel, const uint32_t *sel) -> int {
        if (g.lazy_wb) {  // a graph-path range whose query filled the largest table: its offsets now, in the spare room
            wb_kept.emplace_back();
            {
                std::lock_guard<std::mutex> lg(h->lab.mu);
                h->lab.sort_for(h->del, len);
                uint64_t first;
                h->lab.count(g.lo, g.hi, &first);
                h->lab.word_base(first, g.A, len, wb_kept.back());
            }
            const uint32_t *d_lazy = d_wb + wb_all.size();
            HIP_TRY(hipMemcpyAsync(dv + x.o_wb + wb_all.size() * 4, wb_kept.back().data(), wb_kept.back().size() * 4,
                                   hipMemcpyHostToDevice, s.stream));
            return filtered_exact(v, group_args(g), nsel, sel, g.A, d_lazy, nsel, x, dv, s.stream);
        }
        if (set && !g.d_list) {  // a row beyond the set's budget, or no row of the set: compacted in the scratch
            int r = upload_wb(g);
            if (r != HNSW_OK) return r;
            if (g.srow >= 0) h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
        }
        return filtered_exact(v, group_args(g), nsel, sel, g.A, d_wb + g.wb, multi ? nsel : nq, x, dv, s.stream, g.d_list);
    };
    auto fetch = [&](const hnsw_query_stats *&st) -> int {
        HIP_TRY(hipMemcpyAsync(hv, dv + o_out, out.bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        st = out.at(hv).stats;
        return HNSW_OK;
    };
    // ONE launch of the graph path for the queries of every mask planned on it, then the exact path mask by mask (its
    // scratch reused in stream order), then the result block in one copy
    const uint32_t slots = filt_first_slots_log2(v, efp, ranged);
    if (n_graph && (rc = launch_filtered_graph(v, a, (uint32_t)n_graph, slots, s.stream))) return rc;
    for (const MaskGroup &g : groups)
        if (g.exact && (rc = exact(g, g.nq, multi ? d_xsel + g.q0 : nullptr))) return rc;
    uint64_t n2 = 0;
    const hnsw_query_stats *st;
    if (!n_graph) {
        if ((rc = fetch(st))) return rc;
    } else {
        // queries whose visited table filled up run again with a table twice the size, all masks together, and those
        // that fill the largest one are answered by the exact path, each under its own mask
        std::vector<uint32_t> sel2;
        rc = rerun_overflowed(
            v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v, ranged), d_sel, s.stream, fetch,
            [&](const std::vector<uint32_t> &sel) -> int {
                for (uint32_t i : sel) path[i] = 2;
                sel2 = sel;
                if (multi) std::stable_sort(sel2.begin(), sel2.end(), [&](uint32_t i, uint32_t j) { return group_of[i] < group_of[j]; });
                HIP_TRY(hipMemcpyAsync(d_sel, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, s.stream));
                int r = HNSW_OK;
                for (size_t lo = 0, hi; r == HNSW_OK && lo < sel2.size(); lo = hi) {
                    const uint32_t k = multi ? group_of[sel2[lo]] : 0;
                    for (hi = lo + 1; hi < sel2.size() && (!multi || group_of[sel2[hi]] == k);) hi++;
                    r = exact(groups[k], hi - lo, d_sel + lo);
                }
                return r != HNSW_OK ? r : fetch(st);  // (synchronises: `sel2` lives until then)
            },
            &n2);
        if (rc != HNSW_OK) return rc;
    }
    if (ctr) {
        ctr->exact->fetch_add(n_exact, std::memory_order_relaxed);
        ctr->graph->fetch_add(n_graph - n2, std::memory_order_relaxed);
        ctr->overflow->fetch_add(n2, std::memory_order_relaxed);
    }
    if (set) {
        h->n_filt_set_calls.fetch_add(1, std::memory_order_relaxed);
    } else if (ranged) {
        h->n_filt_range_calls.fetch_add(1, std::memory_order_relaxed);
        h->n_filt_range_ranges.fetch_add(groups.size(), std::memory_order_relaxed);
    } else if (multi) {
        h->n_filt_multi_calls.fetch_add(1, std::memory_order_relaxed);
        h->n_filt_multi_masks.fetch_add(groups.size(), std::memory_order_relaxed);
    }
    if (!pin_block) out.copy_out(hv, ids, dists, counts, stats);
    if (paths) memcpy(paths, path.data(), nq);
    return HNSW_OK;
}

int search_filtered_checked(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const MaskSpec &m,
                            bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                            uint8_t *paths, const PathCounters *ctr) {
    std::vector<hnsw_query_stats> local;
    if (!stats && nq <= 0x7FFFFFFFull) {  // (more queries are refused below, before anything is allocated for them)
        local.resize(nq);
        stats = local.data();
    }
    int rc = search_filtered(h, Q, nq, n, ef, m, exact_only, ids, dists, counts, stats, paths, ctr);
    if (rc != HNSW_OK || n == 0) return rc;
    return first_query_error(stats, nq);
}

int search_device_deleted(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                          float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream, bool finish) {
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n > HX_FILT_MAX_N || efp > HX_FILT_MAX_EF) {
        set_error("search with deleted ids: needs n <= %d and ef' = max(ef, n) <= %d", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    int rc;
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h))) return rc;
    const DevView &v = h->dev.view;
    DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    // the kernels write distances and counts: stream-ordered stand-ins for the optional outputs
    struct Tmp {
        void *p = nullptr;
        hipStream_t st = nullptr;
        ~Tmp() {
            if (p) (void)hipFreeAsync(p, st);
        }
    } t_dists, t_counts;
    if (!d_dists) {
        HIP_TRY(hipMallocAsync(&t_dists.p, nq * n * 4, stream));
        t_dists.st = stream;
        d_dists = static_cast<float *>(t_dists.p);
    }
    if (!d_counts) {
        HIP_TRY(hipMallocAsync(&t_counts.p, nq * 4, stream));
        t_counts.st = stream;
        d_counts = static_cast<uint32_t *>(t_counts.p);
    }
    FilterArgs a{};
    a.Q = dq.q;
    a.allow = nullptr;
    a.allow_bits = index_len(h);
    a.deny = h->del.d_words;
    a.deny_bits = h->del.deny_bits();
    a.n = n;
    a.ef = efp;
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    const uint32_t slots = filt_first_slots_log2(v, efp);
    if (!finish) return launch_filtered_graph(v, a, (uint32_t)nq, slots, stream);

    // scratch: the selection on the device, the statuses on the host; the exact path's part ([selection | its
    // scratch]) is sized only when a query reaches it
    const size_t st_bytes = nq * sizeof(hnsw_query_stats);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), st_bytes))) return rc;
    const hnsw_query_stats *st = nullptr;
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        HIP_TRY(hipMemcpyAsync(lease.s->pin, d_stats, st_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        out = st = static_cast<const hnsw_query_stats *>(lease.s->pin);
        return HNSW_OK;
    };
    uint64_t n2 = 0;
    rc = rerun_overflowed(
        v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v), static_cast<uint32_t *>(lease.s->dev), stream, fetch,
        [&](const std::vector<uint32_t> &sel) -> int {  // path 2
            std::vector<uint32_t> wbase;
            const uint64_t A = count_admissible(h, nullptr, a.allow_bits, wbase);
            const ExactScratch x(align256(sel.size() * 4), sel.size(), n, A, wbase.size());
            int r = lease.prepare(h->dev.device, x.end, st_bytes);
            if (r != HNSW_OK) return r;
            unsigned char *dv = static_cast<unsigned char *>(lease.s->dev);
            HIP_TRY(hipMemcpyAsync(dv, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wbase.data(), wbase.size() * 4, hipMemcpyHostToDevice, stream));
            r = filtered_exact(v, a, sel.size(), reinterpret_cast<const uint32_t *>(dv), A,
                               reinterpret_cast<const uint32_t *>(dv + x.o_wb), sel.size(), x, dv, stream);
            const hnsw_query_stats *unused;
            return r != HNSW_OK ? r : fetch(unused);  // (synchronises: `sel` and `wbase` live until then)
        },
        &n2);
    if (rc != HNSW_OK) return rc;
    h->n_del_graph.fetch_add(nq - n2, std::memory_order_relaxed);
    h->n_del_overflow.fetch_add(n2, std::memory_order_relaxed);
    return first_query_error(st, nq);
}

int search_device_set(hnsw_index *h, hnsw_mask_set *set, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                      const uint32_t *d_mask_of, uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                      hnsw_query_stats *d_stats, hipStream_t stream, bool finish, uint8_t *paths) {
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n > HX_FILT_MAX_N || efp > HX_FILT_MAX_EF) {
        set_error("filtered device search: needs n <= %d and ef' = max(ef, n) <= %d", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if (!d_mask_of && set->n_masks == 0) {
        set_error("filtered device search: every query names row 0 of a set without rows");
        return HNSW_ERR_ARG;
    }
    int rc;
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h))) return rc;
    {
        std::lock_guard<std::mutex> g(set->mu);
        if ((rc = set->sync(h))) return rc;
    }
    const DevView &v = h->dev.view;
    DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    // the kernels write distances and counts: stream-ordered stand-ins for the optional outputs
    struct Tmp {
        void *p = nullptr;
        hipStream_t st = nullptr;
        ~Tmp() {
            if (p) (void)hipFreeAsync(p, st);
        }
    } t_dists, t_counts;
    if (!d_dists) {
        HIP_TRY(hipMallocAsync(&t_dists.p, nq * n * 4, stream));
        t_dists.st = stream;
        d_dists = static_cast<float *>(t_dists.p);
    }
    if (!d_counts) {
        HIP_TRY(hipMallocAsync(&t_counts.p, nq * 4, stream));
        t_counts.st = stream;
        d_counts = static_cast<uint32_t *>(t_counts.p);
    }
    const uint64_t len = index_len(h), bits = std::min<uint64_t>(set->allow_bits, len);
    FilterArgs a{};
    a.Q = dq.q;
    a.allow = set->d_rows();
    a.allow_bits = bits;
    a.mask_of = d_mask_of;
    a.mask_words = set->W;
    a.none_bits = len;
    a.n_masks = set->n_masks;  // the kernel checks d_mask_of against it: the host has not seen those words
    a.deny = h->del.count ? h->del.d_words : nullptr;
    a.deny_bits = h->del.count ? h->del.deny_bits() : 0;
    a.n = n;
    a.ef = efp;
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    const uint32_t slots = filt_first_slots_log2(v, efp);
    if (!finish) return launch_filtered_graph(v, a, (uint32_t)nq, slots, stream);

    // scratch: the selection on the device; the statuses and the rows the queries name on the host; the exact path's
    // part ([selection | its scratch]) is sized only when a query reaches it
    const size_t st_bytes = align256(nq * sizeof(hnsw_query_stats)), pin_bytes = st_bytes + nq * 4;
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), pin_bytes))) return rc;
    const hnsw_query_stats *st = nullptr;
    const uint32_t *mask_of = nullptr;
    bool have_rows = false;
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        unsigned char *pin = static_cast<unsigned char *>(lease.s->pin);
        HIP_TRY(hipMemcpyAsync(pin, d_stats, nq * sizeof(hnsw_query_stats), hipMemcpyDeviceToHost, stream));
        if (d_mask_of && !have_rows) HIP_TRY(hipMemcpyAsync(pin + st_bytes, d_mask_of, nq * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        have_rows = true;
        out = st = reinterpret_cast<const hnsw_query_stats *>(pin);
        mask_of = d_mask_of ? reinterpret_cast<const uint32_t *>(pin + st_bytes) : nullptr;
        return HNSW_OK;
    };
    std::vector<uint8_t> path(nq, 0);
    uint64_t n2 = 0;
    rc = rerun_overflowed(
        v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v), static_cast<uint32_t *>(lease.s->dev), stream, fetch,
        [&](const std::vector<uint32_t> &sel) -> int {  // path 2, row by row
            // (a query that names no row of the set ended with HNSW_ERR_ARG, not with an overflow: every row here exists)
            auto row_of = [&](uint32_t i) { return mask_of ? mask_of[i] : 0u; };
            std::vector<uint32_t> rows(sel.size()), sel2 = sel;
            std::stable_sort(sel2.begin(), sel2.end(), [&](uint32_t i, uint32_t j) { return row_of(i) < row_of(j); });
            for (size_t k = 0; k < sel2.size(); k++) rows[k] = row_of(sel2[k]);
            for (uint32_t i : sel) path[i] = 2;
            std::lock_guard<std::mutex> g(set->mu);  // the set's caches: counts, word offsets, valid lists
            struct Part {
                size_t lo, hi, wb;
                uint64_t A;
                const uint32_t *d_list;
                bool of_set;
            };
            std::vector<Part> parts;
            std::vector<uint32_t> wb_all, wb;
            uint64_t A_max = 0;
            for (size_t lo = 0, hi; lo < sel2.size(); lo = hi) {
                for (hi = lo + 1; hi < sel2.size() && rows[hi] == rows[lo];) hi++;
                Part p{lo, hi, wb_all.size(), 0, nullptr, false};
                if (rows[lo] != HNSW_MASK_NONE && set->W) {
                    const hnsw_mask_set::Row &r = set->counted(h, rows[lo]);
                    p.A = r.A;
                    p.of_set = true;
                    if (r.list_valid) p.d_list = r.d_ids;
                    else wb_all.insert(wb_all.end(), r.wbase.begin(), r.wbase.end());
                } else {
                    p.A = count_admissible(h, nullptr, rows[lo] == HNSW_MASK_NONE ? len : bits, wb);
                    wb_all.insert(wb_all.end(), wb.begin(), wb.end());
                }
                A_max = std::max(A_max, p.A);
                parts.push_back(p);
            }
            const ExactScratch x(align256(sel2.size() * 4), sel2.size(), n, A_max, wb_all.size());
            int r = lease.prepare(h->dev.device, x.end, pin_bytes);
            if (r != HNSW_OK) return r;
            unsigned char *dv = static_cast<unsigned char *>(lease.s->dev);
            const uint32_t *d_sel = reinterpret_cast<const uint32_t *>(dv);
            HIP_TRY(hipMemcpyAsync(dv, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, stream));
            if (!wb_all.empty()) HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, stream));
            for (const Part &p : parts) {
                FilterArgs ax = a;
                ax.mask_of = nullptr;
                const uint32_t row = rows[p.lo];
                ax.allow = p.of_set ? a.allow + (size_t)row * set->W : nullptr;
                ax.allow_bits = row == HNSW_MASK_NONE ? len : bits;
                if (p.of_set && !p.d_list) h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
                r = filtered_exact(v, ax, p.hi - p.lo, d_sel + p.lo, p.A, reinterpret_cast<const uint32_t *>(dv + x.o_wb) + p.wb,
                                   p.hi - p.lo, x, dv, stream, p.d_list);
                if (r != HNSW_OK) return r;
            }
            const hnsw_query_stats *unused;
            return fetch(unused);  // (synchronises: `sel2` and `wb_all` live until then)
        },
        &n2);
    if (rc != HNSW_OK) return rc;
    h->n_filt_graph.fetch_add(nq - n2, std::memory_order_relaxed);
    h->n_filt_overflow.fetch_add(n2, std::memory_order_relaxed);
    h->n_filt_set_calls.fetch_add(1, std::memory_order_relaxed);
    if (paths) memcpy(paths, path.data(), nq);
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status == HNSW_ERR_ARG) {
            set_error("filtered device search: query %llu names mask %u of %u", (unsigned long long)i,
                      mask_of ? mask_of[i] : 0u, set->n_masks);
            return HNSW_ERR_ARG;
        } else if (st[i].status != HNSW_OK) {
            return query_status_error(i, st[i].status);
        }
    return HNSW_OK;
}

int search_device_range(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, const uint32_t *d_lo,
                        const uint32_t *d_hi, uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                        hnsw_query_stats *d_stats, hipStream_t stream, bool finish, uint8_t *paths) {
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n > HX_FILT_MAX_N || efp > HX_FILT_MAX_EF) {
        set_error("filtered device search: needs n <= %d and ef' = max(ef, n) <= %d", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    int rc;
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h)) || (rc = sync_labels(h))) return rc;
    const DevView &v = h->dev.view;
    DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    // the kernels write distances and counts: stream-ordered stand-ins for the optional outputs
    struct Tmp {
        void *p = nullptr;
        hipStream_t st = nullptr;
        ~Tmp() {
            if (p) (void)hipFreeAsync(p, st);
        }
    } t_dists, t_counts;
    if (!d_dists) {
        HIP_TRY(hipMallocAsync(&t_dists.p, nq * n * 4, stream));
        t_dists.st = stream;
        d_dists = static_cast<float *>(t_dists.p);
    }
    if (!d_counts) {
        HIP_TRY(hipMallocAsync(&t_counts.p, nq * 4, stream));
        t_counts.st = stream;
        d_counts = static_cast<uint32_t *>(t_counts.p);
    }
    const uint64_t len = index_len(h);
    FilterArgs a{};
    a.Q = dq.q;
    a.allow = nullptr;
    a.allow_bits = len;
    a.none_bits = len;
    bind_labels(h, a);
    a.range_lo = d_lo;
    a.range_hi = d_hi;
    a.deny = h->del.count ? h->del.d_words : nullptr;
    a.deny_bits = h->del.count ? h->del.deny_bits() : 0;
    a.n = n;
    a.ef = efp;
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    const uint32_t slots = filt_first_slots_log2(v, efp, true);
    if (!finish) return launch_filtered_graph(v, a, (uint32_t)nq, slots, stream);

    // scratch: the selection on the device; the statuses and the ranges of the queries on the host; the exact path's
    // part ([selection | its scratch]) is sized only when a query reaches it
    const size_t st_bytes = align256(nq * sizeof(hnsw_query_stats)), r_bytes = align256(nq * 4);
    const size_t pin_bytes = st_bytes + 2 * r_bytes;
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), pin_bytes))) return rc;
    const hnsw_query_stats *st = nullptr;
    const uint32_t *lo = nullptr, *hi = nullptr;
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        unsigned char *pin = static_cast<unsigned char *>(lease.s->pin);
        HIP_TRY(hipMemcpyAsync(pin, d_stats, nq * sizeof(hnsw_query_stats), hipMemcpyDeviceToHost, stream));
        if (!lo) {
            HIP_TRY(hipMemcpyAsync(pin + st_bytes, d_lo, nq * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(pin + st_bytes + r_bytes, d_hi, nq * 4, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        out = st = reinterpret_cast<const hnsw_query_stats *>(pin);
        lo = reinterpret_cast<const uint32_t *>(pin + st_bytes);
        hi = reinterpret_cast<const uint32_t *>(pin + st_bytes + r_bytes);
        return HNSW_OK;
    };
    auto key = [&](uint32_t i) { return ((uint64_t)lo[i] << 32) | hi[i]; };
    std::vector<uint8_t> path(nq, 0);
    uint64_t n2 = 0;
    rc = rerun_overflowed(
        v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v, true), static_cast<uint32_t *>(lease.s->dev), stream, fetch,
        [&](const std::vector<uint32_t> &sel) -> int {  // path 2, range by range
            std::vector<uint32_t> sel2 = sel;
            std::stable_sort(sel2.begin(), sel2.end(), [&](uint32_t i, uint32_t j) { return key(i) < key(j); });
            std::vector<uint64_t> keys(sel2.size());
            for (size_t k = 0; k < sel2.size(); k++) keys[k] = key(sel2[k]);
            for (uint32_t i : sel) path[i] = 2;
            struct Part {
                size_t lo, hi, wb;
                uint64_t A;
            };
            std::vector<Part> parts;
            std::vector<uint32_t> wb_all, wb;
            uint64_t A_max = 0;
            {
                std::lock_guard<std::mutex> g(h->lab.mu);
                h->lab.sort_for(h->del, len);
                for (size_t p0 = 0, p1; p0 < sel2.size(); p0 = p1) {
                    for (p1 = p0 + 1; p1 < sel2.size() && keys[p1] == keys[p0];) p1++;
                    uint64_t first;
                    const uint64_t A = h->lab.count((uint32_t)(keys[p0] >> 32), (uint32_t)keys[p0], &first);
                    h->lab.word_base(first, A, len, wb);
                    parts.push_back(Part{p0, p1, wb_all.size(), A});
                    wb_all.insert(wb_all.end(), wb.begin(), wb.end());
                    A_max = std::max(A_max, A);
                }
            }
            const ExactScratch x(align256(sel2.size() * 4), sel2.size(), n, A_max, wb_all.size());
            int r = lease.prepare(h->dev.device, x.end, pin_bytes);
            if (r != HNSW_OK) return r;
            unsigned char *dv = static_cast<unsigned char *>(lease.s->dev);
            const uint32_t *d_sel = reinterpret_cast<const uint32_t *>(dv);
            HIP_TRY(hipMemcpyAsync(dv, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, stream));
            for (const Part &p : parts) {
                FilterArgs ax = a;
                ax.range_lo = ax.range_hi = nullptr;
                ax.lo = (uint32_t)(keys[p.lo] >> 32);
                ax.hi = (uint32_t)keys[p.lo];
                r = filtered_exact(v, ax, p.hi - p.lo, d_sel + p.lo, p.A, reinterpret_cast<const uint32_t *>(dv + x.o_wb) + p.wb,
                                   p.hi - p.lo, x, dv, stream);
                if (r != HNSW_OK) return r;
            }
            const hnsw_query_stats *unused;
            return fetch(unused);  // (synchronises: `sel2` and `wb_all` live until then)
        },
        &n2);
    if (rc != HNSW_OK) return rc;
    std::vector<uint64_t> named(nq);
    for (uint64_t i = 0; i < nq; i++) named[i] = key((uint32_t)i);
    std::sort(named.begin(), named.end());
    h->n_filt_graph.fetch_add(nq - n2, std::memory_order_relaxed);
    h->n_filt_overflow.fetch_add(n2, std::memory_order_relaxed);
    h->n_filt_range_calls.fetch_add(1, std::memory_order_relaxed);
    h->n_filt_range_ranges.fetch_add((uint64_t)(std::unique(named.begin(), named.end()) - named.begin()), std::memory_order_relaxed);
    if (paths) memcpy(paths, path.data(), nq);
    return first_query_error(st, nq);
}

int search_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                         float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream) {
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const DevView &v = h->dev.view;
    const size_t st_bytes = nq * sizeof(hnsw_query_stats);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), st_bytes))) return rc;
    SearchScratch &s = *lease.s;
    const hnsw_query_stats *st = static_cast<const hnsw_query_stats *>(s.pin);
    DeviceQueries dq;  // a re-run reads the queries again: the unit-length copy under the cosine option
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    SearchArgs a = ann_args(v, dq.q, n, ef, d_ids, d_dists, d_counts, d_stats);
    rc = rerun_overflowed(
        v, launch_search, a, nq, default_slots_log2(ef, v.S0), max_slots_log2(ef), static_cast<uint32_t *>(s.dev), stream,
        [&](const hnsw_query_stats *&out) -> int {
            HIP_TRY(hipMemcpyAsync(s.pin, d_stats, st_bytes, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            out = st;
            return HNSW_OK;
        },
        nullptr);
    if (rc != HNSW_OK) return rc;
    for (uint64_t i = 0; i < nq; i++) {
        if (st[i].status != HNSW_OK) {  // (this entry point's own wording, not query_status_error's)
            set_error("query %llu failed with status %d%s", (unsigned long long)i, st[i].status,
                      st[i].status == HNSW_ERR_NAN_INPUT    ? " (NaN in the query or in a distance)"
                      : st[i].status == HNSW_ERR_OVERFLOW   ? " (visited table exhausted at its largest size)"
                                                             : "");
            return st[i].status;
        }
    }
    return HNSW_OK;
}

}  // namespace hx
