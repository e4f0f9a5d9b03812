// search_host.cpp -- the host side of the search entry points: the host-pointer path, the filtered / deleted
// orchestration and the completion of a device-pointer call, around one re-run loop.  Host logic only; the kernels
// are search_kernels.hip, search_lean.hip and search_filtered.hip.

#include "search_host.h"
#include "switches.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
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
    const bool zc = sw::zero_copy() && !Q_user && !h->cosine && nq <= sw::zero_copy_max();
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
// The grouped form (exact_grouped) adds [the pass's tables], and its lists lie one behind the other in the ids' room:
// ids_grouped, the ids a pass should have room for (0: the per-group form alone); a pass that needs more is cut in two.
struct ExactScratch {
    size_t o_wb = 0, o_ids = 0, o_part = 0, o_pst = 0, o_tab = 0, end = 0;
    uint64_t ids_cap = 0, rows_cap = 0;
    ExactScratch() = default;
    ExactScratch(size_t base, uint64_t nsel_max, uint32_t n, uint64_t A_max, size_t n_wbase, uint64_t ids_grouped = 0) {
        // chunk x nseg of any launch within those limits (filt_exact_segments: at most 256 segments, and at most
        // 262144 blocks unless the queries alone are more)
        const uint64_t N = std::min<uint64_t>(nsel_max, 65535), s = filt_exact_segments(A_max, 1);
        // (a grouped pass of T <= N queries stays within them as well: every group's segments are chosen for T queries)
        const uint64_t rows = std::min<uint64_t>(N * s, std::max<uint64_t>(262144, N));
        ids_cap = std::max(A_max, ids_grouped);
        rows_cap = rows;
        o_wb = base;
        o_ids = o_wb + align256(n_wbase * 4);
        o_part = o_ids + align256(ids_cap * 4);
        o_pst = o_part + align256((size_t)rows * n * 8);
        o_tab = o_pst + align256((size_t)rows * 4);
        end = o_tab + (ids_grouped ? tab_bytes(N, N) : 0);
    }
    // a pass's tables: [a record per query | its selection | a record per compacted group]
    static size_t tab_bytes(uint64_t nsel, uint64_t ngroups) {
        return align256(nsel * sizeof(ExactQuery)) + align256(nsel * 4) + align256(ngroups * sizeof(ExactGroup));
    }
};

// the exact path for nsel queries under ONE mask (a.allow, a.allow_bits; a.mask_of is not read): those of d_sel, or
// the first nsel of the call; the mask's word offsets are at d_wb.  shape_nsel: the query count the launch shape
// (queries per launch, segments) is chosen for.  d_list: the mask's admissible ids, already compacted (a resident
// set's cached list) -- no compaction is launched and d_wb is not read; nullptr: compacted into the scratch, under
// `ranges` when the mask is the union of several label ranges
int filtered_exact(const DevView &v, const FilterArgs &a, uint64_t nsel, const uint32_t *d_sel, uint64_t A,
                   const uint32_t *d_wb, uint64_t shape_nsel, const ExactScratch &x, unsigned char *dv,
                   hipStream_t stream, const uint32_t *d_list = nullptr, const RangeList *ranges = nullptr) {
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(shape_nsel, 65535), nseg = filt_exact_segments(A, chunk);
    const uint32_t *d_ids = d_list;
    int r = HNSW_OK;
    if (!d_list) {
        uint32_t *d_scratch_ids = reinterpret_cast<uint32_t *>(dv + x.o_ids);
        r = launch_filter_compact(a, (a.allow_bits + 63) / 64, d_wb, d_scratch_ids, stream, ranges);
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

// ---- the filter of a call --------------------------------------------------------------------------------------
// A query's filter is named by a key and a list.  The key: the query's row (or HNSW_MASK_NONE) in a call with a row per
// query, 0 otherwise.  The list: the index of the query's canonical range list in the call's table of them
// (FilterSource::intern), NO_LIST in a call without label ranges: two raw lists with one canonical form are one list.
// The queries under one (key, list) are a group: the planner's unit, and that of the exact path's launches.
constexpr uint64_t UNCOUNTED = ~0ull;
constexpr uint64_t FULL_RANGE = 0xFFFFFFFFull;  // [0, UINT32_MAX]
constexpr uint32_t NO_LIST = ~0u;
constexpr size_t NO_WB = ~(size_t)0;
struct Group {
    uint64_t key = 0;
    uint32_t list = NO_LIST;
    size_t q0 = 0, nq = 0;             // its queries: [q0, q0 + nq) of the sorted list it was cut from
    uint64_t A = UNCOUNTED;            // admissible ids (a row AND a range planned on the graph path: not counted, at most A_ub)
    uint64_t A_ub = 0;
    bool exact = false;                // A <= filter_exact_max: planned on the exact path
    size_t wb = NO_WB, n_wb = 0;       // its word offsets in the list they were counted into (NO_WB: not counted yet)
    const uint32_t *d_list = nullptr;  // a set row's cached list of admissible ids in HBM, when it is valid
};

// What turns a group into what the exact path needs, one per call, made from the call's Filter: the rows and the label
// column behind the groups, the key and the ranges of every query (host memory) and the call's own arguments.  Beyond
// the constructor nothing asks what kind of call it is, only whether a group has words and whether it has a range list.
struct FilterSource {
    hnsw_index *h;
    const Filter::Family family;
    hnsw_mask_set *set;             // Filter::SET
    const uint64_t *masks;          // the caller's words (Filter::ONE, MANY; nullptr: none)
    bool rowed;                     // a row per query (MANY, SET), else key 0
    uint32_t K, n_masks;            // ranges per query; rows
    uint64_t len, bits, row_words;  // the index length, min(allow_bits, len), words of a row
    // per query, in host memory: a device-pointer call has them only once its _finish has fetched them
    const uint32_t *mask_of = nullptr, *lo = nullptr, *hi = nullptr;
    FilterArgs base{};  // every row and range: the graph kernel's wave picks its query's
    // The call's canonical lists (LabelColumn::canonical: disjoint, ascending, no empty member; a list without members
    // is the one empty range (1, 0)), ascending, list j's members at members[start[j] .. start[j + 1]); query i is under
    // list_of[i].  With K == 1 the member is the caller's pair as it is, lo > hi included
    std::vector<uint32_t> list_of, start;
    std::vector<uint64_t> members;
    bool interned() const { return !start.empty(); }
    size_t n_lists() const { return start.size() - 1; }
    uint64_t raw(uint64_t i) const { return ((uint64_t)lo[i] << 32) | hi[i]; }
    void intern(uint64_t nq) {
        list_of.resize(nq);
        members.clear();
        start.assign(1, 0);
        if (K == 1) {  // (no canonical form to make: the distinct pairs, sorted)
            members.resize(nq);
            for (uint64_t i = 0; i < nq; i++) members[i] = raw(i);
            std::sort(members.begin(), members.end());
            members.erase(std::unique(members.begin(), members.end()), members.end());
            for (size_t j = 1; j <= members.size(); j++) start.push_back((uint32_t)j);
            for (uint64_t i = 0; i < nq; i++)
                list_of[i] = (uint32_t)(std::lower_bound(members.begin(), members.end(), raw(i)) - members.begin());
            return;
        }
        std::map<std::vector<uint64_t>, uint32_t> table;
        std::vector<std::map<std::vector<uint64_t>, uint32_t>::iterator> at(nq);
        for (uint64_t i = 0; i < nq; i++) {
            std::vector<uint64_t> c = LabelColumn::canonical(lo + i * K, hi + i * K, K);
            if (c.empty()) c.push_back(1ull << 32);
            at[i] = table.emplace(std::move(c), 0u).first;
        }
        for (auto &e : table) {
            e.second = (uint32_t)n_lists();
            members.insert(members.end(), e.first.begin(), e.first.end());
            start.push_back((uint32_t)members.size());
        }
        for (uint64_t i = 0; i < nq; i++) list_of[i] = at[i]->second;
    }

    FilterSource(hnsw_index *h_, const Filter &f)
        : h(h_), family(f.family), set(f.rows == Filter::SET ? f.set : nullptr),
          masks(f.rows == Filter::ONE || f.rows == Filter::MANY ? f.masks : nullptr),
          rowed(f.rows == Filter::MANY || f.rows == Filter::SET), K(f.K), n_masks(set ? set->n_masks : f.n_masks),
          len(index_len(h_)) {
        const uint64_t allow_bits = set ? set->allow_bits : f.rows == Filter::ALL ? len : f.allow_bits;
        bits = std::min<uint64_t>(allow_bits, len);
        row_words = (allow_bits + 63) / 64;
        if (!f.on_device) mask_of = f.mask_of, lo = f.lo, hi = f.hi;
    }

    uint64_t key(uint32_t i) const { return rowed && mask_of ? mask_of[i] : 0; }
    uint32_t list(uint32_t i) const { return K ? list_of[i] : NO_LIST; }
    const uint64_t *members_of(const Group &g) const { return members.data() + start[g.list]; }
    size_t n_members(const Group &g) const { return start[g.list + 1] - start[g.list]; }
    // the key names a row with words (masks may be NULL when allow_bits is 0: nothing is allowed, no word is read)
    bool has_words(uint64_t key) const { return key != HNSW_MASK_NONE && (set ? set->W != 0 : masks != nullptr); }
    // the group is under its range list.  Next to a set, [0, UINT32_MAX] is no range: the group is the plain row, with the
    // set's caches (and so is a row of a set without words: nothing is allowed); under HNSW_MASK_NONE it is the plain range
    bool ranged(const Group &g) const {
        return K && (!set || (members_of(g)[0] != FULL_RANGE && (g.key == HNSW_MASK_NONE || set->W != 0)));
    }
    // its id bound (without rows of its own a call's bits are the index length)
    uint64_t bound(uint64_t key) const { return key == HNSW_MASK_NONE ? len : bits; }

    // base, but for the outputs and the selection; d_*: what the kernels read, on the device
    void bind(const float *d_Q, const uint64_t *d_allow, const uint32_t *d_mask_of, const uint32_t *d_lo,
              const uint32_t *d_hi, uint32_t n, uint32_t efp) {
        base.Q = d_Q;
        base.allow = d_allow;
        base.allow_bits = bits;
        base.mask_of = d_mask_of;
        base.mask_words = row_words;
        base.none_bits = len;
        base.n_masks = n_masks;  // the kernel checks mask_of against it (the host may not have seen those words)
        base.deny = h->del.count ? h->del.d_words : nullptr;
        base.deny_bits = h->del.count ? h->del.deny_bits() : 0;
        if (K) bind_labels(h, base);
        base.range_lo = d_lo;
        base.range_hi = d_hi;
        base.n_ranges = K;  // (the kernels read it above 1 only)
        base.n = n;
        base.ef = efp;
    }
    // the arguments of an exact-path launch: the group's row, its ranges, or both, alone
    FilterArgs args(const Group &g) const {
        FilterArgs ax = base;
        const uint64_t m0 = ranged(g) ? members_of(g)[0] : 0;  // (the first member; one member: the launch's whole range)
        ax.mask_of = nullptr;
        ax.allow = has_words(g.key) ? base.allow + g.key * row_words : nullptr;
        ax.allow_bits = bound(g.key);
        ax.range_lo = ax.range_hi = nullptr;      // (the group's range as scalars)
        if (!ranged(g)) ax.labels = nullptr;      // (a plain row next to ranged groups: the compaction reads its words alone)
        ax.lo = (uint32_t)(m0 >> 32), ax.hi = (uint32_t)m0;
        ax.n_ranges = 0;
        return ax;
    }
    // ... and its canonical list, by value, for the compaction (n == 0: the group is under args' lo / hi alone)
    RangeList range_list(const Group &g) const {
        RangeList r{};
        if (!ranged(g) || n_members(g) < 2) return r;
        r.n = (uint32_t)n_members(g);
        for (uint32_t j = 0; j < r.n; j++) r.lo[j] = (uint32_t)(members_of(g)[j] >> 32), r.hi[j] = (uint32_t)members_of(g)[j];
        return r;
    }

    // What `resolve` reads is locked by this: a set's caches (a row is counted when it, the deleted set or the length
    // changed), and the label column's sorted copy (made under the lock, by the first group that has a range, when the
    // column, the deleted set or the length changed).  The set's first, then the column's
    struct Locks {
        std::unique_lock<std::mutex> set, lab;
        bool held() const { return set.owns_lock() || lab.owns_lock(); }
    };
    Locks lock() const {
        Locks l;
        if (set) l.set = std::unique_lock<std::mutex>(set->mu);
        if (K) l.lab = std::unique_lock<std::mutex>(h->lab.mu);
        return l;
    }
    // The admissible ids of a row AND a range: the undeleted ids below `bits` whose bit is set in the row and whose
    // label lies in [lo, hi].  Neither side's count says how many: the cheaper side is walked -- the range's slice of
    // the sorted copy (undeleted ids already) testing the row's bits, or the row's set bits testing labels -- and only
    // while the count stays within `limit`: beyond it the group is on the graph path and the count is not needed
    // (UNCOUNTED; A_ub, the smaller side, bounds it).  The same walk gives the compaction's offsets, the admissible ids
    // before every block of 64 words.  The row's own cached count is read; its offsets and its list are the row's alone
    uint64_t count_both(uint32_t row, uint32_t lo, uint32_t hi, int64_t limit, std::vector<uint32_t> &wbase, uint64_t &A_ub) const {
        uint64_t first = 0;
        const uint64_t S = h->lab.count(lo, hi, &first), RA = set->counted(h, row).A;
        A_ub = std::min(S, RA);
        const uint64_t n_words = (bits + 63) / 64, n_wblk = std::max<uint64_t>(1, (n_words + 63) / 64);
        const uint64_t *w = set->row_words(row);
        uint64_t A = 0;
        if (S <= RA) {
            wbase.assign(n_wblk + 1, 0);  // ids per block, shifted by one
            for (uint64_t i = first; i < first + S; i++) {
                const uint32_t id = (uint32_t)h->lab.sorted[i];
                if (id >= bits || ((w[id >> 6] >> (id & 63)) & 1ull) == 0) continue;
                if ((int64_t)++A > limit) return UNCOUNTED;
                wbase[(id >> 12) + 1]++;
            }
            for (size_t b = 1; b < wbase.size(); b++) wbase[b] += wbase[b - 1];
            wbase.pop_back();
        } else {
            const std::vector<uint64_t> &deny = h->del.words;
            const bool denies = h->del.count > 0;
            wbase.assign(n_wblk, 0);
            for (uint64_t ww = 0; ww < n_words; ww++) {
                if (ww % 64 == 0) wbase[ww / 64] = (uint32_t)A;
                uint64_t x = w[ww];
                if (ww == n_words - 1 && bits % 64) x &= (1ull << (bits % 64)) - 1;
                if (denies && ww < deny.size()) x &= ~deny[ww];
                for (; x; x &= x - 1) {
                    if (h->lab.get(ww * 64 + (uint64_t)__builtin_ctzll(x)) - lo > hi - lo) continue;
                    if ((int64_t)++A > limit) return UNCOUNTED;
                }
            }
        }
        return A;
    }
    // Counts a group: A (kept when it is known already), exact = A <= exact_max, a set row's list while it is valid, and
    // its word offsets, appended to wbs.  The admissible ids of a range list are its disjoint members' slices of the
    // sorted copy, each found by two binary searches: A is their sum; the offsets cost a pass over the slices and are
    // counted only when the group is exact.  A row AND a range are counted by count_both, up to exact_max
    void resolve(Group &g, int64_t exact_max, std::vector<uint32_t> &wbs) const {
        std::vector<uint32_t> own;
        const std::vector<uint32_t> *wb = &own;
        const bool rg = ranged(g), words = has_words(g.key);
        uint64_t A = 0;
        std::vector<std::pair<uint64_t, uint64_t>> slices;  // (first, count) of every member
        if (rg) h->lab.sort_for(h->del, len);
        if (rg && words) {
            const uint32_t lo1 = (uint32_t)(members_of(g)[0] >> 32), hi1 = (uint32_t)members_of(g)[0];
            A = lo1 > hi1 ? 0 : count_both((uint32_t)g.key, lo1, hi1, exact_max, own, g.A_ub);
            if (A == UNCOUNTED) {
                g.exact = false;
                return;
            }
        } else if (rg) {
            for (size_t j = 0; j < n_members(g); j++) {
                uint64_t first = 0;
                const uint64_t c = h->lab.count((uint32_t)(members_of(g)[j] >> 32), (uint32_t)members_of(g)[j], &first);
                slices.emplace_back(first, c);
                A += c;
            }
        } else if (set && words) {
            const hnsw_mask_set::Row &r = set->counted(h, (uint32_t)g.key);
            A = r.A;
            wb = &r.wbase;
            g.d_list = r.list_valid ? r.d_ids : nullptr;
        } else {
            A = count_admissible(h, words ? masks + g.key * row_words : nullptr, bound(g.key), own);
        }
        if (g.A == UNCOUNTED) g.A = A;
        g.exact = (int64_t)g.A <= exact_max;
        if (rg && !g.exact) return;
        if (rg && !words) h->lab.word_base(slices, len, own);
        g.wb = wbs.size();
        g.n_wb = wb->size();
        wbs.insert(wbs.end(), wb->begin(), wb->end());
    }
    // the distinct groups of the call's nq queries, for its counters (a device-pointer call's, which cuts no groups)
    uint64_t n_groups(uint64_t nq) const {
        if (!(rowed && mask_of)) return n_lists();
        std::vector<std::pair<uint64_t, uint64_t>> named(nq);  // (a row per query: K == 1, the pair is the list)
        for (uint64_t i = 0; i < nq; i++) named[i] = {mask_of[i], raw(i)};
        std::sort(named.begin(), named.end());
        return (uint64_t)(std::unique(named.begin(), named.end()) - named.begin());
    }
};

// stable-sorts query indices by (key, list) and cuts them into runs: ascending key (HNSW_MASK_NONE last among rows),
// ascending list within a key, the caller's order within a run
bool group_before(const Group &g, uint64_t key, uint32_t list) { return g.key != key ? g.key < key : g.list < list; }
std::vector<Group> group_by_key(std::vector<uint32_t> &idx, const FilterSource &src) {
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t i, uint32_t j) {
        const uint64_t ki = src.key(i), kj = src.key(j);
        return ki != kj ? ki < kj : src.list(i) < src.list(j);
    });
    std::vector<Group> runs;
    for (size_t k = 0; k < idx.size(); k++) {
        const uint64_t key = src.key(idx[k]);
        const uint32_t list = src.list(idx[k]);
        if (k == 0 || key != runs.back().key || list != runs.back().list) {
            runs.emplace_back();
            runs.back().key = key;
            runs.back().list = list;
            runs.back().q0 = k;
        }
        runs.back().nq++;
    }
    return runs;
}

// Where a call's exact path runs: a device arena with its scratch, a stream, and the word offsets on the host (wbs)
// and on the device (d_wb, where group g's are at d_wb + g.wb).  send: they are not there yet and go up group by group
// (under a set, where most groups have a list and need none).
struct ExactPlace {
    unsigned char *dv;
    ExactScratch x;
    hipStream_t stream;
    const uint32_t *wbs;
    uint32_t *d_wb;
    bool send;
};

// the exact path for the g.nq queries of one group: those of d_sel, or the first g.nq of the call
int exact_group(const FilterSource &src, const Group &g, const uint32_t *d_sel, uint64_t shape_nsel, const ExactPlace &at) {
    if (!g.d_list && at.send) {  // compacted in the scratch: a row beyond the set's budget, or no row of the set
        HIP_TRY(hipMemcpyAsync(at.d_wb + g.wb, at.wbs + g.wb, g.n_wb * 4, hipMemcpyHostToDevice, at.stream));
        if (src.set && src.has_words(g.key) && !src.ranged(g)) src.h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
    }
    const RangeList ranges = src.range_list(g);
    return filtered_exact(src.h->dev.view, src.args(g), g.nq, d_sel, g.A, at.d_wb + g.wb, shape_nsel, at.x, at.dv, at.stream,
                          g.d_list, &ranges);
}

// ---- the grouped form of the exact path -----------------------------------------------------
// Many small groups -- a coalesced batch of one-query calls, each under its tenant's filter -- cost three dependent
// launches each in the form above.  Here the groups of a pass share them: ONE compaction whose blockIdx.y is the group,
// ONE scan and ONE merge over every query of every group, each query under its own list.  What a launch has in its
// scalars otherwise is in two tables in the arena (ExactGroup, ExactQuery: search_filtered.h), written on the host and
// sent up in one copy with the pass's selection.  The lists lie one behind the other in the ids' room; a group whose
// list a resident set holds contributes it by pointer and is not compacted; one without admissible ids is not either; one
// under K > 1 ranges keeps a compaction launch of its own (its RangeList travels by value) and shares the other two.  The
// results are those of the per-group form bit for bit: the top n keys of a list do not depend on how it was cut.
struct PassItem {
    Group g;                // (g.wb is not read: the offsets are wbs / d_wb)
    const uint32_t *sel;    // its queries, on the host ...
    const uint32_t *d_sel;  // ... and on the device (read when the group has to go by itself)
    const uint32_t *wbs;    // its word offsets on the host, and their place on the device
    uint32_t *d_wb;
    bool send;              // they are not there yet ...
    int from;               // ... and go up with those of the pass's other groups from the same host array (0 or 1)
};

int exact_grouped(const FilterSource &src, std::vector<PassItem> &items, const ExactPlace &at,
                  std::vector<std::vector<unsigned char>> &keep) {
    hnsw_index *h = src.h;
    const DevView &v = h->dev.view;
    uint64_t total = 0;
    for (const PassItem &it : items) total += it.g.nq;
    const uint32_t shape = (uint32_t)std::min<uint64_t>(total, 65535);
    uint32_t *d_ids0 = reinterpret_cast<uint32_t *>(at.dv + at.x.o_ids);
    auto compacts = [](const PassItem &it) { return !it.g.d_list && it.g.A > 0; };
    size_t i0 = 0;
    while (i0 < items.size()) {
        // the pass: as many groups from i0 as the launch limits and the rooms take
        uint64_t nsel = 0, rows = 0, ids = 0;
        size_t i1 = i0;
        for (; i1 < items.size(); i1++) {
            const Group &g = items[i1].g;
            const uint64_t r = g.nq * filt_exact_segments(g.A, shape), a = compacts(items[i1]) ? g.A : 0;
            if (nsel + g.nq > 65535 || rows + r > std::min<uint64_t>(at.x.rows_cap, HX_FILT_MAX_PART_ROWS - 1) || ids + a > at.x.ids_cap) break;
            nsel += g.nq, rows += r, ids += a;
        }
        if (i1 == i0) {  // a group no pass takes: by itself, in the per-group form
            PassItem &it = items[i0++];
            ExactPlace p = at;
            p.wbs = it.wbs, p.d_wb = it.d_wb, p.send = it.send;
            it.g.wb = 0;
            if (int r = exact_group(src, it.g, it.d_sel, it.g.nq, p)) return r;
            continue;
        }
        const size_t o_sel = align256(nsel * sizeof(ExactQuery)), o_gt = o_sel + align256(nsel * 4);
        keep.emplace_back(o_gt + (i1 - i0) * sizeof(ExactGroup));
        unsigned char *blob = keep.back().data();
        ExactQuery *qt = reinterpret_cast<ExactQuery *>(blob);
        uint32_t *sel = reinterpret_cast<uint32_t *>(blob + o_sel);
        ExactGroup *gt = reinterpret_cast<ExactGroup *>(blob + o_gt);
        uint32_t ngt = 0, max_nseg = 1;
        uint64_t y = 0, row = 0, at_id = 0, max_words = 0;
        // the spans of host offsets that go up, one copy per host array (its groups' places on the device mirror it)
        const uint32_t *send_lo[2] = {nullptr, nullptr}, *send_hi[2] = {nullptr, nullptr};
        uint32_t *send_to[2] = {nullptr, nullptr};
        for (size_t i = i0; i < i1; i++) {
            const PassItem &it = items[i];
            const Group &g = it.g;
            const uint32_t nseg = filt_exact_segments(g.A, shape);
            const uint32_t *list = g.d_list ? g.d_list : d_ids0 + at_id;
            max_nseg = std::max(max_nseg, nseg);
            if (compacts(it)) {
                const FilterArgs ax = src.args(g);
                const RangeList ranges = src.range_list(g);
                if (it.send) {
                    // (the groups of a pass have their offsets in one host array, a place apart on the device as there)
                    const int f = it.from;
                    if (!send_lo[f] || it.wbs < send_lo[f]) send_lo[f] = it.wbs, send_to[f] = it.d_wb;
                    if (!send_hi[f] || it.wbs + g.n_wb > send_hi[f]) send_hi[f] = it.wbs + g.n_wb;
                    if (src.set && src.has_words(g.key) && !src.ranged(g)) h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
                }
                if (ranges.n > 1) {  // (after the offsets are up: below)
                } else {
                    ExactGroup &e = gt[ngt++];
                    e.allow = ax.allow;
                    e.word_base = it.d_wb;
                    e.ids = d_ids0 + at_id;
                    e.allow_bits = ax.allow_bits;
                    e.lo = ax.lo, e.hi = ax.hi;
                    e.ranged = ax.labels != nullptr;
                    e.pad = 0;
                    max_words = std::max<uint64_t>(max_words, (ax.allow_bits + 63) / 64);
                }
                at_id += g.A;
            }
            for (size_t k = 0; k < g.nq; k++, y++) {
                qt[y].ids = list;
                qt[y].A = (uint32_t)g.A;
                qt[y].seg = (uint32_t)(row << HX_FILT_SEG_BITS) | nseg;
                sel[y] = it.sel[k];
                row += nseg;
            }
        }
        unsigned char *d_tab = at.dv + at.x.o_tab;
        HIP_TRY(hipMemcpyAsync(d_tab, blob, o_gt + ngt * sizeof(ExactGroup), hipMemcpyHostToDevice, at.stream));
        for (int f = 0; f < 2; f++)
            if (send_lo[f])
                HIP_TRY(hipMemcpyAsync(send_to[f], send_lo[f], (size_t)(send_hi[f] - send_lo[f]) * 4, hipMemcpyHostToDevice, at.stream));
        FilterArgs a = src.base;  // what the groups share; a group's row and range are in its record
        a.mask_of = nullptr;
        a.allow = nullptr;
        a.range_lo = a.range_hi = nullptr;
        a.lo = a.hi = 0;
        a.n_ranges = 0;
        a.qsel = reinterpret_cast<const uint32_t *>(d_tab + o_sel);
        int r = launch_filter_compact_grouped(a, reinterpret_cast<const ExactGroup *>(d_tab + o_gt), ngt, max_words, at.stream);
        at_id = 0;
        for (size_t i = i0; r == HNSW_OK && i < i1; i++) {
            if (!compacts(items[i])) continue;
            const Group &g = items[i].g;
            const RangeList ranges = src.range_list(g);
            if (ranges.n > 1) {
                const FilterArgs ax = src.args(g);
                r = launch_filter_compact(ax, (ax.allow_bits + 63) / 64, items[i].d_wb, d_ids0 + at_id, at.stream, &ranges);
            }
            at_id += g.A;
        }
        if (r == HNSW_OK)
            r = launch_filtered_exact_grouped(v, a, (uint32_t)nsel, reinterpret_cast<const ExactQuery *>(d_tab), max_nseg,
                                              reinterpret_cast<unsigned long long *>(at.dv + at.x.o_part),
                                              reinterpret_cast<int32_t *>(at.dv + at.x.o_pst), at.stream);
        if (r != HNSW_OK) return r;
        i0 = i1;
    }
    return HNSW_OK;
}

// Path 2: the queries of `sel` filled the largest visited table and are answered by the exact path, each under its own
// filter, group by group; then `fetch`, which synchronises.  The host form comes with its plan (`planned`, ascending
// key; shape_nsel; `at`: its arena, laid out up front because the queries and the result block live in it, with the
// selection at d_sel and room for one group's offsets at at.d_wb + spare) and nothing is allocated; a device form
// (`grow`) has counted nothing yet and sizes [selection | exact scratch] in its lease only now.  A group that is not
// counted yet -- every group of a device form, a graph-planned range of the host form -- is counted here, and its
// offsets go up to that one room just before its launches (the scratch is reused in stream order).
template <class Fetch>
int path2(const FilterSource &src, const std::vector<uint32_t> &sel, std::vector<uint8_t> &path,
          const std::vector<Group> *planned, uint64_t shape_nsel, ExactPlace at, uint32_t *d_sel, size_t spare,
          ScratchLease *grow, size_t pin_bytes, Fetch fetch, bool grouping) {
    std::vector<uint32_t> sel2 = sel, wb_late;
    std::vector<Group> runs = group_by_key(sel2, src);
    for (uint32_t i : sel) path[i] = 2;
    FilterSource::Locks lock;  // (a set's stays until the end: its lists are read by the launches)
    std::vector<bool> late(runs.size(), false);
    grouping = grouping && runs.size() > 1;  // (grouped: the late groups' offsets lie one behind the other, as in wb_late)
    uint64_t A_max = 0, A_sum = 0;
    size_t n_wb = 0;
    for (size_t k = 0; k < runs.size(); k++) {
        Group &g = runs[k];
        if (planned) {
            const Group &p = *std::lower_bound(planned->begin(), planned->end(), g,
                                               [](const Group &x, const Group &y) { return group_before(x, y.key, y.list); });
            g.A = p.A, g.wb = p.wb, g.n_wb = p.n_wb, g.d_list = p.d_list;
        }
        if (g.wb == NO_WB) {
            if (!lock.held()) lock = src.lock();
            src.resolve(g, INT64_MAX, wb_late);
            late[k] = true;
        }
        A_max = std::max(A_max, g.A);
        A_sum += g.d_list ? 0 : g.A;
        n_wb = std::max(n_wb, g.n_wb);
    }
    if (lock.lab.owns_lock()) lock.lab.unlock();  // (the column's: never across a sync)
    if (grow) {
        at.x = ExactScratch(align256(sel2.size() * 4), sel2.size(), src.base.n, A_max, grouping ? wb_late.size() : n_wb,
                            grouping ? std::max<uint64_t>(A_sum, 1) : 0);
        int r = grow->prepare(src.h->dev.device, at.x.end, pin_bytes);
        if (r != HNSW_OK) return r;
        at.dv = static_cast<unsigned char *>(grow->s->dev);
        d_sel = reinterpret_cast<uint32_t *>(at.dv);
        at.d_wb = reinterpret_cast<uint32_t *>(at.dv + at.x.o_wb);
        spare = 0;
    }
    HIP_TRY(hipMemcpyAsync(d_sel, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, at.stream));
    std::vector<std::vector<unsigned char>> keep;
    if (grouping) {  // one more pass of the grouped form
        std::vector<PassItem> items;
        for (size_t k = 0; k < runs.size(); k++) {
            const Group &g = runs[k];
            if (late[k])
                items.push_back({g, sel2.data() + g.q0, d_sel + g.q0, wb_late.data() + g.wb, at.d_wb + spare + g.wb, true, 1});
            else
                items.push_back({g, sel2.data() + g.q0, d_sel + g.q0, at.wbs + g.wb, at.d_wb + g.wb, at.send, 0});
        }
        int r = exact_grouped(src, items, at, keep);
        if (r != HNSW_OK) return r;
        const hnsw_query_stats *unused;
        return fetch(unused);  // (synchronises: `sel2`, `wb_late` and the tables live until then)
    }
    for (size_t k = 0; k < runs.size(); k++) {
        Group g = runs[k];
        ExactPlace p = at;
        if (late[k]) {  // its offsets: from wb_late to the one room
            p.wbs = wb_late.data() + g.wb;
            p.d_wb = at.d_wb + spare;
            p.send = true;
            g.wb = 0;
        }
        int r = exact_group(src, g, d_sel + g.q0, shape_nsel ? shape_nsel : g.nq, p);
        if (r != HNSW_OK) return r;
    }
    const hnsw_query_stats *unused;
    return fetch(unused);  // (synchronises: `sel2` and `wb_late` live until then)
}

// The counters of a call that ended well, by the entry points that made it: its queries per path under filtered_* or
// deleted_*, the call itself, and its groups
void count_call(hnsw_index *h, Filter::Family family, uint64_t n_graph, uint64_t n_exact, uint64_t n_overflow, uint64_t n_groups) {
    if (family == Filter::SCAN) return;  // (hnsw_brute_force counts nothing)
    const bool del = family == Filter::DELETED;
    (del ? h->n_del_graph : h->n_filt_graph).fetch_add(n_graph, std::memory_order_relaxed);
    (del ? h->n_del_exact : h->n_filt_exact).fetch_add(n_exact, std::memory_order_relaxed);
    (del ? h->n_del_overflow : h->n_filt_overflow).fetch_add(n_overflow, std::memory_order_relaxed);
    std::atomic<uint64_t> *calls = nullptr, *groups = nullptr;
    switch (family) {
        case Filter::MULTI: calls = &h->n_filt_multi_calls, groups = &h->n_filt_multi_masks; break;
        case Filter::OF_SET: calls = &h->n_filt_set_calls; break;
        case Filter::RANGE: calls = &h->n_filt_range_calls, groups = &h->n_filt_range_ranges; break;
        case Filter::SET_RANGE: calls = &h->n_filt_set_range_calls, groups = &h->n_filt_set_range_groups; break;
        case Filter::RANGES: calls = &h->n_filt_ranges_calls, groups = &h->n_filt_ranges_groups; break;
        // (hnsw_search_filtered: `calls` are its leaders' launches, and every query of one is a call answered)
        case Filter::ONE_QUERY:
            calls = &h->n_filt_one_batches;
            h->n_filt_one_calls.fetch_add(n_graph + n_exact + n_overflow, std::memory_order_relaxed);
            break;
        default: break;
    }
    if (calls) calls->fetch_add(1, std::memory_order_relaxed);
    if (groups) groups->fetch_add(n_groups, std::memory_order_relaxed);
}

// the combinations of rows and ranges no entry point offers (search_host.h's table)
int check_filter(const Filter &f) {
    if (f.K <= (f.rows == Filter::ALL ? (uint32_t)HX_FILT_MAX_RANGES : f.rows == Filter::SET ? 1u : 0u)) return HNSW_OK;
    set_error("filtered search: no search under these rows and %u label ranges per query", f.K);
    return HNSW_ERR_ARG;
}

}  // namespace

int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const Filter &f,
                    bool exact_only, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats,
                    uint8_t *paths, void *pin_block, bool grouped) {
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
    if (src.rowed) {
        bool masked = false;
        for (uint64_t i = 0; i < nq; i++) {
            if (src.mask_of[i] == HNSW_MASK_NONE) continue;
            if (src.mask_of[i] >= src.n_masks) {
                set_error("filtered search: query %llu names mask %u of %u", (unsigned long long)i, src.mask_of[i], src.n_masks);
                return HNSW_ERR_ARG;
            }
            masked = true;
        }
        if (masked && !src.set && !src.masks && f.allow_bits != 0) {
            set_error("filtered search: needs the masks its queries name when allow_bits > 0");
            return HNSW_ERR_ARG;
        }
    }
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
    // ---- the planner, per group: its admissible ids decide its queries' path.  A set stays locked until its HBM copy
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
    const uint32_t d = v.dim;
    // device arena: [queries | masks | row of every query | lo | hi | selection | the exact path's selection | the exact
    // path's scratch | result block]: the caller's masks when it brought any (all n_masks rows in one copy; a one-mask
    // call sends the words below `bits` only; a set's rows are in HBM already), the rows with a row per query, lo and hi
    // with ranges -- and then the word offsets have room for one more group, that of a path 2 group, counted when a
    // query gets there.  The result block comes back in one copy to pinned memory: the caller's block, or the scratch's
    // and from there to the caller's buffers
    const uint64_t up_words = !src.masks ? 0 : rowed ? (uint64_t)src.n_masks * src.row_words : (bits + 63) / 64;
    const size_t o_q = 0, o_mask = o_q + align256(nq * d * 4), o_mof = o_mask + align256(up_words * 8);
    const size_t o_lo = o_mof + (rowed ? align256(nq * 4) : 0), o_hi = o_lo + (ranged ? align256(nq * rk * 4) : 0);
    const size_t o_sel = o_hi + (ranged ? align256(nq * rk * 4) : 0), o_xsel = o_sel + align256(nq * 4);
    // The grouped form of the exact path (exact_grouped): the lists of a pass's groups lie one behind the other, so the
    // ids' room is that of the planned pass, and of a path 2 pass up to 4 Mi ids (one that needs more is cut); the late
    // offsets of a path 2 pass lie one behind the other as well, a group's worth for every group not counted yet
    const bool grouping = multi && groups.size() > 1 && (grouped || h->filter_exact_grouped);
    uint64_t ids_grouped = 0, ids_late = 0, n_late = 0, n_exact_groups = 0;
    for (const Group &g : groups) {
        if (g.exact) ids_grouped += g.A, n_exact_groups++;
        if (!g.exact) ids_late += g.A == UNCOUNTED ? g.A_ub : g.A;
        if (g.wb == NO_WB) n_late++;
    }
    ids_grouped = grouping ? std::max<uint64_t>({ids_grouped, std::min<uint64_t>(ids_late, 4u << 20), 1}) : 0;
    const size_t wb_lazy = ranged ? std::max<uint64_t>(1, ((src.len + 63) / 64 + 63) / 64) * (grouping ? std::max<uint64_t>(1, n_late) : 1) : 0;
    const ExactScratch x(o_xsel + align256(multi ? nq * 4 : 0), nq, n, A_max, wb_all.size() + wb_lazy, ids_grouped);
    const size_t o_out = x.end;
    const ResultBlock out(nq, n);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, pin_block ? 0 : out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(s.dev);
    void *hv = pin_block ? pin_block : s.pin;
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + o_sel), *d_xsel = reinterpret_cast<uint32_t *>(dv + o_xsel);
    uint32_t *d_mof = reinterpret_cast<uint32_t *>(dv + o_mof), *d_lo = reinterpret_cast<uint32_t *>(dv + o_lo),
             *d_hi = reinterpret_cast<uint32_t *>(dv + o_hi);
    HIP_TRY(hipMemcpyAsync(dv + o_q, Q, nq * d * 4, hipMemcpyHostToDevice, s.stream));
    if ((rc = cosine_queries(h, dv + o_q, nq, s.stream))) return rc;
    if (up_words) HIP_TRY(hipMemcpyAsync(dv + o_mask, src.masks, up_words * 8, hipMemcpyHostToDevice, s.stream));
    // (under a set the word offsets of a group go up only when a compaction of it runs)
    const ExactPlace at{dv, x, s.stream, wb_all.data(), reinterpret_cast<uint32_t *>(dv + x.o_wb), set != nullptr};
    if (!set && (bits || multi) && !wb_all.empty())
        HIP_TRY(hipMemcpyAsync(at.d_wb, wb_all.data(), wb_all.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (ranged) {
        HIP_TRY(hipMemcpyAsync(d_lo, src.lo, nq * rk * 4, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(d_hi, src.hi, nq * rk * 4, hipMemcpyHostToDevice, s.stream));
    }
    if (rowed) HIP_TRY(hipMemcpyAsync(d_mof, src.mask_of, nq * 4, hipMemcpyHostToDevice, s.stream));
    if (!gsel.empty()) HIP_TRY(hipMemcpyAsync(d_sel, gsel.data(), gsel.size() * 4, hipMemcpyHostToDevice, s.stream));
    if (multi && n_exact) HIP_TRY(hipMemcpyAsync(d_xsel, order.data(), nq * 4, hipMemcpyHostToDevice, s.stream));
    src.bind(reinterpret_cast<const float *>(dv + o_q),
             set ? set->d_rows() : up_words ? reinterpret_cast<const uint64_t *>(dv + o_mask) : nullptr,
             rowed ? d_mof : nullptr, ranged ? d_lo : nullptr, ranged ? d_hi : nullptr, n, efp);
    FilterArgs &a = src.base;
    a.qsel = gsel.empty() ? nullptr : d_sel;
    out.bind(a, dv + o_out);
    if (set) {
        // the lists of the rows planned on the exact path: a valid one is used as it is, the others are compacted
        // into the set (while its budget lasts) here, once, for this call and the ones after it
        const uint64_t budget = h->mask_set_cache_mb > 0 ? (uint64_t)h->mask_set_cache_mb << 20 : 0;
        std::vector<hnsw_mask_set::Row *> made;
        for (Group &g : groups) {
            if (!src.has_words(g.key) || src.ranged(g)) continue;  // (a row AND a range: compacted in the scratch, not the row's list)
            hnsw_mask_set::Row &r = set->rows[(size_t)g.key];
            if (!r.list_valid && g.exact && set->reserve_list(r, budget)) {
                HIP_TRY(hipMemcpyAsync(at.d_wb + g.wb, at.wbs + g.wb, g.n_wb * 4, hipMemcpyHostToDevice, s.stream));
                if ((rc = launch_filter_compact(src.args(g), (bits + 63) / 64, at.d_wb + g.wb, r.d_ids, s.stream))) return rc;
                h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
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
        HIP_TRY(hipMemcpyAsync(hv, dv + o_out, out.bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        st = out.at(hv).stats;
        return HNSW_OK;
    };
    // ONE launch of the graph path for the queries of every group planned on it, then the exact path group by group
    // (its scratch reused in stream order), then the result block in one copy
    const uint32_t range_lds = filt_range_lds(ranged, (uint32_t)rk);
    const uint32_t slots = filt_first_slots_log2(v, efp, range_lds);
    if (n_graph && (rc = launch_filtered_graph(v, a, (uint32_t)n_graph, slots, s.stream))) return rc;
    std::vector<std::vector<unsigned char>> keep;  // (the tables of the grouped passes, until the fetch has synchronised)
    if (grouping && n_exact_groups > 1) {
        std::vector<PassItem> items;
        for (const Group &g : groups)
            if (g.exact) items.push_back({g, order.data() + g.q0, d_xsel + g.q0, at.wbs + g.wb, at.d_wb + g.wb, at.send, 0});
        if ((rc = exact_grouped(src, items, at, keep))) return rc;
    } else {
        for (const Group &g : groups)
            if (g.exact && (rc = exact_group(src, g, multi ? d_xsel + g.q0 : nullptr, g.nq, at))) return rc;
    }
    uint64_t n2 = 0;
    const hnsw_query_stats *st;
    if (!n_graph) {
        if ((rc = fetch(st))) return rc;
    } else {
        // queries whose visited table filled up run again with a table twice the size, all groups together, and those
        // that fill the largest one take path 2
        rc = rerun_overflowed(
            v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v, range_lds), d_sel, s.stream, fetch,
            [&](const std::vector<uint32_t> &sel) -> int {
                return path2(src, sel, path, &groups, multi ? 0 : nq, at, d_sel, wb_all.size(), nullptr, 0, fetch, grouping);
            },
            &n2);
        if (rc != HNSW_OK) return rc;
    }
    count_call(h, src.family, n_graph - n2, n_exact, n2, groups.size());
    if (!pin_block) out.copy_out(hv, ids, dists, counts, stats);
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
            return path2(src, sel, path, nullptr, 0, ExactPlace{nullptr, ExactScratch(), stream, nullptr, nullptr, true},
                         nullptr, 0, &lease, pin_bytes, fetch, h->filter_exact_grouped != 0);
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
