// filter_plan.cpp -- the planner of a filtered search: a call's queries cut into groups, every group counted.  Host
// arithmetic over the caller's words, a resident set's caches and the label column; no call into the device runtime.

#include "filter_plan.h"

#include <algorithm>
#include <map>
#include <utility>

namespace hx {

namespace {

// The walk over a mask's words below `bits`: the last word's tail is masked, the deleted ids are cleared, and before
// every block of 64 words the admissible ids so far are noted in wbase (the compaction kernel's offsets).
// count(w, x) -> how many of the bits left in word w are admissible, or UNCOUNTED: the walk ends there with UNCOUNTED
template <class Count>
uint64_t walk_words(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase, Count count) {
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
        const uint64_t c = count(w, x);
        if (c == UNCOUNTED) return UNCOUNTED;
        A += c;
    }
    return A;
}

}  // namespace

uint64_t count_admissible(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase) {
    return walk_words(h, allow, bits, wbase, [](uint64_t, uint64_t x) { return (uint64_t)__builtin_popcountll(x); });
}

void bind_labels(const hnsw_index *h, FilterArgs &a) {
    a.labels = h->lab.d_labels();
    a.label_len = std::min<uint64_t>(h->lab.labels.size(), 2 * h->lab.d_cap);
}

int check_filter(const Filter &f) {
    if (f.K <= (f.rows == Filter::ALL ? (uint32_t)HX_FILT_MAX_RANGES : f.rows == Filter::SET ? 1u : 0u)) return HNSW_OK;
    set_error("filtered search: no search under these rows and %u label ranges per query", f.K);
    return HNSW_ERR_ARG;
}

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

int FilterSource::check_rows(uint64_t nq, uint64_t allow_bits) const {
    bool masked = false;
    for (uint64_t i = 0; rowed && i < nq; i++) {
        if (mask_of[i] == HNSW_MASK_NONE) continue;
        if (mask_of[i] >= n_masks) {
            set_error("filtered search: query %llu names mask %u of %u", (unsigned long long)i, mask_of[i], n_masks);
            return HNSW_ERR_ARG;
        }
        masked = true;
    }
    if (masked && !set && !masks && allow_bits != 0) {
        set_error("filtered search: needs the masks its queries name when allow_bits > 0");
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

FilterSource::FilterSource(hnsw_index *h_, const Filter &f)
    : h(h_), family(f.family), set(f.rows == Filter::SET ? f.set : nullptr),
      masks(f.rows == Filter::ONE || f.rows == Filter::MANY ? f.masks : nullptr),
      rowed(f.rows == Filter::MANY || f.rows == Filter::SET), K(f.K), n_masks(set ? set->n_masks : f.n_masks),
      len(index_len(h_)) {
    const uint64_t allow_bits = set ? set->allow_bits : f.rows == Filter::ALL ? len : f.allow_bits;
    bits = std::min<uint64_t>(allow_bits, len);
    row_words = (allow_bits + 63) / 64;
    if (!f.on_device) mask_of = f.mask_of, lo = f.lo, hi = f.hi;
}

void FilterSource::intern(uint64_t nq) {
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

void FilterSource::bind(const float *d_Q, const uint64_t *d_allow, const uint32_t *d_mask_of, const uint32_t *d_lo,
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

FilterArgs FilterSource::shared_args() const {
    FilterArgs a = base;
    a.mask_of = nullptr;
    a.allow = nullptr;
    a.range_lo = a.range_hi = nullptr;
    a.lo = a.hi = 0;
    a.n_ranges = 0;
    return a;
}

FilterArgs FilterSource::args(const Group &g) const {
    FilterArgs ax = shared_args();
    const uint64_t m0 = ranged(g) ? members_of(g)[0] : 0;  // (the first member; one member: the launch's whole range)
    ax.allow = has_words(g.key) ? base.allow + g.key * row_words : nullptr;
    ax.allow_bits = bound(g.key);
    if (!ranged(g)) ax.labels = nullptr;  // (a plain row next to ranged groups: the compaction reads its words alone)
    ax.lo = (uint32_t)(m0 >> 32), ax.hi = (uint32_t)m0;  // (the group's range as scalars)
    return ax;
}

RangeList FilterSource::range_list(const Group &g) const {
    RangeList r{};
    if (!ranged(g) || n_members(g) < 2) return r;
    r.n = (uint32_t)n_members(g);
    for (uint32_t j = 0; j < r.n; j++) r.lo[j] = (uint32_t)(members_of(g)[j] >> 32), r.hi[j] = (uint32_t)members_of(g)[j];
    return r;
}

FilterSource::Locks FilterSource::lock() const {
    Locks l;
    if (set) l.set = std::unique_lock<std::mutex>(set->mu);
    if (K) l.lab = std::unique_lock<std::mutex>(h->lab.mu);
    return l;
}

uint64_t FilterSource::count_both(uint32_t row, uint32_t lo, uint32_t hi, int64_t limit, std::vector<uint32_t> &wbase,
                                  uint64_t &A_ub) const {
    uint64_t first = 0;
    const uint64_t S = h->lab.count(lo, hi, &first), RA = set->counted(h, row).A;
    A_ub = std::min(S, RA);
    const uint64_t *w = set->row_words(row);
    uint64_t A = 0;
    if (S > RA)  // the row's set bits, testing labels
        return walk_words(h, w, bits, wbase, [&](uint64_t ww, uint64_t x) {
            uint64_t c = 0;
            for (; x; x &= x - 1) {
                if (h->lab.get(ww * 64 + (uint64_t)__builtin_ctzll(x)) - lo > hi - lo) continue;
                if ((int64_t)++A > limit) return UNCOUNTED;
                c++;
            }
            return c;
        });
    const uint64_t n_words = (bits + 63) / 64, n_wblk = std::max<uint64_t>(1, (n_words + 63) / 64);
    wbase.assign(n_wblk + 1, 0);  // ids per block, shifted by one
    for (uint64_t i = first; i < first + S; i++) {
        const uint32_t id = (uint32_t)h->lab.sorted[i];
        if (id >= bits || ((w[id >> 6] >> (id & 63)) & 1ull) == 0) continue;
        if ((int64_t)++A > limit) return UNCOUNTED;
        wbase[(id >> 12) + 1]++;
    }
    for (size_t b = 1; b < wbase.size(); b++) wbase[b] += wbase[b - 1];
    wbase.pop_back();
    return A;
}

void FilterSource::resolve(Group &g, int64_t exact_max, std::vector<uint32_t> &wbs) const {
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
    g.off.at = wbs.size();
    g.off.n = wb->size();
    wbs.insert(wbs.end(), wb->begin(), wb->end());
}

uint64_t FilterSource::n_groups(uint64_t nq) const {
    if (!(rowed && mask_of)) return n_lists();
    std::vector<std::pair<uint64_t, uint64_t>> named(nq);  // (a row per query: K == 1, the pair is the list)
    for (uint64_t i = 0; i < nq; i++) named[i] = {mask_of[i], raw(i)};
    std::sort(named.begin(), named.end());
    return (uint64_t)(std::unique(named.begin(), named.end()) - named.begin());
}

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

}  // namespace hx
