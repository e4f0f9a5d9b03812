// filter_plan.h -- the planner of a filtered search (filter_plan.cpp): the groups of a call, how many ids each admits,
// and what the exact path needs to know of a group.  Host arithmetic only: nothing here touches the device (internal)
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "search_host.h"

namespace hx {

// ---- the filter of a call --------------------------------------------------------------------------------------
// A query's filter is named by a key and a list.  The key: the query's row (or HNSW_MASK_NONE) in a call with a row per
// query, 0 otherwise.  The list: the index of the query's canonical range list in the call's table of them
// (FilterSource::intern), NO_LIST in a call without label ranges: two raw lists with one canonical form are one list.
// The queries under one (key, list) are a group: the planner's unit, and that of the exact path's launches.
constexpr uint64_t UNCOUNTED = ~0ull;
constexpr uint64_t FULL_RANGE = 0xFFFFFFFFull;  // [0, UINT32_MAX]
constexpr uint32_t NO_LIST = ~0u;
constexpr size_t NO_WB = ~(size_t)0;

// Where a group's word offsets (the admissible ids before every block of 64 words, the compaction's input) are, said
// once.  `resolve` appends them to a list that still grows, so it notes an index; once the list is final they are bound
// to their places (bind), and from then on the exact path reads the pointers alone.
struct WordOffsets {
    size_t at = NO_WB, n = 0;       // in the list they were counted into (NO_WB: not counted yet)
    const uint32_t *host = nullptr; // bound: on the host ...
    uint32_t *dev = nullptr;        // ... and their place on the device
    bool send = false;              // they are not there yet and go up just before the group's compaction
    bool late = false;              // counted by path 2 (its list), not by the planner (the call's)
    bool counted() const { return at != NO_WB; }
    void bind(const uint32_t *list, uint32_t *d_place, bool send_) { host = list + at, dev = d_place, send = send_; }
};

struct Group {
    uint64_t key = 0;
    uint32_t list = NO_LIST;
    size_t q0 = 0, nq = 0;             // its queries: [q0, q0 + nq) of the sorted list it was cut from
    uint64_t A = UNCOUNTED;            // admissible ids (a row AND a range planned on the graph path: not counted, at most A_ub)
    uint64_t A_ub = 0;
    bool exact = false;                // A <= filter_exact_max: planned on the exact path
    WordOffsets off;
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

    FilterSource(hnsw_index *h_, const Filter &f);

    bool interned() const { return !start.empty(); }
    size_t n_lists() const { return start.size() - 1; }
    uint64_t raw(uint64_t i) const { return ((uint64_t)lo[i] << 32) | hi[i]; }
    void intern(uint64_t nq);

    // a host-pointer call of nq queries: every row a query names exists, and the rows came with their words
    int check_rows(uint64_t nq, uint64_t allow_bits) const;
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
              const uint32_t *d_hi, uint32_t n, uint32_t efp);
    // what the launches of the exact path share: base without a row, a range or a row and ranges per query
    FilterArgs shared_args() const;
    // the arguments of an exact-path launch: the group's row, its ranges, or both, alone
    FilterArgs args(const Group &g) const;
    // ... and its canonical list, by value, for the compaction (n == 0: the group is under args' lo / hi alone)
    RangeList range_list(const Group &g) const;
    // a compaction of g into the scratch or the set is about to run: counted when it is a plain row of a set
    void count_compaction(const Group &g) const {
        if (set && has_words(g.key) && !ranged(g)) h->n_set_compactions.fetch_add(1, std::memory_order_relaxed);
    }

    // What `resolve` reads is locked by this: a set's caches (a row is counted when it, the deleted set or the length
    // changed), and the label column's sorted copy (made under the lock, by the first group that has a range, when the
    // column, the deleted set or the length changed).  The set's first, then the column's
    struct Locks {
        std::unique_lock<std::mutex> set, lab;
        bool held() const { return set.owns_lock() || lab.owns_lock(); }
    };
    Locks lock() const;
    // The admissible ids of a row AND a range: the undeleted ids below `bits` whose bit is set in the row and whose
    // label lies in [lo, hi].  Neither side's count says how many: the cheaper side is walked -- the range's slice of
    // the sorted copy (undeleted ids already) testing the row's bits, or the row's set bits testing labels -- and only
    // while the count stays within `limit`: beyond it the group is on the graph path and the count is not needed
    // (UNCOUNTED; A_ub, the smaller side, bounds it).  The same walk gives the compaction's offsets, the admissible ids
    // before every block of 64 words.  The row's own cached count is read; its offsets and its list are the row's alone
    uint64_t count_both(uint32_t row, uint32_t lo, uint32_t hi, int64_t limit, std::vector<uint32_t> &wbase, uint64_t &A_ub) const;
    // Counts a group: A (kept when it is known already), exact = A <= exact_max, a set row's list while it is valid, and
    // its word offsets, appended to wbs.  The admissible ids of a range list are its disjoint members' slices of the
    // sorted copy, each found by two binary searches: A is their sum; the offsets cost a pass over the slices and are
    // counted only when the group is exact.  A row AND a range are counted by count_both, up to exact_max
    void resolve(Group &g, int64_t exact_max, std::vector<uint32_t> &wbs) const;
    // the distinct groups of the call's nq queries, for its counters (a device-pointer call's, which cuts no groups)
    uint64_t n_groups(uint64_t nq) const;
};

// the column as the kernels see it (after its HBM copy is brought up to date: at least the index length; never more
// than the copy holds)
void bind_labels(const hnsw_index *h, FilterArgs &a);

// stable-sorts query indices by (key, list) and cuts them into runs: ascending key (HNSW_MASK_NONE last among rows),
// ascending list within a key, the caller's order within a run
inline bool group_before(const Group &g, uint64_t key, uint32_t list) { return g.key != key ? g.key < key : g.list < list; }
std::vector<Group> group_by_key(std::vector<uint32_t> &idx, const FilterSource &src);

// the combinations of rows and ranges no entry point offers (search_host.h's table)
int check_filter(const Filter &f);

// The counters of a call that ended well, by the entry points that made it: its queries per path under filtered_* or
// deleted_*, the call itself, and its groups
void count_call(hnsw_index *h, Filter::Family family, uint64_t n_graph, uint64_t n_exact, uint64_t n_overflow, uint64_t n_groups);

}  // namespace hx
