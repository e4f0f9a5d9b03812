// filter_exact.h -- the exact path of a filtered search (filter_exact.cpp): a group's admissible ids compacted into a
// list and scanned, group by group or many groups in one pass, and path 2, which answers by it the queries that filled
// the graph path's largest visited table (internal)
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "filter_plan.h"

namespace hx {

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
    uint32_t *d_wb(unsigned char *dv) const { return reinterpret_cast<uint32_t *>(dv + o_wb); }
};

// Where a call's exact path runs: a device arena with its scratch, and a stream.  (Where a group's word offsets are is
// the group's to say: Group::off.)
struct ExactPlace {
    unsigned char *dv;
    ExactScratch x;
    hipStream_t stream;
};

// The exact path for the g.nq queries of one group: those of d_sel, or the first g.nq of the call.  shape_nsel: the
// query count the launch shape (queries per launch, segments) is chosen for.  A group with a resident set's cached
// list is scanned from it; any other is compacted into the scratch from its word offsets, which go up first when they
// are not there yet (under a set, where most groups have a list and need none)
int exact_group(const FilterSource &src, const Group &g, const uint32_t *d_sel, uint64_t shape_nsel, const ExactPlace &at);

// a group in a pass of the grouped form, with its queries on the host and on the device (read when the group has to go
// by itself)
struct PassItem {
    const Group &g;
    const uint32_t *sel, *d_sel;
};
// The grouped form: the groups of `items` in as few passes as the launch limits and the rooms
// allow.  keep: the passes' tables, which the copies read until the stream is synchronised
int exact_grouped(const FilterSource &src, const std::vector<PassItem> &items, const ExactPlace &at,
                  std::vector<std::vector<unsigned char>> &keep);

// Path 2: the queries of `sel` filled the largest visited table and are answered by the exact path, each under its own
// filter, then `fetch`, which synchronises.  Its groups are looked up in `planned` (ascending key: the host form's
// plan; nullptr: a device form, which has counted nothing); a group that is not counted yet -- every group of a device
// form, a graph-planned range of the host form -- is counted here, and only then is it known what room the pass needs:
// `place` gets that and says where it runs.
struct Path2Need {
    uint64_t nsel, A_max, A_sum;  // its queries; the longest list, and all lists that have to be compacted
    size_t n_wb, n_wb_late;       // the most word offsets of one group; those of all late groups
    bool grouping;                // it runs as one pass of the grouped form (two or more groups, and the caller asks for it)
};
struct Path2Place {
    ExactPlace at;
    uint32_t *d_sel;   // room for the selection
    uint32_t *d_late;  // ... and for the late groups' word offsets: one group's, or n_wb_late under `grouping`
};
int path2(const FilterSource &src, const std::vector<uint32_t> &sel, std::vector<uint8_t> &path,
          const std::vector<Group> *planned, uint64_t shape_nsel, bool grouping,
          const std::function<int(const Path2Need &, Path2Place &)> &place, const std::function<int()> &fetch);

}  // namespace hx
