// filter_exact.cpp -- the exact path of a filtered search, per group and grouped, and path 2.  The kernels are
// search_filtered.hip; what a group is and how it was counted is filter_plan.cpp's.

#include "filter_exact.h"

namespace hx {

// One compaction of the group's admissible ids into the scratch (under its range list when it is the union of several
// label ranges) -- or none: a resident set's cached list is scanned as it is, its offsets are not read -- then the scan
// and merge, 65535 queries per launch
int exact_group(const FilterSource &src, const Group &g, const uint32_t *d_sel, uint64_t shape_nsel, const ExactPlace &at) {
    const DevView &v = src.h->dev.view;
    const FilterArgs a = src.args(g);
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(shape_nsel, 65535), nseg = filt_exact_segments(g.A, chunk);
    const uint32_t *d_ids = g.d_list;
    int r = HNSW_OK;
    if (!g.d_list) {  // a row beyond the set's budget, or no row of the set
        if (g.off.send) {
            HIP_TRY(hipMemcpyAsync(g.off.dev, g.off.host, g.off.n * 4, hipMemcpyHostToDevice, at.stream));
            src.count_compaction(g);
        }
        const RangeList ranges = src.range_list(g);
        uint32_t *d_scratch_ids = reinterpret_cast<uint32_t *>(at.dv + at.x.o_ids);
        r = launch_filter_compact(a, (a.allow_bits + 63) / 64, g.off.dev, d_scratch_ids, at.stream, &ranges);
        d_ids = d_scratch_ids;
    }
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
        r = launch_filtered_exact(v, ac, (uint32_t)std::min<uint64_t>(chunk, g.nq - c), d_ids, (uint32_t)g.A, nseg,
                                  reinterpret_cast<unsigned long long *>(at.dv + at.x.o_part),
                                  reinterpret_cast<int32_t *>(at.dv + at.x.o_pst), at.stream);
    }
    return r;
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
int exact_grouped(const FilterSource &src, const std::vector<PassItem> &items, const ExactPlace &at,
                  std::vector<std::vector<unsigned char>> &keep) {
    const DevView &v = src.h->dev.view;
    uint64_t total = 0;
    for (const PassItem &it : items) total += it.g.nq;
    const uint32_t shape = (uint32_t)std::min<uint64_t>(total, 65535);
    uint32_t *d_ids0 = reinterpret_cast<uint32_t *>(at.dv + at.x.o_ids);
    auto compacts = [](const Group &g) { return !g.d_list && g.A > 0; };
    size_t i0 = 0;
    while (i0 < items.size()) {
        // the pass: as many groups from i0 as the launch limits and the rooms take
        uint64_t nsel = 0, rows = 0, ids = 0;
        size_t i1 = i0;
        for (; i1 < items.size(); i1++) {
            const Group &g = items[i1].g;
            const uint64_t r = g.nq * filt_exact_segments(g.A, shape), a = compacts(g) ? g.A : 0;
            if (nsel + g.nq > 65535 || rows + r > std::min<uint64_t>(at.x.rows_cap, HX_FILT_MAX_PART_ROWS - 1) || ids + a > at.x.ids_cap) break;
            nsel += g.nq, rows += r, ids += a;
        }
        if (i1 == i0) {  // a group no pass takes: by itself, in the per-group form
            const PassItem &it = items[i0++];
            if (int r = exact_group(src, it.g, it.d_sel, it.g.nq, at)) return r;
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
        // the spans of host offsets that go up, one copy per host array (the planner's, path 2's): a span may cover the
        // offsets of groups that need none, and the groups' places on the device mirror the array
        const uint32_t *send_lo[2] = {nullptr, nullptr}, *send_hi[2] = {nullptr, nullptr};
        uint32_t *send_to[2] = {nullptr, nullptr};
        for (size_t i = i0; i < i1; i++) {
            const Group &g = items[i].g;
            const uint32_t nseg = filt_exact_segments(g.A, shape);
            const uint32_t *list = g.d_list ? g.d_list : d_ids0 + at_id;
            max_nseg = std::max(max_nseg, nseg);
            if (compacts(g)) {
                const FilterArgs ax = src.args(g);
                if (g.off.send) {
                    const int f = g.off.late;
                    if (!send_lo[f] || g.off.host < send_lo[f]) send_lo[f] = g.off.host, send_to[f] = g.off.dev;
                    if (!send_hi[f] || g.off.host + g.off.n > send_hi[f]) send_hi[f] = g.off.host + g.off.n;
                    src.count_compaction(g);
                }
                if (src.range_list(g).n <= 1) {  // (K > 1 ranges: a launch of its own, after the offsets are up, below)
                    ExactGroup &e = gt[ngt++];
                    e.allow = ax.allow;
                    e.word_base = g.off.dev;
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
                sel[y] = items[i].sel[k];
                row += nseg;
            }
        }
        unsigned char *d_tab = at.dv + at.x.o_tab;
        HIP_TRY(hipMemcpyAsync(d_tab, blob, o_gt + ngt * sizeof(ExactGroup), hipMemcpyHostToDevice, at.stream));
        for (int f = 0; f < 2; f++)
            if (send_lo[f])
                HIP_TRY(hipMemcpyAsync(send_to[f], send_lo[f], (size_t)(send_hi[f] - send_lo[f]) * 4, hipMemcpyHostToDevice, at.stream));
        FilterArgs a = src.shared_args();  // what the groups share; a group's row and range are in its record
        a.qsel = reinterpret_cast<const uint32_t *>(d_tab + o_sel);
        int r = launch_filter_compact_grouped(a, reinterpret_cast<const ExactGroup *>(d_tab + o_gt), ngt, max_words, at.stream);
        at_id = 0;
        for (size_t i = i0; r == HNSW_OK && i < i1; i++) {
            const Group &g = items[i].g;
            if (!compacts(g)) continue;
            const RangeList ranges = src.range_list(g);
            if (ranges.n > 1) {
                const FilterArgs ax = src.args(g);
                r = launch_filter_compact(ax, (ax.allow_bits + 63) / 64, g.off.dev, d_ids0 + at_id, at.stream, &ranges);
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

// The host form comes with its arena laid out up front, because the queries and the result block live in it, and
// nothing is allocated; a device form sizes [selection | exact scratch] in its lease only now.  A late group's offsets
// go up just before its launches: to the one room when the groups run one by one (the scratch is reused in stream
// order), one behind the other, as in wb_late, when they run as one pass.
int path2(const FilterSource &src, const std::vector<uint32_t> &sel, std::vector<uint8_t> &path,
          const std::vector<Group> *planned, uint64_t shape_nsel, bool grouping,
          const std::function<int(const Path2Need &, Path2Place &)> &place, const std::function<int()> &fetch) {
    std::vector<uint32_t> sel2 = sel, wb_late;
    std::vector<Group> runs = group_by_key(sel2, src);
    for (uint32_t i : sel) path[i] = 2;
    FilterSource::Locks lock;  // (a set's stays until the end: its lists are read by the launches)
    Path2Need need{sel2.size(), 0, 0, 0, 0, grouping && runs.size() > 1};
    for (Group &g : runs) {
        if (planned) {
            const Group &p = *std::lower_bound(planned->begin(), planned->end(), g,
                                               [](const Group &x, const Group &y) { return group_before(x, y.key, y.list); });
            g.A = p.A, g.off = p.off, g.d_list = p.d_list;
        }
        if (!g.off.counted()) {
            if (!lock.held()) lock = src.lock();
            src.resolve(g, INT64_MAX, wb_late);
            g.off.late = true;
        }
        need.A_max = std::max(need.A_max, g.A);
        need.A_sum += g.d_list ? 0 : g.A;
        need.n_wb = std::max(need.n_wb, g.off.n);
    }
    need.n_wb_late = wb_late.size();
    if (lock.lab.owns_lock()) lock.lab.unlock();  // (the column's: never across a sync)
    Path2Place p{};
    int r = place(need, p);
    if (r != HNSW_OK) return r;
    for (Group &g : runs)  // (wb_late is final)
        if (g.off.late) g.off.bind(wb_late.data(), p.d_late + (need.grouping ? g.off.at : 0), true);
    HIP_TRY(hipMemcpyAsync(p.d_sel, sel2.data(), sel2.size() * 4, hipMemcpyHostToDevice, p.at.stream));
    std::vector<std::vector<unsigned char>> keep;
    if (need.grouping) {  // one more pass of the grouped form
        std::vector<PassItem> items;
        for (const Group &g : runs) items.push_back({g, sel2.data() + g.q0, p.d_sel + g.q0});
        r = exact_grouped(src, items, p.at, keep);
    } else {
        for (size_t k = 0; r == HNSW_OK && k < runs.size(); k++)
            r = exact_group(src, runs[k], p.d_sel + runs[k].q0, shape_nsel ? shape_nsel : runs[k].nq, p.at);
    }
    if (r != HNSW_OK) return r;
    return fetch();  // (synchronises: `sel2`, `wb_late` and the tables live until then)
}

}  // namespace hx
