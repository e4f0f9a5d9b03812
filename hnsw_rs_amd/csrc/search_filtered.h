// search_filtered.h -- filtered k-NN (hnsw_search_batch_filtered): the arguments of the kernels in
// search_filtered.hip and their launchers.  gfx950 only.
//
// An allow-list is a bitmask over ids: id i is allowed iff i < allow_bits and bit i & 63 of word i >> 6 is set
// (allow_bits is already clamped to the index length by the caller); without a mask (allow == nullptr) every id
// below allow_bits is.  One mask serves the call (mask_of == nullptr), or allow holds rows of mask_words words
// and query q walks under row mask_of[q] (hnsw_search_batch_filtered_multi); HNSW_MASK_NONE there means no mask:
// every id below none_bits.  The rows may be a resident mask set's (mask_set.h), and mask_of may then come from the
// caller's device memory, unseen by the host: the graph kernel checks it against n_masks and answers a query that
// names a row beyond it with status HNSW_ERR_ARG before it reads a mask word.  Only the graph kernel reads mask_of: the
// exact path's kernels are launched per mask with allow at that mask's row, or, in the grouped form (ExactGroup, below), once
// for all masks with every group's row in its record.  The handle's deleted set (hnsw_mark_deleted) is a second mask of
// the same layout, deny: an id is admissible iff it is allowed and not denied.
//
// A label range (hnsw_search_batch_filtered_range) is a third filter, in place of the allow-list: labels is the handle's
// resident label column (labels.h), one uint32 per id, and id i is allowed iff i < allow_bits and lo <= label(i) <= hi,
// where label(i) is labels[i] for i < label_len and 0 beyond it (the host keeps label_len at or above the index length,
// with zeros beyond the labels that were set: the graph kernel has one bound for the id and for the label read).  The
// graph kernel's wave takes its query's range from range_lo[q] / range_hi[q] (they may be the caller's device memory);
// the exact path's kernels are launched per range with the scalars lo and hi.  lo > hi is an empty range: nothing is allowed and no label is read.
//
// A call may have a column AND the rows of a resident set (hnsw_search_batch_filtered_set_range): id i is then allowed iff
// i < allow_bits, lo <= label(i) <= hi and its bit is set in the query's row; a HNSW_MASK_NONE query has no bit test and
// the bound none_bits.  The graph kernel's wave picks its row by mask_of[q] as in a call with rows alone and keeps the
// row's pointer next to its range; the compaction of an exact-path launch ANDs allow's word onto the word it made from
// the labels (allow == nullptr there: the range alone).
//
// A query may be under SEVERAL ranges (hnsw_search_batch_filtered_ranges; n_ranges = K > 1, and no rows): id i is then
// allowed iff i < allow_bits and label(i) lies in at least one of [range_lo[q K + j], range_hi[q K + j]], j < K.  A member
// with lo > hi is empty; the members may overlap and come in any order (the caller's device memory, as it is).  The
// graph kernel's wave keeps its K members in LDS behind its 16-byte slot, an empty one replaced by a copy of one that is
// not (harmless under any-of; all empty: the id bound 0, as an empty range has today).  An exact-path launch gets its
// list by value (RangeList: n members, disjoint and none of them empty: the host's canonical form), and the
// compaction's word is made from `label in any of them`.  The list is the compaction kernel's own argument, not a part
// of FilterArgs: see n_ranges there.
#pragma once

#include "device_index.h"

namespace hx {

#define HX_FILT_MAX_EF 256  // ef' on the graph path: F and R are four registers per lane at most
#define HX_FILT_MAX_N 64    // results per query (both paths)
#define HX_FILT_RANGE_LDS 16  // bytes of LDS a wave under a label range keeps its range in (lo, hi - lo, its mask row's pointer)
#define HX_FILT_MAX_RANGES 16   // members of a query's range list (HNSW_RANGES_MAX); each keeps 8 bytes more (lo, hi - lo)
#define HX_FILT_MAX_SLOTS_LOG2 15  // the largest visited table: 32768 slots, at most 24576 ids (75 %)

struct FilterArgs {
    const float *Q;            // nq x dim (device)
    const uint32_t *qsel;      // optional: launch block b serves query qsel[b]
    const uint64_t *allow;     // mask words (device), or nullptr: every id < allow_bits
    uint64_t allow_bits;       // min(caller's allow_bits, index length)
    const uint32_t *mask_of;   // optional (device): query q's row of allow, or HNSW_MASK_NONE; nullptr: row 0
    uint64_t mask_words;       // words per row of allow (read with mask_of only)
    uint64_t none_bits;        // the id bound of a HNSW_MASK_NONE query: the index length
    const uint64_t *deny;      // the deleted ids' mask words (device), or nullptr: nothing deleted
    uint64_t deny_bits;        // ids the deny mask covers (a multiple of 64); ids beyond it are not denied
    uint32_t n, ef;            // results per query, ef' = max(ef, n, 1)
    uint32_t n_masks;          // rows of allow (read with mask_of only): a mask_of entry is below it or HNSW_MASK_NONE
    // K > 1: the graph kernel's query q is under the K ranges range_lo / range_hi [q K, q K + K); <= 1: under the one
    // range [q].  (Here, in what was padding: the struct is the kernels' argument block, and the 128d graph kernel
    // loses a wave of occupancy when it grows)
    uint32_t n_ranges;
    const uint32_t *labels;    // the label column (device), or nullptr: the call has no label range
    uint64_t label_len;        // labels the column holds; an id at or beyond it has label 0
    const uint32_t *range_lo;  // with labels, the graph kernel (device): query q is under [range_lo[q], range_hi[q]] ...
    const uint32_t *range_hi;
    uint32_t lo, hi;           // ... and the compaction of an exact-path launch under [lo, hi]
    uint32_t *out_ids;         // nq x n
    float *out_dists;          // nq x n
    uint32_t *out_counts;      // nq
    hnsw_query_stats *out_stats;  // nq
};

// The range list of an exact-path launch under several ranges (by value: the launch needs no allocation or copy);
// n <= 1: the launch is under FilterArgs::lo / hi alone
struct RangeList {
    uint32_t n = 0;
    uint32_t lo[HX_FILT_MAX_RANGES], hi[HX_FILT_MAX_RANGES];
};

// The second source form of hx_filt_merge_kernel (hnsw_merge_topk_device): instead of the nseg partial key lists of one
// index, the result lists of n_shards indexes, shard-major -- ids[s][q][j] (ids local to shard s, pad UINT32_MAX),
// dists[s][q][j], counts[s][q] (nullptr: an entry is present iff its id is not the pad) and stats[s][q] (nullptr: none
// are summed or written).  A present entry's key is (dist bits << 32) | (base[s] + stride[s] * id); the query's n smallest
// distinct keys are written as the exact path writes them.  base and stride travel by value: the launch needs no
// allocation, copy or synchronisation.  ids == nullptr: the kernel's first form.
//
// The third source form (hnsw_group_by_label_device), selected by per_group != 0 -- not by
// `labels`, which may be nullptr (label_len 0: every label is 0): ONE candidate list per query, ids[q][j] / dists[q][j],
// j < pool, counts[q] and stats[q] as above (n_shards, base and stride are not read), collapsed by label into the
// n_groups nearest groups of at most per_group entries each.  Nothing is sorted: the collapse is defined by position.
// The ids and distances go to FilterArgs::out_ids / out_dists as [q][n_groups][per_group], the number of groups to
// out_counts, the query's stats record to out_stats unchanged, the groups' labels and sizes to group_labels /
// group_sizes [q][n_groups].  FilterArgs::n is not read.
//
// The fourth source form (hnsw_radius_cut_device), selected by cut_out != 0 next to ids (zero in
// every other launch): ONE candidate list per query, ids[q][j] / dists[q][j], j < pool, counts[q] and stats[q] as above,
// cut at radius[q] -- the present entries with dist <= radius[q] (an f32 compare: a NaN on either side keeps nothing), in
// their input order, to FilterArgs::out_ids / out_dists as [q][cut_out], padded behind; their number to out_counts, the
// stats record to out_stats unchanged, HX_RADIUS_MORE to flags[q] iff the status is HNSW_OK, all pool entries are
// present and all of them were kept.  Block b serves query FilterArgs::qsel[b] when that is set (an entry at or beyond
// nq is not served); the rows of other queries are not touched.  Nothing is sorted and no LDS is used.
//
// The fifth source form (hnsw_drop_ids_device), selected by drop_out != 0 next to ids (zero in every
// other launch): ONE candidate list per query, ids[q][j] / dists[q][j], j < pool, counts[q] and stats[q] as above, and
// ex[q][s], s < ex_width -- THE DROP of include/hnsw_mi355x.h: the present entries whose id equals no present exclusion
// id, in their input order, the first drop_out of them to FilterArgs::out_ids / out_dists as [q][drop_out], padded
// behind; the number written to out_counts, the present entries removed over all of pool to dropped[q], the stats record
// to out_stats unchanged unless src_status[q] is not HNSW_OK: then the query has no present entry and the record carries
// that status.  FilterArgs::qsel is honoured as in the cut form.  Nothing is sorted and no LDS is used.
#define HX_DROP_MAX_WIDTH 64      // exclusion ids per query: one lane each
#define HX_MERGE_MAX_SHARDS 64
#define HX_GROUP_POOL_MAX 256     // candidates per query: four per lane
#define HX_GROUP_SLOTS_MAX 1024   // n_groups x per_group: the slot table in LDS
#define HX_RADIUS_MAX_N 1024      // entries per list of the cut: a search's register-resident list
#define HX_RADIUS_MORE 1u
struct MergeLists {
    const uint32_t *ids;
    const float *dists;
    const uint32_t *counts;
    const hnsw_query_stats *stats;
    uint32_t n_shards, nq;
    uint32_t base[HX_MERGE_MAX_SHARDS], stride[HX_MERGE_MAX_SHARDS];
    const uint32_t *labels;   // the label column (device), or nullptr
    uint64_t label_len;       // labels the column holds; an id at or beyond it has label 0
    uint32_t pool, n_groups, per_group;
    uint32_t cut_out;         // != 0: the cut form, and the stride of its output rows (pool <= cut_out)
    uint32_t *group_labels, *group_sizes;
    const float *radius;      // the cut form: nq radii (device)
    uint32_t *flags;          // the cut form: nq flag words, or nullptr
    // the drop form (drop_out != 0; zero in every other launch, which reads nothing below)
    const uint32_t *ex;         // nq x ex_width exclusion ids (device), pad UINT32_MAX
    const int32_t *src_status;  // nq compose statuses (device), or nullptr
    uint32_t *dropped;          // nq words: present entries removed by the exclusion, or nullptr
    uint32_t drop_out;          // != 0: the drop form, and the stride of its output rows (drop_out <= pool)
    uint32_t ex_width;          // exclusion slots per query, 1 .. HX_DROP_MAX_WIDTH: one lane each
};

// The grouped form of the exact path: the exact-path groups of a call in ONE compaction, ONE scan
// and ONE merge launch.  What differs from group to group travels in two device tables instead of the kernels' scalars;
// with a nullptr table every kernel is the per-group form above.
//   ExactGroup, one per compacted group (the compaction's blockIdx.y): the group's row of mask words (nullptr: none), its
//   id bound, its label range (ranged == 0: the group has no range and no label is read), its word offsets and the list
//   it writes.  A block at or beyond the group's words exits.
//   ExactQuery, one per selected query (the scan's blockIdx.y, the merge's blockIdx.x): the list its group's admissible
//   ids are in (compacted by this call, or a resident set's cached one), A, and where its partial lists are: nseg of them
//   from row `part` of the call's partial keys and statuses, packed as (part << 9) | nseg (nseg <= 256, part < 2^23).  A
//   scan block whose segment is at or beyond nseg exits.
struct ExactGroup {
    const uint64_t *allow;
    const uint32_t *word_base;
    uint32_t *ids;
    uint64_t allow_bits;
    uint32_t lo, hi;
    uint32_t ranged, pad;
};
struct ExactQuery {
    const uint32_t *ids;
    uint32_t A;
    uint32_t seg;
};
static_assert(sizeof(ExactQuery) == 16 && sizeof(ExactGroup) == 48, "the tables' records are read as they are laid out here");
#define HX_FILT_SEG_BITS 9
#define HX_FILT_MAX_PART_ROWS (1u << (32 - HX_FILT_SEG_BITS))

// ids a layer-0 visited table of 2^slots_log2 slots holds before the graph path reports HNSW_ERR_OVERFLOW
__host__ __device__ inline uint32_t filt_visited_limit(uint32_t slots_log2) { return (1u << slots_log2) - (1u << (slots_log2 - 2)); }
// first table size for ef' (the generic kernel's choice) and the largest one the dimension leaves room for in LDS
// (range_lds: the bytes a wave keeps its range or ranges in, filt_range_lds; 0 for a call without a label column)
inline uint32_t filt_range_lds(bool ranged, uint32_t n_ranges = 1) {
    return ranged ? HX_FILT_RANGE_LDS + (n_ranges > 1 ? 8u * n_ranges : 0u) : 0u;
}
uint32_t filt_first_slots_log2(const DevView &v, uint32_t ef, uint32_t range_lds = 0);
uint32_t filt_max_slots_log2(const DevView &v, uint32_t range_lds = 0);

// graph path: `nblocks` queries (a.qsel selects them when set); a query whose visited table fills up ends with
// status HNSW_ERR_OVERFLOW and is run again by the caller with a larger table or answered by the exact path
int launch_filtered_graph(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2,
                          hipStream_t stream);
// exact path, step 1: the ascending list of admissible ids (a.allow, a.allow_bits, a.deny, a.deny_bits) in the
// n_words words below allow_bits; with a.labels, "allowed" is the range [a.lo, a.hi] over the column and the kernel
// makes the words itself (and ANDs a.allow's onto them when that is set as well).  word_base[b] = admissible ids in words [0, 64 b) (computed by the caller, who counts A
// anyway); ids[A]
// ; list (optional, with a.labels and without a.allow): the ids whose label lies in any of its ranges
int launch_filter_compact(const FilterArgs &a, uint64_t n_words, const uint32_t *word_base, uint32_t *ids,
                          hipStream_t stream, const RangeList *list = nullptr);
// exact path, step 2: top-n of the `nsel` queries (a.qsel, or the first nsel) over the A listed ids; part holds
// nsel x nseg x n keys of scratch.  Writes ids, dists, counts and stats (n_dist = A, n_exp = sum_deg = 0).
uint32_t filt_exact_segments(uint64_t A, uint32_t nsel);
int launch_filtered_exact(const DevView &v, const FilterArgs &a, uint32_t nsel, const uint32_t *ids, uint32_t A,
                          uint32_t nseg, unsigned long long *part, int32_t *part_status, hipStream_t stream);
// the grouped form: `ngroups` groups compacted in one launch (the widest has max_words words), then the `nsel` queries of
// a.qsel scanned and merged in one launch each, every query over its own list (qtab[y]; max_nseg: the most segments any
// of them has).  a carries what the groups share: the rows' base is not read (a group's row is in its record), the label
// column, the deleted set, n, Q, the outputs.
int launch_filter_compact_grouped(const FilterArgs &a, const ExactGroup *gtab, uint32_t ngroups, uint64_t max_words,
                                  hipStream_t stream);
int launch_filtered_exact_grouped(const DevView &v, const FilterArgs &a, uint32_t nsel, const ExactQuery *qtab,
                                  uint32_t max_nseg, unsigned long long *part, int32_t *part_status, hipStream_t stream);
// the top n (1 <= n <= HX_FILT_MAX_N) by (distance bits, global id) of m.nq queries over the lists of m.n_shards shards:
// ONE launch of hx_filt_merge_kernel in its shard-list form, one wave per query.  out_counts may be nullptr; out_stats
// goes with m.stats.  A query some shard answered with a status other than HNSW_OK gets that status (the lowest-numbered
// such shard's), count 0 and padded rows; n_dist, n_exp and sum_deg are the uint32 sums over the shards.
int launch_merge_lists(const MergeLists &m, uint32_t n, uint32_t *out_ids, float *out_dists, uint32_t *out_counts,
                       hnsw_query_stats *out_stats, hipStream_t stream);
// the collapse by label of m.nq candidate lists of m.pool entries (the third form; m.ids, m.dists, m.pool, m.n_groups,
// m.per_group, m.group_labels and m.group_sizes set, 1 <= n_groups, per_group <= pool <= HX_GROUP_POOL_MAX and
// n_groups x per_group <= HX_GROUP_SLOTS_MAX): ONE launch of hx_filt_merge_kernel, one wave per query.  out_counts may be
// nullptr; out_stats goes with m.stats.
int launch_group_by_label(const MergeLists &m, uint32_t *out_ids, float *out_dists, uint32_t *out_counts,
                          hnsw_query_stats *out_stats, hipStream_t stream);
// the cut at a radius of candidate lists of m.pool entries into rows of m.cut_out (the fourth form; m.ids, m.dists,
// m.radius, m.pool and m.cut_out set, 1 <= pool <= cut_out <= HX_RADIUS_MAX_N): ONE launch of hx_filt_merge_kernel, one
// wave per served query -- the n_sel queries of sel (device), or, with sel == nullptr, all m.nq.  out_counts and m.flags
// may be nullptr; out_stats goes with m.stats.
int launch_radius_cut(const MergeLists &m, const uint32_t *sel, uint32_t n_sel, uint32_t *out_ids, float *out_dists,
                      uint32_t *out_counts, hnsw_query_stats *out_stats, hipStream_t stream);
// the drop of exclusion ids from candidate lists of m.pool entries into rows of m.drop_out (the fifth form; m.ids, m.dists,
// m.ex, m.ex_width, m.pool and m.drop_out set, 1 <= drop_out <= pool <= HX_RADIUS_MAX_N, 1 <= ex_width <=
// HX_DROP_MAX_WIDTH): ONE launch of hx_filt_merge_kernel, one wave per served query, selected as launch_radius_cut's.
// out_counts, m.src_status and m.dropped may be nullptr; out_stats goes with m.stats.
int launch_drop_ids(const MergeLists &m, const uint32_t *sel, uint32_t n_sel, uint32_t *out_ids, float *out_dists,
                    uint32_t *out_counts, hnsw_query_stats *out_stats, hipStream_t stream);

}  // namespace hx
