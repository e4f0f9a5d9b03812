// options.cpp -- the options and the statistics of a handle, one table each: hnsw_set_option and hnsw_clone walk
// the first, hnsw_get_stat the second (what the names mean: include/hnsw_mi355x.h).

#include <algorithm>
#include <cstring>

#include "handle.h"

namespace hx {

namespace {

template <class T> T stored(const T &x) { return x; }
template <class T> T stored(const std::atomic<T> &x) { return x.load(); }

// what a value has to be, with the text of the refusal (after the option's name)
enum Bound { ANY, POSITIVE, NOT_NEGATIVE, ZERO_OR_ONE };
const char *refusal(Bound b, int64_t value) {
    if (b == POSITIVE && value < 1) return "must be positive";
    if (b == NOT_NEGATIVE && value < 0) return "must not be negative";
    if (b == ZERO_OR_ONE && value != 0 && value != 1) return "must be 0 or 1";
    return nullptr;
}

// RELEASES: storing it releases the HBM snapshot (rebuilt by the next upload; not on a replica); CO_LOCKED: it is
// stored under the coalescer's lock
enum { RELEASES = 1, CO_LOCKED = 2 };
constexpr int64_t NO_CLAMP = INT64_MAX;

struct Option {
    const char *name;
    Bound bound;
    int64_t clamp;  // larger values are stored as this one
    int flags;
    void (*store)(hnsw_index &h, int64_t value);
    void (*copy)(hnsw_index &to, const hnsw_index &from);  // the stored field itself, not a value parsed again
};
// FIELD: the member of the handle that holds the option; STORED: what `value` becomes in it
#define HX_OPTION(NAME, BOUND, CLAMP, FLAGS, FIELD, STORED)                            \
    {NAME, BOUND, CLAMP, FLAGS, [](hnsw_index &h, int64_t value) { h.FIELD = STORED; }, \
     [](hnsw_index &to, const hnsw_index &from) { to.FIELD = stored(from.FIELD); }}
const Option kOptions[] = {
    HX_OPTION("inline_rows", ANY, NO_CLAMP, RELEASES, dev.inline_rows, (int)value),
    HX_OPTION("inline_budget_mb", ANY, NO_CLAMP, RELEASES, dev.fat_budget_bytes, (uint64_t)value << 20),
    HX_OPTION("gpu_build", ANY, NO_CLAMP, 0, gpu_build, (int)value),
    // points already stored stay as they are: set it before the first insert (or on a loaded index whose
    // rows were stored under it -- the reference's file format has no field for a metric)
    HX_OPTION("metric_cosine", ANY, NO_CLAMP, 0, cosine, value != 0),
    HX_OPTION("filter_exact_max", ANY, NO_CLAMP, 0, filter_exact_max, value),
    HX_OPTION("filter_exact_grouped", ZERO_OR_ONE, NO_CLAMP, 0, filter_exact_grouped, (int)value),
    HX_OPTION("mask_set_cache_mb", NOT_NEGATIVE, 1 << 20, 0, mask_set_cache_mb, value),
    HX_OPTION("gpu_build_batch_max", POSITIVE, 1 << 20, 0, build_batch_max, (uint32_t)value),
    HX_OPTION("gpu_build_batch_div", POSITIVE, 1 << 20, 0, build_batch_div, (uint32_t)value),
    HX_OPTION("coalesce_us", ANY, 100000, CO_LOCKED, co.window_us, value),
    HX_OPTION("coalesce_depth", POSITIVE, 64, CO_LOCKED, co.depth, (uint32_t)value),
    HX_OPTION("coalesce_max", POSITIVE, CoBatch::COUNT, CO_LOCKED, co.cap, (uint32_t)value),  // (what a batch's word can count)
};
#undef HX_OPTION

struct Stat {
    const char *name;
    uint64_t (*get)(const hnsw_index &h);
};
#define HX_STAT(NAME, VALUE) {NAME, [](const hnsw_index &h) -> uint64_t { return VALUE; }}
const Stat kStats[] = {
    HX_STAT("uploads", h.n_uploads),
    HX_STAT("point_patches", h.n_point_patches),
    HX_STAT("patch_fallbacks", h.n_patch_fallbacks),
    HX_STAT("build_points", h.build.points),
    HX_STAT("build_batches", h.build.batches),
    HX_STAT("build_rows_read", h.build.rows_read),
    HX_STAT("build_adj_rows", h.build.adj_rows),
    HX_STAT("build_adj_ids", h.build.adj_ids),
    HX_STAT("build_records", h.build.records),
    HX_STAT("build_removals", h.build.removals),
    HX_STAT("build_insert_kernel_us", (uint64_t)(h.build.insert_kernel_s * 1e6)),
    HX_STAT("build_insert_phase_us", (uint64_t)(h.build.insert_phase_s * 1e6)),
    HX_STAT("build_connect_us", (uint64_t)(h.build.connect_s * 1e6)),
    HX_STAT("build_connect_kernel_us", (uint64_t)(h.build.connect_kernel_s * 1e6)),
    HX_STAT("build_rows_owned", h.build.rows_owned),
    HX_STAT("build_rows_received", h.build.rows_received),
    HX_STAT("build_exchange_bytes", h.build.exchange_bytes),
    HX_STAT("build_exchange_us", (uint64_t)(h.build.exchange_s * 1e6)),
    HX_STAT("build_cpu_path_points", h.build.cpu_path_points),
    HX_STAT("build_rerun_points", h.build.rerun_points),
    HX_STAT("build_kept_last_edges", h.build.kept_last_edges),
    HX_STAT("filtered_queries_graph", h.n_filt_graph),
    HX_STAT("filtered_queries_exact", h.n_filt_exact),
    HX_STAT("filtered_overflow_exact", h.n_filt_overflow),
    HX_STAT("label_words_uploaded", h.lab.words_uploaded),
    HX_STAT("filtered_range_calls", h.n_filt_range_calls),
    HX_STAT("filtered_range_ranges", h.n_filt_range_ranges),
    HX_STAT("filtered_set_range_calls", h.n_filt_set_range_calls),
    HX_STAT("filtered_set_range_groups", h.n_filt_set_range_groups),
    HX_STAT("filtered_one_calls", h.n_filt_one_calls),
    HX_STAT("filtered_one_batches", h.n_filt_one_batches),
    HX_STAT("filtered_ranges_calls", h.n_filt_ranges_calls),
    HX_STAT("filtered_ranges_groups", h.n_filt_ranges_groups),
    HX_STAT("filtered_multi_calls", h.n_filt_multi_calls),
    HX_STAT("filtered_multi_masks", h.n_filt_multi_masks),
    HX_STAT("mask_set_words_uploaded", h.n_set_words_uploaded),
    HX_STAT("mask_set_recounts", h.n_set_recounts),
    HX_STAT("mask_set_compactions", h.n_set_compactions),
    HX_STAT("filtered_set_calls", h.n_filt_set_calls),
    HX_STAT("shard_calls", h.n_shard_calls),
    HX_STAT("shard_merges", h.n_shard_merges),
    HX_STAT("grouped_calls", h.n_grouped_calls),
    HX_STAT("grouped_launches", h.n_grouped_launches),
    HX_STAT("radius_calls", h.n_radius_calls),
    HX_STAT("radius_rungs", h.n_radius_rungs),
    HX_STAT("radius_launches", h.n_radius_launches),
    HX_STAT("diverse_calls", h.n_diverse_calls),
    HX_STAT("diverse_launches", h.n_diverse_launches),
    HX_STAT("from_rows_calls", h.n_from_rows_calls),
    HX_STAT("from_rows_compose_launches", h.n_from_rows_compose),
    HX_STAT("from_rows_drop_launches", h.n_from_rows_drop),
    HX_STAT("multi_calls", h.n_multi_calls),
    HX_STAT("multi_fuse_launches", h.n_multi_fuse),
    HX_STAT("late_calls", h.n_late_calls),
    HX_STAT("late_launches", h.n_late_launches),
    HX_STAT("docs_calls", h.n_docs_calls),
    HX_STAT("docs_launches", h.n_docs_launches),
    HX_STAT("doc_index_uploads", h.lab.doc.uploads),
    HX_STAT("doc_index_keys_uploaded", h.lab.doc.keys_uploaded),
    HX_STAT("refine_calls", h.n_refine_calls),
    HX_STAT("refine_launches", h.n_refine_launches),
    HX_STAT("row_table_writes", h.n_row_table_writes),
    HX_STAT("hybrid_calls", h.n_hybrid_calls),
    HX_STAT("hybrid_fuse_launches", h.n_hybrid_fuse),
    HX_STAT("boost_calls", h.n_boost_calls),
    HX_STAT("boost_launches", h.n_boost_launches + hx::boost_device_launches()),
    HX_STAT("deleted", h.del.count),
    HX_STAT("deleted_mask_words_uploaded", h.del.words_uploaded),
    HX_STAT("deleted_queries_graph", h.n_del_graph),
    HX_STAT("deleted_queries_exact", h.n_del_exact),
    HX_STAT("deleted_overflow_exact", h.n_del_overflow),
    HX_STAT("coalesced_batches", h.co.n_batches),
    HX_STAT("coalesced_queries", h.co.n_queries),
    HX_STAT("coalesced_max_batch", h.co.max_batch),
    HX_STAT("coalesce_ns_window", h.co.ns_window),
    HX_STAT("coalesce_ns_turn", h.co.ns_turn),
    HX_STAT("coalesce_ns_gpu", h.co.ns_gpu),
    HX_STAT("coalesce_ns_handout", h.co.ns_handout),
};
#undef HX_STAT

// the row of a table under a name, or nullptr
template <class Row, size_t N>
const Row *find(const Row (&table)[N], const char *name) {
    const Row *r = std::find_if(table, table + N, [&](const Row &row) { return !strcmp(row.name, name); });
    return r == table + N ? nullptr : r;
}

}  // namespace

int set_option(hnsw_index *h, const char *key, int64_t value) {
    std::lock_guard<std::mutex> g(h->mu);
    const Option *o = find(kOptions, key);
    if (!o) {
        set_error("unknown option %s", key);
        return HNSW_ERR_ARG;
    }
    if (const char *why = refusal(o->bound, value)) {
        set_error("%s %s", key, why);
        return HNSW_ERR_ARG;
    }
    value = std::min(value, o->clamp);
    std::unique_lock<SpinLock> cg(h->co.mu, std::defer_lock);
    if (o->flags & CO_LOCKED) cg.lock();
    o->store(*h, value);
    if ((o->flags & RELEASES) && !is_replica(h)) h->dev.release();
    return HNSW_OK;
}

void copy_options(hnsw_index *to, const hnsw_index *from) { for (const Option &o : kOptions) o.copy(*to, *from); }

int get_stat(const hnsw_index *h, const char *key, uint64_t *out) {
    const Stat *s = find(kStats, key);
    if (!s) {
        set_error("unknown statistic %s", key);
        return HNSW_ERR_ARG;
    }
    *out = s->get(*h);
    return HNSW_OK;
}

}  // namespace hx
