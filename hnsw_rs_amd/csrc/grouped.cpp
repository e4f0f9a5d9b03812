// grouped.cpp -- grouped search (include/hnsw_mi355x.h, "grouped search"): the collapse of candidate lists by label on
// the device, and a search answered as its nearest groups.  Host logic only; the collapse is hx_filt_merge_kernel's
// third source form (search_filtered.hip).

#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"
#include "search_host.h"

using hx::set_error;

static_assert(HX_GROUP_POOL_MAX == HNSW_GROUP_POOL_MAX, "the kernel's lanes hold the ABI's pool limit");

namespace {

bool per_query_status(int rc) {
    return rc == HNSW_ERR_NAN_INPUT || rc == HNSW_ERR_NODE_NOT_IN_GRAPH || rc == HNSW_ERR_OVERFLOW;
}

// the limits of the collapse (`what`: the entry point, for the text)
int check_group_shape(const char *what, uint32_t pool, uint32_t n_groups, uint32_t per_group) {
    if (pool == 0 || pool > HNSW_GROUP_POOL_MAX || n_groups == 0 || n_groups > pool || per_group == 0 || per_group > pool ||
        (uint64_t)n_groups * per_group > HX_GROUP_SLOTS_MAX) {
        set_error("%s: needs 1 <= pool <= %d, 1 <= n_groups, per_group <= pool and n_groups x per_group <= %d", what,
                  HNSW_GROUP_POOL_MAX, HX_GROUP_SLOTS_MAX);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// The grouped block of nq queries: [ids | dists | group labels | group sizes | counts | stats], the same layout in the
// device arena and in pinned memory, so it comes back in ONE copy (as ResultBlock, search_host.h).
struct GroupBlock {
    size_t ids = 0, dists, labels, sizes, counts, stats, bytes;
    GroupBlock(uint64_t nq, uint32_t n_groups, uint32_t per_group) {
        const size_t slots = (size_t)nq * n_groups * per_group * 4, groups = (size_t)nq * n_groups * 4;
        dists = ids + hx::align256(slots);
        labels = dists + hx::align256(slots);
        sizes = labels + hx::align256(groups);
        counts = sizes + hx::align256(groups);
        stats = counts + hx::align256(nq * 4);
        bytes = stats + hx::align256(nq * sizeof(hnsw_query_stats));
    }
    template <class T>
    T *at(void *base, size_t off) const {
        return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off);
    }
};

// the collapse of nq lists already in HBM: the label column brought up to date, then the one launch
int collapse(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_groups, uint32_t per_group, const uint32_t *d_ids_in,
             const float *d_dists_in, const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, uint32_t *d_ids,
             float *d_dists, uint32_t *d_group_labels, uint32_t *d_group_sizes, uint32_t *d_counts, hnsw_query_stats *d_stats,
             hipStream_t stream) {
    hx::MergeLists m{};
    if (int rc = hx::labels_on_device(h, &m.labels, &m.label_len)) return rc;
    m.ids = d_ids_in;
    m.dists = d_dists_in;
    m.counts = d_counts_in;
    m.stats = d_stats_in;
    m.nq = (uint32_t)nq;
    m.pool = pool;
    m.n_groups = n_groups;
    m.per_group = per_group;
    m.group_labels = d_group_labels;
    m.group_sizes = d_group_sizes;
    if (int rc = hx::launch_group_by_label(m, d_ids, d_dists, d_counts, d_stats, stream)) return rc;
    h->n_grouped_launches.fetch_add(1, std::memory_order_relaxed);
    return HNSW_OK;
}

}  // namespace

extern "C" {

int hnsw_group_by_label_device(hnsw_index *h, uint64_t nq, uint32_t pool, uint32_t n_groups, uint32_t per_group,
                               const uint32_t *d_ids_in, const float *d_dists_in, const uint32_t *d_counts_in,
                               const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_dists,
                               uint32_t *d_group_labels, uint32_t *d_group_sizes, uint32_t *d_counts,
                               hnsw_query_stats *d_stats, void *stream) {
    if (!h) {
        set_error("group by label: null handle");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if (int rc = check_group_shape("group by label", pool, n_groups, per_group)) return rc;
    if (nq > 0x7FFFFFFFull) {
        set_error("group by label: at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    if (!d_ids_in || !d_dists_in || !d_ids || !d_dists || !d_group_labels || !d_group_sizes) {
        set_error("group by label: needs the candidates' ids and distances and the id, distance, group label and group size outputs");
        return HNSW_ERR_ARG;
    }
    if ((d_stats_in != nullptr) != (d_stats != nullptr)) {
        set_error("group by label: the stats output goes with the candidates' stats, both or neither");
        return HNSW_ERR_ARG;
    }
    int rc = hx::check_search_args(h, 0);  // (the lists are a search's: the handle has points and a complete build)
    if (rc != HNSW_OK || (rc = hx::ensure_uploaded(h))) return rc;
    return collapse(h, nq, pool, n_groups, per_group, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
                    d_group_labels, d_group_sizes, d_counts, d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_grouped(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_groups, uint32_t per_group,
                              uint32_t pool, uint32_t ef, hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo,
                              const uint32_t *hi, uint32_t *ids, float *dists, uint32_t *group_labels, uint32_t *group_sizes,
                              uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (set && set->owner != h) {
        set_error("grouped search: the mask set belongs to another handle");
        return HNSW_ERR_ARG;
    }
    if (mask_of && !set) {
        set_error("grouped search: mask_of needs its mask set");
        return HNSW_ERR_ARG;
    }
    if ((lo != nullptr) != (hi != nullptr)) {
        set_error("grouped search: a label range needs lo and hi, both or neither");
        return HNSW_ERR_ARG;
    }
    if (nq == 0) return HNSW_OK;
    if ((rc = check_group_shape("grouped search", pool, n_groups, per_group))) return rc;
    const bool filtered = set || lo;
    if ((filtered || h->del.count) && pool > HX_FILT_MAX_N) {
        set_error("grouped search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || !group_labels || nq > 0x7FFFFFFFull) {
        set_error("grouped search: needs queries, an id buffer, a group label buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    const uint64_t dim = h->dev.replica ? h->dev.view.dim : h->host->dim;
    // device arena: [queries | candidate ids [nq][pool] | dists | counts | stats | grouped block], the grouped block
    // back in one copy to the pinned arena
    const size_t cand = hx::align256(nq * pool * 4);
    const size_t o_q = 0, o_ids = o_q + hx::align256(nq * dim * 4), o_dists = o_ids + cand, o_counts = o_dists + cand;
    const size_t o_stats = o_counts + hx::align256(nq * 4), o_out = o_stats + hx::align256(nq * sizeof(hnsw_query_stats));
    const GroupBlock out(nq, n_groups, per_group);
    // The candidates.  Under a filter or deletions they are the HOST form's: only it lets the planner choose the exact
    // path ("filter_exact_max"), and the call is defined by it (as the deleted shard of hnsw_search_batch_shards)
    std::vector<uint32_t> h_ids, h_counts;
    std::vector<float> h_dists;
    std::vector<hnsw_query_stats> h_stats;
    const bool host_form = filtered || h->del.count;
    if (host_form) {
        h_ids.resize(nq * pool), h_dists.resize(nq * pool), h_counts.resize(nq), h_stats.resize(nq);
        if (set && lo)
            rc = hnsw_search_batch_filtered_set_range(h, Q, nq, pool, ef, set, mask_of, lo, hi, h_ids.data(), h_dists.data(),
                                                      h_counts.data(), h_stats.data(), nullptr);
        else if (set)
            rc = hnsw_search_batch_filtered_set(h, Q, nq, pool, ef, set, mask_of, h_ids.data(), h_dists.data(), h_counts.data(),
                                                h_stats.data(), nullptr);
        else if (lo)
            rc = hnsw_search_batch_filtered_range(h, Q, nq, pool, ef, lo, hi, h_ids.data(), h_dists.data(), h_counts.data(),
                                                  h_stats.data(), nullptr);
        else
            rc = hnsw_search_batch(h, Q, nq, pool, ef, h_ids.data(), h_dists.data(), h_counts.data(), h_stats.data());
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev);
    float *d_Q = reinterpret_cast<float *>(dv + o_q), *d_dists_in = reinterpret_cast<float *>(dv + o_dists);
    uint32_t *d_ids_in = reinterpret_cast<uint32_t *>(dv + o_ids), *d_counts_in = reinterpret_cast<uint32_t *>(dv + o_counts);
    hnsw_query_stats *d_stats_in = reinterpret_cast<hnsw_query_stats *>(dv + o_stats);
    if (host_form) {  // (the host vectors outlive the copies: the stream is synchronised below)
        HIP_TRY(hipMemcpyAsync(d_ids_in, h_ids.data(), nq * pool * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_dists_in, h_dists.data(), nq * pool * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_counts_in, h_counts.data(), nq * 4, hipMemcpyHostToDevice, sc.stream));
        HIP_TRY(hipMemcpyAsync(d_stats_in, h_stats.data(), nq * sizeof(hnsw_query_stats), hipMemcpyHostToDevice, sc.stream));
    } else {  // as a caller of the device entry point would run it: launch, then _finish
        HIP_TRY(hipMemcpyAsync(d_Q, Q, nq * dim * 4, hipMemcpyHostToDevice, sc.stream));
        rc = hnsw_search_batch_device(h, d_Q, nq, pool, ef, d_ids_in, d_dists_in, d_counts_in, d_stats_in, sc.stream);
        if (rc != HNSW_OK) return rc;
        rc = hnsw_search_batch_device_finish(h, d_Q, nq, pool, ef, d_ids_in, d_dists_in, d_counts_in, d_stats_in, sc.stream);
        if (rc != HNSW_OK && !per_query_status(rc)) return rc;
    }
    rc = collapse(h, nq, pool, n_groups, per_group, d_ids_in, d_dists_in, d_counts_in, d_stats_in,
                  out.at<uint32_t>(dv + o_out, out.ids), out.at<float>(dv + o_out, out.dists),
                  out.at<uint32_t>(dv + o_out, out.labels), out.at<uint32_t>(dv + o_out, out.sizes),
                  out.at<uint32_t>(dv + o_out, out.counts), out.at<hnsw_query_stats>(dv + o_out, out.stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    HIP_TRY(hipMemcpyAsync(sc.pin, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    h->n_grouped_calls.fetch_add(1, std::memory_order_relaxed);
    const size_t slots = (size_t)nq * n_groups * per_group * 4, groups = (size_t)nq * n_groups * 4;
    memcpy(ids, out.at<uint32_t>(sc.pin, out.ids), slots);
    if (dists) memcpy(dists, out.at<float>(sc.pin, out.dists), slots);
    memcpy(group_labels, out.at<uint32_t>(sc.pin, out.labels), groups);
    if (group_sizes) memcpy(group_sizes, out.at<uint32_t>(sc.pin, out.sizes), groups);
    if (counts) memcpy(counts, out.at<uint32_t>(sc.pin, out.counts), nq * 4);
    const hnsw_query_stats *st = out.at<hnsw_query_stats>(sc.pin, out.stats);
    if (stats) memcpy(stats, st, nq * sizeof(hnsw_query_stats));
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return hx::query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // extern "C"
