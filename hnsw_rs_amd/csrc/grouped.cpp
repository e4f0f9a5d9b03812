// grouped.cpp -- grouped search (include/hnsw_mi355x.h, "grouped search"): the collapse of candidate lists by label on
// the device, and a search answered as its nearest groups.  Host logic only; the collapse is hx_filt_merge_kernel's
// third source form (search_filtered.hip), the candidate stage around it lists_host.h.

#include "lists_host.h"

using hx::set_error;

static_assert(HX_GROUP_POOL_MAX == HNSW_GROUP_POOL_MAX, "the kernel's lanes hold the ABI's pool limit");

namespace {

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
    if (int rc = hx::need_handle("group by label", h)) return rc;
    if (nq == 0) return HNSW_OK;
    if (int rc = check_group_shape("group by label", pool, n_groups, per_group)) return rc;
    if (int rc = hx::check_nq("group by label", nq)) return rc;
    if (!d_ids_in || !d_dists_in || !d_ids || !d_dists || !d_group_labels || !d_group_sizes) {
        set_error("group by label: needs the candidates' ids and distances and the id, distance, group label and group size outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("group by label", "candidates'", d_stats_in, d_stats)) return rc;
    if (int rc = hx::ready_for_lists(h)) return rc;
    return collapse(h, nq, pool, n_groups, per_group, d_ids_in, d_dists_in, d_counts_in, d_stats_in, d_ids, d_dists,
                    d_group_labels, d_group_sizes, d_counts, d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_grouped(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n_groups, uint32_t per_group,
                              uint32_t pool, uint32_t ef, hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo,
                              const uint32_t *hi, uint32_t *ids, float *dists, uint32_t *group_labels, uint32_t *group_sizes,
                              uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    const hx::CandidateFilter f{set, mask_of, lo, hi};
    if ((rc = hx::check_candidate_filter("grouped search", h, f))) return rc;
    if (nq == 0) return HNSW_OK;
    if ((rc = check_group_shape("grouped search", pool, n_groups, per_group))) return rc;
    const bool host_form = f.filtered() || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("grouped search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Q || !ids || !group_labels || nq > 0x7FFFFFFFull) {
        set_error("grouped search: needs queries, an id buffer, a group label buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    hx::HostLists lists;
    if (host_form && (rc = hx::host_candidates(h, Q, nq, pool, ef, f, lists))) return rc;
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    // device arena: [queries | re-run selection | candidate block (nq, pool) | grouped block]; pinned arena: [the
    // candidates' stats | grouped block]
    const hx::ResultBlock cand(nq, pool);
    const size_t slots = (size_t)nq * n_groups * per_group * 4, groups = (size_t)nq * n_groups * 4;
    hx::ColumnBlock out;  // [ids | dists | group labels | group sizes | counts | stats]
    const size_t c_ids = out.add(slots), c_dists = out.add(slots), c_labels = out.add(groups), c_sizes = out.add(groups);
    const size_t c_counts = out.add(nq * 4), c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_resel = o_q + hx::align256(nq * v.dim * 4), o_cand = o_resel + hx::align256(nq * 4);
    const size_t o_out = o_cand + cand.bytes, p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    if (host_form) {
        rc = hx::upload(lists, c, sc.stream, true);
    } else {
        float *d_Q = hx::at<float>(dv, o_q);
        if ((rc = hx::queries_up(h, d_Q, Q, nq, sc.stream))) return rc;
        rc = hx::device_candidates(v, d_Q, nq, pool, ef, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    }
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = collapse(h, nq, pool, n_groups, per_group, c.ids, c.dists, c.counts, c.stats, hx::at<uint32_t>(d_out, c_ids),
                  hx::at<float>(d_out, c_dists), hx::at<uint32_t>(d_out, c_labels), hx::at<uint32_t>(d_out, c_sizes),
                  hx::at<uint32_t>(d_out, c_counts), hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_grouped_calls,
                          {ids, dists, group_labels, group_sizes, counts, stats}, nq);
}

}  // extern "C"
