// partition.cpp -- partitioned search (include/hnsw_mi355x.h, "partitioned search"): the top-n merge of per-shard
// result lists on the device, and S handles on one device answered as one index.  Host logic only; the merge is
// hx_filt_merge_kernel's shard-list form (search_filtered.hip), the candidate stage before it lists_host.h.

#include <cstring>

#include "lists_host.h"
#include "rerun.h"

using hx::set_error;

static_assert(HX_MERGE_MAX_SHARDS == HNSW_MERGE_MAX_SHARDS, "the kernel's id map holds the ABI's shard limit");

namespace {

// the merge of the shards' lists [S][nq][n] already in HBM: the one launch.  base / stride of every shard travel by
// value in the kernel's arguments (stride NULL: all 1)
int merge(uint32_t n_shards, uint64_t nq, uint32_t n, const uint32_t *d_ids_in, const float *d_dists_in,
          const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, const uint32_t *id_base, const uint32_t *id_stride,
          uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream) {
    hx::MergeLists m{};
    m.ids = d_ids_in;
    m.dists = d_dists_in;
    m.counts = d_counts_in;
    m.stats = d_stats_in;
    m.n_shards = n_shards;
    m.nq = (uint32_t)nq;
    for (uint32_t s = 0; s < n_shards; s++) {
        m.base[s] = id_base[s];
        m.stride[s] = id_stride ? id_stride[s] : 1u;
    }
    return hx::launch_merge_lists(m, n, d_ids, d_dists, d_counts, d_stats, stream);
}

}  // namespace

extern "C" {

int hnsw_merge_topk_device(uint32_t n_shards, uint64_t nq, uint32_t n, const uint32_t *d_ids_in, const float *d_dists_in,
                           const uint32_t *d_counts_in, const hnsw_query_stats *d_stats_in, const uint32_t *id_base,
                           const uint32_t *id_stride, uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                           hnsw_query_stats *d_stats, void *stream) {
    if (nq == 0) return HNSW_OK;
    if (n_shards == 0 || n_shards > HNSW_MERGE_MAX_SHARDS || n == 0 || n > HX_FILT_MAX_N || nq > 0x7FFFFFFFull) {
        set_error("shard merge: needs 1 to %d shards, 1 <= n <= %d and at most 2^31 - 1 queries", HNSW_MERGE_MAX_SHARDS,
                  HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!d_ids_in || !d_dists_in || !id_base || !d_ids || !d_dists) {
        set_error("shard merge: needs the shards' ids and distances, their id bases and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("shard merge", "shards'", d_stats_in, d_stats)) return rc;
    return merge(n_shards, nq, n, d_ids_in, d_dists_in, d_counts_in, d_stats_in, id_base, id_stride, d_ids, d_dists, d_counts,
                 d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_shards(hnsw_index *const *shards, uint32_t n_shards, const uint32_t *id_base,
                             const uint32_t *id_stride, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    if (!shards || n_shards == 0 || n_shards > HNSW_MERGE_MAX_SHARDS || !id_base) {
        set_error("partitioned search: needs 1 to %d shards and their id bases", HNSW_MERGE_MAX_SHARDS);
        return HNSW_ERR_ARG;
    }
    uint64_t dim = 0;
    int device = -1;
    for (uint32_t s = 0; s < n_shards; s++) {
        hnsw_index *h = shards[s];
        if (!h) {
            set_error("partitioned search: shard %u is a null handle", s);
            return HNSW_ERR_ARG;
        }
        hnsw_params p;
        int rc = hnsw_get_params(h, &p);
        if (rc != HNSW_OK) return rc;
        if (s == 0) dim = p.dim;
        if (p.dim != dim) {
            set_error("partitioned search: shard %u has dimension %llu, shard 0 %llu", s, (unsigned long long)p.dim,
                      (unsigned long long)dim);
            return HNSW_ERR_ARG;
        }
        if (h->device >= 0) {  // (a handle not bound yet goes where the others are)
            if (device >= 0 && h->device != device) {
                set_error("partitioned search: shard %u is bound to device %d, another shard to device %d", s, h->device, device);
                return HNSW_ERR_ARG;
            }
            device = h->device;
        }
    }
    if (n > HX_FILT_MAX_N || nq > 0x7FFFFFFFull) {
        set_error("partitioned search: needs n <= %d and at most 2^31 - 1 queries", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    for (uint32_t s = 0; s < n_shards; s++)
        if (int rc = hx::check_search_args(shards[s], ef)) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || !ids) {
        set_error("partitioned search: needs queries and an id buffer");
        return HNSW_ERR_ARG;
    }
    if (n == 0) {
        if (counts) memset(counts, 0, nq * 4);
        return HNSW_OK;
    }
    // every shard's snapshot on the one device: shard 0's (or the bound one's), where the scratch and the merge are
    hnsw_index *const h0 = shards[0];
    if (h0->device < 0 && device >= 0) {
        if (int rc = hnsw_set_device(h0, device)) return rc;
    }
    for (uint32_t s = 0; s < n_shards; s++) {
        hnsw_index *h = shards[s];
        if (s > 0 && h->device < 0) {
            if (int rc = hnsw_set_device(h, h0->dev.device)) return rc;
        }
        if (int rc = hx::ensure_uploaded(h)) return rc;
        if (h->dev.device != h0->dev.device) {
            set_error("partitioned search: shard %u is on device %d, shard 0 on device %d", s, h->dev.device, h0->dev.device);
            return HNSW_ERR_ARG;
        }
    }
    // device arena: [queries | ids [S][nq][n] | dists [S][nq][n] | counts [S][nq] | stats [S][nq] | result block], the
    // result block back in one copy to the pinned arena
    const uint64_t S = n_shards;
    const size_t o_q = 0, o_ids = o_q + hx::align256(nq * dim * 4), o_dists = o_ids + hx::align256(S * nq * n * 4);
    const size_t o_counts = o_dists + hx::align256(S * nq * n * 4), o_stats = o_counts + hx::align256(S * nq * 4);
    const size_t o_out = o_stats + hx::align256(S * nq * sizeof(hnsw_query_stats));
    const hx::ResultBlock out(nq, n);
    hx::ScratchLease lease(h0);
    if (int rc = lease.prepare(h0->dev.device, o_out + out.bytes, out.bytes)) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev);
    float *d_Q = hx::at<float>(dv, o_q), *d_dists_in = hx::at<float>(dv, o_dists);
    uint32_t *d_ids_in = hx::at<uint32_t>(dv, o_ids), *d_counts_in = hx::at<uint32_t>(dv, o_counts);
    hnsw_query_stats *d_stats_in = hx::at<hnsw_query_stats>(dv, o_stats);
    HIP_TRY(hipMemcpyAsync(d_Q, Q, nq * dim * 4, hipMemcpyHostToDevice, sc.stream));
    // each shard as a caller of its own device entry point would run it: launch, then _finish (overflow re-runs and the
    // cosine option are the shard's).  A per-query error stays in the shard's stats and reaches the merged row; anything
    // else ends the call.  A shard with deleted ids is the exception: its device entry point always walks the graph,
    // while its hnsw_search_batch lets the planner choose ("filter_exact_max"), and the call is defined by the latter --
    // so such a shard is answered by its host form and its lists go up into its slice.  (Not device_candidates, which
    // wants the unit-length queries in place: the shards share one d_Q and each has its own cosine option, so the unit
    // copy has to stay the shard's own, as its device entry point makes it.)
    std::vector<hx::HostLists> lists(S);  // one per shard: each outlives its asynchronous copies, until the merge is back
    for (uint64_t s = 0; s < S; s++) {
        const hx::ResultBlock::Ptrs c{d_ids_in + s * nq * n, d_dists_in + s * nq * n, d_counts_in + s * nq, d_stats_in + s * nq};
        if (shards[s]->del.count) {
            if (int rc = hx::host_candidates(shards[s], Q, nq, n, ef, {}, lists[s])) return rc;
            if (int rc = hx::upload(lists[s], c, sc.stream, true)) return rc;
            continue;
        }
        int rc = hnsw_search_batch_device(shards[s], d_Q, nq, n, ef, c.ids, c.dists, c.counts, c.stats, sc.stream);
        if (rc != HNSW_OK) return rc;
        rc = hnsw_search_batch_device_finish(shards[s], d_Q, nq, n, ef, c.ids, c.dists, c.counts, c.stats, sc.stream);
        if (rc != HNSW_OK && !hx::per_query_status(rc)) return rc;
    }
    h0->n_shard_calls.fetch_add(1, std::memory_order_relaxed);
    const hx::ResultBlock::Ptrs o = out.at(dv + o_out);
    if (int rc = merge(n_shards, nq, n, d_ids_in, d_dists_in, d_counts_in, d_stats_in, id_base, id_stride, o.ids, o.dists,
                       o.counts, o.stats, sc.stream))
        return rc;
    h0->n_shard_merges.fetch_add(1, std::memory_order_relaxed);
    HIP_TRY(hipMemcpyAsync(sc.pin, dv + o_out, out.bytes, hipMemcpyDeviceToHost, sc.stream));
    HIP_TRY(hipStreamSynchronize(sc.stream));
    out.copy_out(sc.pin, ids, dists, counts, stats);
    return hx::first_query_error(out.at(sc.pin).stats, nq);
}

}  // extern "C"
