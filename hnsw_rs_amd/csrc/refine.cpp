// refine.cpp -- refined search (include/hnsw_mi355x.h, "refined search"): a candidate list re-scored against full rows
// kept in HBM and cut to the nearest, on the device, and a search answered from the index's own rows and then ranked by
// the full ones.  Host logic only; the refinement is hx_distance_kernel's sixth source form (exact_scan.hip), the table
// row_table.h, the candidate stage around it lists_host.h.

#include <algorithm>
#include <cstring>

#include "lists_host.h"
#include "row_table.h"

using hx::set_error;

static_assert(HX_REFINE_POOL_MAX == HNSW_REFINE_POOL_MAX, "the kernel's LDS holds the ABI's pool limit");
static_assert(HX_REFINE_MAX_DIM == HNSW_REFINE_MAX_DIM, "the kernel's staged query holds the ABI's dimension limit");

namespace {

// the limits of the refinement (`what`: the entry point, `n`: its name for the output length, for the text)
int check_refine_shape(const char *what, const char *n, uint32_t pool, uint32_t n_out, uint32_t full_dim, uint32_t dtype) {
    if (n_out == 0 || n_out > pool || pool > HNSW_REFINE_POOL_MAX) {
        set_error("%s: needs 1 <= %s <= pool <= %d", what, n, HNSW_REFINE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    if (full_dim == 0 || full_dim > HNSW_REFINE_MAX_DIM) {
        set_error("%s: needs 1 <= full_dim <= %d", what, HNSW_REFINE_MAX_DIM);
        return HNSW_ERR_ARG;
    }
    if (dtype != HNSW_ROWS_F32 && dtype != HNSW_ROWS_F16) {
        set_error("%s: the dtype is HNSW_ROWS_F32 (0) or HNSW_ROWS_F16 (1)", what);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// the refinement over nq lists already in HBM: the one launch
int refine(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t full_dim, uint32_t dtype, const void *d_table,
           uint64_t table_rows, const float *d_Qfull, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
           const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
           hipStream_t stream) {
    hx::DiverseLists d{};
    d.ids = d_ids_in;
    d.counts = d_counts_in;
    d.stats = d_stats_in;
    d.pool = pool;
    d.n_out = n_out;
    d.nq = (uint32_t)nq;
    d.out_ids = d_ids;
    d.out_dists = d_dists;
    d.out_counts = d_counts;
    d.out_stats = d_stats;
    d.queries = d_Qfull;
    d.table = d_table;
    d.table_rows = table_rows;
    d.full_dim = full_dim;
    d.table_dtype = dtype;
    return hx::launch_refine(d, stream);
}

}  // namespace

extern "C" {

int hnsw_refine_device(uint64_t nq, uint32_t pool, uint32_t n_out, uint32_t full_dim, uint32_t dtype, const void *d_table,
                       uint64_t table_rows, const float *d_Qfull, const uint32_t *d_ids_in, const uint32_t *d_counts_in,
                       const hnsw_query_stats *d_stats_in, uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                       hnsw_query_stats *d_stats, void *stream) {
    if (nq == 0) return HNSW_OK;
    if (int rc = check_refine_shape("refine", "n_out", pool, n_out, full_dim, dtype)) return rc;
    if (int rc = hx::check_nq("refine", nq)) return rc;
    if (!d_table || !d_Qfull || !d_ids_in || !d_ids || !d_dists) {
        set_error("refine: needs the table, the full queries, the candidates' ids and the id and distance outputs");
        return HNSW_ERR_ARG;
    }
    if (int rc = hx::check_stats_pair("refine", "candidates'", d_stats_in, d_stats)) return rc;
    return refine(nq, pool, n_out, full_dim, dtype, d_table, table_rows, d_Qfull, d_ids_in, d_counts_in, d_stats_in, d_ids,
                  d_dists, d_counts, d_stats, static_cast<hipStream_t>(stream));
}

int hnsw_search_batch_refined(hnsw_index *h, hnsw_row_table *t, const float *Q, const float *Qfull, uint64_t nq, uint32_t n,
                              uint32_t pool, uint32_t ef, hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo,
                              const uint32_t *hi, uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    int rc = hx::check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    const hx::CandidateFilter f{set, mask_of, lo, hi};
    if ((rc = hx::check_candidate_filter("refined search", h, f))) return rc;
    if (nq == 0) return HNSW_OK;
    if (!t) {
        set_error("refined search: needs a row table");
        return HNSW_ERR_ARG;
    }
    if (t->owner != h) {
        set_error("refined search: the row table belongs to another handle");
        return HNSW_ERR_ARG;
    }
    const uint32_t full_dim = t->full_dim;
    if ((rc = check_refine_shape("refined search", "n", pool, n, full_dim, t->dtype))) return rc;
    const bool host_form = f.filtered() || h->del.count;
    if (host_form && pool > HX_FILT_MAX_N) {
        set_error("refined search: needs pool <= %d under a filter or while ids are deleted", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!Qfull || !ids || nq > 0x7FFFFFFFull) {
        set_error("refined search: needs the full queries, an id buffer and at most 2^31 - 1 queries");
        return HNSW_ERR_ARG;
    }
    const uint64_t dim = hx::is_replica(h) ? h->dev.view.dim : h->host->dim;
    if (!Q && full_dim < dim) {
        set_error("refined search: without Q the index's queries are the first %llu elements of a full row, which has %u",
                  (unsigned long long)dim, full_dim);
        return HNSW_ERR_ARG;
    }
    const uint64_t table_rows = t->rows, len = hx::index_len(h);
    if (table_rows < len) {
        set_error("refined search: the row table has %llu rows, the index %llu", (unsigned long long)table_rows,
                  (unsigned long long)len);
        return HNSW_ERR_ARG;
    }
    const uint32_t efp = std::max(std::max(ef, pool), 1u);
    hx::HostLists lists;
    std::vector<float> q_prefix;  // the host form searches host rows: the prefixes, packed
    if (host_form) {
        if (!Q) {
            q_prefix.resize(nq * dim);
            for (uint64_t i = 0; i < nq; i++) memcpy(&q_prefix[i * dim], Qfull + i * full_dim, dim * 4);
        }
        if ((rc = hx::host_candidates(h, Q ? Q : q_prefix.data(), nq, pool, efp, f, lists))) return rc;
    }
    if ((rc = hx::ensure_uploaded(h))) return rc;
    const hx::DevView &v = h->dev.view;
    if (t->device != h->dev.device) {
        set_error("refined search: the row table sits on device %d, the snapshot on device %d", t->device, h->dev.device);
        return HNSW_ERR_ARG;
    }
    // device arena: [queries | full queries | re-run selection | candidate block (nq, pool) | refined block]; pinned arena:
    // [the candidates' stats | refined block]
    const hx::ResultBlock cand(nq, pool);
    hx::ColumnBlock out;  // [ids | dists | counts | stats]
    const size_t c_ids = out.add(nq * n * 4), c_dists = out.add(nq * n * 4), c_counts = out.add(nq * 4);
    const size_t c_stats = out.add(nq * sizeof(hnsw_query_stats));
    const size_t o_q = 0, o_qf = o_q + hx::align256(nq * v.dim * 4), o_resel = o_qf + hx::align256(nq * full_dim * 4);
    const size_t o_cand = o_resel + hx::align256(nq * 4), o_out = o_cand + cand.bytes;
    const size_t p_out = hx::align256(nq * sizeof(hnsw_query_stats));
    hx::ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, p_out + out.bytes))) return rc;
    hx::SearchScratch &sc = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(sc.dev), *hv = static_cast<unsigned char *>(sc.pin);
    float *d_Q = hx::at<float>(dv, o_q), *d_Qfull = hx::at<float>(dv, o_qf);
    const hx::ResultBlock::Ptrs c = cand.at(dv + o_cand);
    // the full queries go up as given: the cosine option is the index's and applies to its own queries alone
    HIP_TRY(hipMemcpyAsync(d_Qfull, Qfull, nq * full_dim * 4, hipMemcpyHostToDevice, sc.stream));
    if (host_form) {
        rc = hx::upload(lists, c, sc.stream, false);  // (the distances are not an input of the refinement)
    } else {
        if (Q) {
            rc = hx::queries_up(h, d_Q, Q, nq, sc.stream);
        } else {  // the prefixes: one strided copy, no host repack
            HIP_TRY(hipMemcpy2DAsync(d_Q, (size_t)v.dim * 4, Qfull, (size_t)full_dim * 4, (size_t)v.dim * 4, nq,
                                     hipMemcpyHostToDevice, sc.stream));
            rc = hx::cosine_queries(h, d_Q, nq, sc.stream);
        }
        if (rc != HNSW_OK) return rc;
        rc = hx::device_candidates(v, d_Q, nq, pool, efp, nullptr, 0, c, hx::at<uint32_t>(dv, o_resel), sc.stream, hv);
    }
    if (rc != HNSW_OK) return rc;
    unsigned char *d_out = dv + o_out;
    rc = refine(nq, pool, n, full_dim, t->dtype, t->d_rows, table_rows, d_Qfull, c.ids, c.counts, c.stats,
                hx::at<uint32_t>(d_out, c_ids), hx::at<float>(d_out, c_dists), hx::at<uint32_t>(d_out, c_counts),
                hx::at<hnsw_query_stats>(d_out, c_stats), sc.stream);
    if (rc != HNSW_OK) return rc;
    h->n_refine_launches.fetch_add(1, std::memory_order_relaxed);
    return hx::bring_back(out, d_out, hv + p_out, sc.stream, h->n_refine_calls, {ids, dists, counts, stats}, nq);
}

}  // extern "C"
