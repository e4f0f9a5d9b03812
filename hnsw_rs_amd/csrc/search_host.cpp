// search_host.cpp -- the host side of the unfiltered search entry points: the host-pointer path and the completion of a
// device-pointer call, around the re-run loop (rerun.h).  Host logic only; the kernels are search_kernels.hip and
// search_lean.hip.  Filtered search, and these entry points while ids are deleted, are filter_host.cpp.

#include "rerun.h"
#include "switches.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace hx {

// ---- the host-pointer search path --------------------------------------------------------------------------
HostSearchPlan plan_host_search(uint64_t nq, uint32_t d, uint32_t n, uint32_t n_entry) {
    HostSearchPlan p{};
    p.o_q = 0;
    p.o_sel = p.o_q + align256(nq * d * 4);
    p.o_ent = p.o_sel + align256(nq * 4);
    p.o_out = p.o_ent + align256((size_t)n_entry * 4);
    p.out = ResultBlock(nq, n);
    p.dev_bytes = p.o_out + p.out.bytes;
    p.p_q = 0;
    p.p_out = align256(nq * d * 4);
    p.pin_bytes = p.p_out + p.out.bytes;
    return p;
}

SearchArgs ann_args(const DevView &v, const float *dQ, uint32_t n, uint32_t ef, uint32_t *ids, float *dists,
                    uint32_t *counts, hnsw_query_stats *stats) {
    SearchArgs a{};
    a.Q = dQ;
    a.qsel = nullptr;
    a.entries = nullptr;
    a.n_entry = 1;
    a.layer_hi = (int32_t)v.nb_layers - 1;  // template.rs:322-326: layers L-1..1 with ef = 1,
    a.layer_lo = 0;                         // then layer 0 with ef
    a.ef_upper = 1;
    a.ef_bottom = ef;
    a.n = n;
    a.out_ids = ids;
    a.out_dists = dists;
    a.out_counts = counts;
    a.out_stats = stats;
    return a;
}

int query_status_error(uint64_t i, int32_t status) {
    switch (status) {
        case HNSW_OK:
            break;
        case HNSW_ERR_NAN_INPUT:
            set_error("query %llu: NaN in the query or in a distance", (unsigned long long)i);
            break;
        case HNSW_ERR_NODE_NOT_IN_GRAPH:
            set_error("Error in search_layer: node not in Graph (query %llu)", (unsigned long long)i);
            break;
        case HNSW_ERR_OVERFLOW:
            set_error("query %llu: visited table exhausted at its largest size", (unsigned long long)i);
            break;
        default:
            set_error("query %llu failed with status %d", (unsigned long long)i, status);
    }
    return status;
}

int search_staged(hnsw_index *h, SearchScratch &s, const HostSearchPlan &p, SearchArgs a_host, uint64_t nq,
                  const uint32_t *entries, const float *Q_user) {
    const DevView &v = h->dev.view;
    unsigned char *dv = static_cast<unsigned char *>(s.dev), *hv = static_cast<unsigned char *>(s.pin);
    int rc;
    // Small calls skip both copies: pinned host memory is mapped into the device's address space, the kernel reads
    // each query once (400 B per wave over the link) and writes its few result words straight into the pinned
    // result block.  Measured on the 1M x 100d index: a lone 1024-query call 225 us against 232 us with the copies, but
    // 2 / 3 concurrent 1024-query callers 5.2 / 7.5 M q/s against 5.9 / 8.0 M (the copy engines overlap with the other
    // caller's kernel, reads over the link from a busy kernel do not) -- so calls of up to 512 queries (every coalesced
    // batch of up to 512 callers) go without copies, larger ones, and calls whose queries are normalised on the
    // device first (the cosine option), keep them.
    const bool zc = sw::zero_copy() && !Q_user && !h->cosine && nq <= sw::zero_copy_max();
    SearchArgs a = a_host;
    if (zc) {
        a.Q = reinterpret_cast<const float *>(hv + p.p_q);
    } else {
        HIP_TRY(hipMemcpyAsync(dv + p.o_q, Q_user ? (const void *)Q_user : (const void *)(hv + p.p_q), nq * v.dim * 4,
                               hipMemcpyHostToDevice, s.stream));
        if ((rc = cosine_queries(h, dv + p.o_q, nq, s.stream))) return rc;
        a.Q = reinterpret_cast<const float *>(dv + p.o_q);
    }
    p.out.bind(a, zc ? hv + p.p_out : dv + p.o_out);  // where the kernel writes the result block
    if (entries) {
        HIP_TRY(hipMemcpyAsync(dv + p.o_ent, entries, (size_t)a.n_entry * 4, hipMemcpyHostToDevice, s.stream));
        a.entries = reinterpret_cast<const uint32_t *>(dv + p.o_ent);
    }
    const uint32_t ef_max = std::max(a.ef_bottom, a.ef_upper);
    const uint32_t slots = default_slots_log2(ef_max, v.S0);
    if ((rc = launch_search(v, a, (uint32_t)nq, slots, s.stream))) return rc;
    return rerun_overflowed(
        v, launch_search, a, nq, slots, max_slots_log2(ef_max), reinterpret_cast<uint32_t *>(dv + p.o_sel), s.stream,
        [&](const hnsw_query_stats *&st) -> int {
            if (!zc) HIP_TRY(hipMemcpyAsync(hv + p.p_out, dv + p.o_out, p.out.bytes, hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
            st = p.out.at(hv + p.p_out).stats;
            return HNSW_OK;
        },
        nullptr);
}

int search_host(hnsw_index *h, SearchArgs a_host, const float *Q, uint64_t nq, uint32_t *ids, float *dists,
                uint32_t *counts, hnsw_query_stats *stats, const uint32_t *entries) {
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const uint32_t d = h->dev.view.dim;
    HostSearchPlan p = plan_host_search(nq, d, a_host.n, entries ? a_host.n_entry : 0);
    // queries go through the pinned arena up to 8 MiB (a batch of 1024 x 100d is 400 KB); beyond that the
    // runtime's own pageable staging serves, and the pinned arena holds the result block only
    const bool stage_q = nq * (size_t)d * 4 <= (8u << 20);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, p.dev_bytes, stage_q ? p.pin_bytes : p.out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    if (!stage_q) p.p_out = 0;
    unsigned char *hv = static_cast<unsigned char *>(s.pin);
    if (stage_q) memcpy(hv + p.p_q, Q, nq * (size_t)d * 4);
    if ((rc = search_staged(h, s, p, a_host, nq, entries, stage_q ? nullptr : Q))) return rc;
    p.out.copy_out(hv + p.p_out, ids, dists, counts, stats);
    return first_query_error(p.out.at(hv + p.p_out).stats, nq);
}

int search_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                         float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream) {
    int rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const DevView &v = h->dev.view;
    const size_t st_bytes = nq * sizeof(hnsw_query_stats);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), st_bytes))) return rc;
    SearchScratch &s = *lease.s;
    const hnsw_query_stats *st = static_cast<const hnsw_query_stats *>(s.pin);
    DeviceQueries dq;  // a re-run reads the queries again: the unit-length copy under the cosine option
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    SearchArgs a = ann_args(v, dq.q, n, ef, d_ids, d_dists, d_counts, d_stats);
    rc = rerun_overflowed(
        v, launch_search, a, nq, default_slots_log2(ef, v.S0), max_slots_log2(ef), static_cast<uint32_t *>(s.dev), stream,
        [&](const hnsw_query_stats *&out) -> int {
            HIP_TRY(hipMemcpyAsync(s.pin, d_stats, st_bytes, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            out = st;
            return HNSW_OK;
        },
        nullptr);
    if (rc != HNSW_OK) return rc;
    for (uint64_t i = 0; i < nq; i++) {
        if (st[i].status != HNSW_OK) {  // (this entry point's own wording, not query_status_error's)
            set_error("query %llu failed with status %d%s", (unsigned long long)i, st[i].status,
                      st[i].status == HNSW_ERR_NAN_INPUT    ? " (NaN in the query or in a distance)"
                      : st[i].status == HNSW_ERR_OVERFLOW   ? " (visited table exhausted at its largest size)"
                                                             : "");
            return st[i].status;
        }
    }
    return HNSW_OK;
}

}  // namespace hx
