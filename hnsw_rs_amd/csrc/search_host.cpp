// search_host.cpp -- the host side of the search entry points: the host-pointer path, the filtered / deleted
// orchestration and the completion of a device-pointer call, around one re-run loop.  Host logic only; the kernels
// are search_kernels.hip, search_lean.hip and search_filtered.hip.

#include "search_host.h"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace hx {

namespace {

// ---- the re-run loop ---------------------------------------------------------------------------------------------
// A query whose visited table filled up ends with status HNSW_ERR_OVERFLOW and is run again with a table twice the
// size, until none is left or the largest table is reached.  The first launch is the caller's (perhaps in an earlier
// call); what differs from site to site comes in as
//   launch, a:   launch_search or launch_filtered_graph and its arguments (a.qsel is set to the selection);
//   fetch(st):   bring the statuses (or the whole result block) of everything launched so far back to the host,
//                synchronise, and say where they are;
//   exhausted(sel):  answer the queries that filled the largest table some other way and fetch again -- or nullptr:
//                their status stays HNSW_ERR_OVERFLOW for the caller to report.
// d_sel holds the selection on the device (room for nq ids).  n_exhausted = queries handed to `exhausted`.
template <class Args, class Fetch, class Exhausted>
int rerun_overflowed(const DevView &v, int (*launch)(const DevView &, const Args &, uint32_t, uint32_t, hipStream_t), Args &a,
                     uint64_t nq, uint32_t slots, uint32_t max_slots, uint32_t *d_sel, hipStream_t stream, Fetch fetch,
                     Exhausted exhausted, uint64_t *n_exhausted = nullptr) {
    std::vector<uint32_t> sel;
    while (true) {
        const hnsw_query_stats *st = nullptr;
        int rc = fetch(st);
        if (rc != HNSW_OK) return rc;
        sel.clear();
        for (uint64_t i = 0; i < nq; i++)
            if (st[i].status == HNSW_ERR_OVERFLOW) sel.push_back((uint32_t)i);
        if (sel.empty()) return HNSW_OK;
        if (slots >= max_slots) {
            if constexpr (std::is_same_v<Exhausted, std::nullptr_t>) {
                return HNSW_OK;
            } else {
                if (n_exhausted) *n_exhausted = sel.size();
                return exhausted(sel);
            }
        }
        HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // `sel` is reused by the next round
        a.qsel = d_sel;
        if ((rc = launch(v, a, (uint32_t)sel.size(), ++slots, stream))) return rc;
    }
}

// first per-query failure of a call, with its text
int first_query_error(const hnsw_query_stats *st, uint64_t nq) {
    for (uint64_t i = 0; i < nq; i++)
        if (st[i].status != HNSW_OK) return query_status_error(i, st[i].status);
    return HNSW_OK;
}

}  // namespace

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
    static const bool zc_allowed = !(getenv("HNSW_MI355X_ZERO_COPY") && atoi(getenv("HNSW_MI355X_ZERO_COPY")) == 0);
    static const uint64_t zc_max = getenv("HNSW_MI355X_ZERO_COPY_MAX") ? strtoull(getenv("HNSW_MI355X_ZERO_COPY_MAX"), nullptr, 0) : 512;
    const bool zc = zc_allowed && !Q_user && !h->cosine && nq <= zc_max;
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

// ---- filtered search, and the unfiltered entry points while ids are deleted --------------------------------------
namespace {

// brings the deleted set's HBM copy up to date on the snapshot's device (on a stream of the handle's own, so that a
// caller's stream is not synchronised); a no-op while nothing is deleted
int sync_deleted(hnsw_index *h) {
    if (h->del.count == 0) return HNSW_OK;
    std::lock_guard<std::mutex> g(h->mu);
    if (h->del.d_words && h->del.d_device == h->dev.device && h->del.dirty.empty()) return HNSW_OK;
    ScratchLease lease(h);
    int rc = lease.prepare(h->dev.device, 0, 0);
    if (rc != HNSW_OK) return rc;
    return h->del.sync(h->dev.device, lease.s->stream);
}

// The admissible ids of a call: below bits = min(allow_bits, len), allowed by `allow` (nullptr: all), not deleted.
// -> A, and the admissible ids before every block of 64 words (the compaction kernel's offsets)
uint64_t count_admissible(const hnsw_index *h, const uint64_t *allow, uint64_t bits, std::vector<uint32_t> &wbase) {
    const uint64_t n_words = (bits + 63) / 64, n_wblk = (n_words + 63) / 64;
    const std::vector<uint64_t> &deny = h->del.words;
    const bool denies = h->del.count > 0;
    wbase.assign(std::max<uint64_t>(1, n_wblk), 0);
    uint64_t A = 0;
    for (uint64_t w = 0; w < n_words; w++) {
        if (w % 64 == 0) wbase[w / 64] = (uint32_t)A;
        uint64_t x = allow ? allow[w] : ~0ull;
        if (w == n_words - 1 && bits % 64) x &= (1ull << (bits % 64)) - 1;
        if (denies && w < deny.size()) x &= ~deny[w];
        A += (uint64_t)__builtin_popcountll(x);
    }
    return A;
}

// The exact path's scratch for up to nsel queries over A admissible ids, from `base` in a device arena:
// [word offsets | admissible ids | partial keys | partial statuses]; `chunk` queries per launch, `nseg` segments each
struct ExactScratch {
    uint32_t chunk, nseg;
    size_t o_wb, o_ids, o_part, o_pst, end;
    ExactScratch(size_t base, uint64_t nsel, uint32_t n, uint64_t A, size_t n_wbase)
        : chunk((uint32_t)std::min<uint64_t>(nsel, 65535)), nseg(filt_exact_segments(A, chunk)) {
        o_wb = base;
        o_ids = o_wb + align256(n_wbase * 4);
        o_part = o_ids + align256(A * 4);
        o_pst = o_part + align256((size_t)chunk * nseg * n * 8);
        end = o_pst + align256((size_t)chunk * nseg * 4);
    }
};

// the exact path for nsel queries: those of d_sel, or the first nsel of the call; the word offsets are in place
int filtered_exact(const DevView &v, const FilterArgs &a, uint64_t nsel, const uint32_t *d_sel, uint64_t A,
                   const ExactScratch &x, unsigned char *dv, hipStream_t stream) {
    uint32_t *d_ids = reinterpret_cast<uint32_t *>(dv + x.o_ids);
    int r = launch_filter_compact(a, (a.allow_bits + 63) / 64, reinterpret_cast<const uint32_t *>(dv + x.o_wb), d_ids, stream);
    for (uint64_t c = 0; r == HNSW_OK && c < nsel; c += x.chunk) {
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
        r = launch_filtered_exact(v, ac, (uint32_t)std::min<uint64_t>(x.chunk, nsel - c), d_ids, (uint32_t)A, x.nseg,
                                  reinterpret_cast<unsigned long long *>(dv + x.o_part),
                                  reinterpret_cast<int32_t *>(dv + x.o_pst), stream);
    }
    return r;
}

}  // namespace

int search_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const uint64_t *allow,
                    uint64_t allow_bits, bool exact_only, uint32_t *ids, float *dists, uint32_t *counts,
                    hnsw_query_stats *stats, uint8_t *paths, const PathCounters *ctr, void *pin_block) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || (!ids && !pin_block) || nq > 0x7FFFFFFFull || n > HX_FILT_MAX_N) {
        set_error("filtered search: needs queries, an id buffer, a mask when allow_bits > 0 and n <= %d",
                  HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (n == 0) {  // nothing returned, nothing launched
        if (counts) memset(counts, 0, nq * 4);
        return HNSW_OK;
    }
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    const uint64_t bits = std::min<uint64_t>(allow_bits, index_len(h));
    const uint64_t n_words = (bits + 63) / 64;
    std::vector<uint32_t> wbase;
    const uint64_t A = count_admissible(h, allow, bits, wbase);
    const bool exact_all = exact_only || (int64_t)A <= h->filter_exact_max;
    if (!exact_all && efp > HX_FILT_MAX_EF) {
        set_error("filtered search: ef' = max(ef, n) = %u is above the graph path's maximum of %d", efp, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h))) return rc;
    const DevView &v = h->dev.view;
    const uint32_t d = v.dim;
    // device arena: [queries | mask | selection | the exact path's scratch | result block]; the result block comes
    // back in one copy to pinned memory: the caller's block, or the scratch's and from there to the caller's buffers
    const size_t o_q = 0, o_mask = o_q + align256(nq * d * 4), o_sel = o_mask + align256(allow ? n_words * 8 : 0);
    const ExactScratch x(o_sel + align256(nq * 4), nq, n, A, wbase.size());
    const size_t o_out = x.end;
    const ResultBlock out(nq, n);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, o_out + out.bytes, pin_block ? 0 : out.bytes))) return rc;
    SearchScratch &s = *lease.s;
    unsigned char *dv = static_cast<unsigned char *>(s.dev);
    void *hv = pin_block ? pin_block : s.pin;
    HIP_TRY(hipMemcpyAsync(dv + o_q, Q, nq * d * 4, hipMemcpyHostToDevice, s.stream));
    if ((rc = cosine_queries(h, dv + o_q, nq, s.stream))) return rc;
    if (n_words) {
        if (allow) HIP_TRY(hipMemcpyAsync(dv + o_mask, allow, n_words * 8, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wbase.data(), wbase.size() * 4, hipMemcpyHostToDevice, s.stream));
    }
    FilterArgs a{};
    a.Q = reinterpret_cast<const float *>(dv + o_q);
    a.allow = allow ? reinterpret_cast<const uint64_t *>(dv + o_mask) : nullptr;
    a.allow_bits = bits;
    a.deny = h->del.count ? h->del.d_words : nullptr;
    a.deny_bits = h->del.count ? h->del.deny_bits() : 0;
    a.n = n;
    a.ef = efp;
    out.bind(a, dv + o_out);
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(dv + o_sel);
    auto fetch = [&](const hnsw_query_stats *&st) -> int {
        HIP_TRY(hipMemcpyAsync(hv, dv + o_out, out.bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        st = out.at(hv).stats;
        return HNSW_OK;
    };
    std::vector<uint8_t> path(nq, exact_all ? 1 : 0);
    uint64_t n2 = 0;
    const hnsw_query_stats *st;
    if (exact_all) {
        if ((rc = filtered_exact(v, a, nq, nullptr, A, x, dv, s.stream)) || (rc = fetch(st))) return rc;
    } else {
        // graph path; queries whose visited table filled up run again with a table twice the size, and those
        // that fill the largest one are answered by the exact path
        const uint32_t slots = filt_first_slots_log2(v, efp);
        if ((rc = launch_filtered_graph(v, a, (uint32_t)nq, slots, s.stream))) return rc;
        rc = rerun_overflowed(
            v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v), d_sel, s.stream, fetch,
            [&](const std::vector<uint32_t> &sel) -> int {
                for (uint32_t i : sel) path[i] = 2;
                HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s.stream));
                int r = filtered_exact(v, a, sel.size(), d_sel, A, x, dv, s.stream);
                return r != HNSW_OK ? r : fetch(st);  // (synchronises: `sel` lives until then)
            },
            &n2);
        if (rc != HNSW_OK) return rc;
    }
    if (ctr) {
        if (exact_all)
            ctr->exact->fetch_add(nq, std::memory_order_relaxed);
        else
            ctr->graph->fetch_add(nq - n2, std::memory_order_relaxed);
        ctr->overflow->fetch_add(n2, std::memory_order_relaxed);
    }
    if (!pin_block) out.copy_out(hv, ids, dists, counts, stats);
    if (paths) memcpy(paths, path.data(), nq);
    return HNSW_OK;
}

int search_filtered_checked(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, const uint64_t *allow,
                            uint64_t allow_bits, bool exact_only, uint32_t *ids, float *dists, uint32_t *counts,
                            hnsw_query_stats *stats, uint8_t *paths, const PathCounters *ctr) {
    std::vector<hnsw_query_stats> local;
    if (!stats) {
        local.resize(nq);
        stats = local.data();
    }
    int rc = search_filtered(h, Q, nq, n, ef, allow, allow_bits, exact_only, ids, dists, counts, stats, paths, ctr);
    if (rc != HNSW_OK || n == 0) return rc;
    return first_query_error(stats, nq);
}

int search_device_deleted(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, uint32_t *d_ids,
                          float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, hipStream_t stream, bool finish) {
    const uint32_t efp = std::max(std::max(ef, n), 1u);
    if (n > HX_FILT_MAX_N || efp > HX_FILT_MAX_EF) {
        set_error("search with deleted ids: needs n <= %d and ef' = max(ef, n) <= %d", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    int rc;
    if ((rc = ensure_uploaded(h)) || (rc = sync_deleted(h))) return rc;
    const DevView &v = h->dev.view;
    DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, stream))) return rc;
    // the kernels write distances and counts: stream-ordered stand-ins for the optional outputs
    struct Tmp {
        void *p = nullptr;
        hipStream_t st = nullptr;
        ~Tmp() {
            if (p) (void)hipFreeAsync(p, st);
        }
    } t_dists, t_counts;
    if (!d_dists) {
        HIP_TRY(hipMallocAsync(&t_dists.p, nq * n * 4, stream));
        t_dists.st = stream;
        d_dists = static_cast<float *>(t_dists.p);
    }
    if (!d_counts) {
        HIP_TRY(hipMallocAsync(&t_counts.p, nq * 4, stream));
        t_counts.st = stream;
        d_counts = static_cast<uint32_t *>(t_counts.p);
    }
    FilterArgs a{};
    a.Q = dq.q;
    a.allow = nullptr;
    a.allow_bits = index_len(h);
    a.deny = h->del.d_words;
    a.deny_bits = h->del.deny_bits();
    a.n = n;
    a.ef = efp;
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    const uint32_t slots = filt_first_slots_log2(v, efp);
    if (!finish) return launch_filtered_graph(v, a, (uint32_t)nq, slots, stream);

    // scratch: the selection on the device, the statuses on the host; the exact path's part ([selection | its
    // scratch]) is sized only when a query reaches it
    const size_t st_bytes = nq * sizeof(hnsw_query_stats);
    ScratchLease lease(h);
    if ((rc = lease.prepare(h->dev.device, align256(nq * 4), st_bytes))) return rc;
    const hnsw_query_stats *st = nullptr;
    auto fetch = [&](const hnsw_query_stats *&out) -> int {
        HIP_TRY(hipMemcpyAsync(lease.s->pin, d_stats, st_bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        out = st = static_cast<const hnsw_query_stats *>(lease.s->pin);
        return HNSW_OK;
    };
    uint64_t n2 = 0;
    rc = rerun_overflowed(
        v, launch_filtered_graph, a, nq, slots, filt_max_slots_log2(v), static_cast<uint32_t *>(lease.s->dev), stream, fetch,
        [&](const std::vector<uint32_t> &sel) -> int {  // path 2
            std::vector<uint32_t> wbase;
            const uint64_t A = count_admissible(h, nullptr, a.allow_bits, wbase);
            const ExactScratch x(align256(sel.size() * 4), sel.size(), n, A, wbase.size());
            int r = lease.prepare(h->dev.device, x.end, st_bytes);
            if (r != HNSW_OK) return r;
            unsigned char *dv = static_cast<unsigned char *>(lease.s->dev);
            HIP_TRY(hipMemcpyAsync(dv, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(dv + x.o_wb, wbase.data(), wbase.size() * 4, hipMemcpyHostToDevice, stream));
            r = filtered_exact(v, a, sel.size(), reinterpret_cast<const uint32_t *>(dv), A, x, dv, stream);
            const hnsw_query_stats *unused;
            return r != HNSW_OK ? r : fetch(unused);  // (synchronises: `sel` and `wbase` live until then)
        },
        &n2);
    if (rc != HNSW_OK) return rc;
    h->n_del_graph.fetch_add(nq - n2, std::memory_order_relaxed);
    h->n_del_overflow.fetch_add(n2, std::memory_order_relaxed);
    return first_query_error(st, nq);
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
