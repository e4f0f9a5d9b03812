// device_build.cpp -- the on-device builds behind insert_bulk ("gpu_build" = 1 / 2, hnsw_insert_bulk_device,
// hnsw_insert_bulk_sharded).  Host logic only; the kernels are in build_kernels.hip, build_sort.hip and patch.hip.

#include "device_build.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "hip_util.h"
#include "shard_exchange.h"
#include "switches.h"

namespace hx {
namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point x, Clock::time_point y) { return std::chrono::duration<double>(y - x).count(); }
int sync_device() {
    HIP_TRY(hipDeviceSynchronize());
    return HNSW_OK;
}
// fn(lo, hi) over [lo, hi) in nt pieces, each on a thread of its own (nt <= 1: on this one)
template <class F>
void for_ranges(unsigned nt, uint64_t lo, uint64_t hi, F &&fn) {
    if (nt <= 1) return fn(lo, hi);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(fn, lo + (hi - lo) * t / nt, lo + (hi - lo) * (t + 1) / nt);
    for (auto &t : th) t.join();
}
using InserterPtr = std::unique_ptr<Inserter, void (*)(Inserter *)>;
InserterPtr make_inserter(const HostIndex &host) { return InserterPtr(new_inserter(host.len()), free_inserter); }
int copy_to_host(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return HNSW_OK;
}
// the insert kernel's buffers for batches of up to bmax points, and its arguments that point at them
struct InsertBuffers {
    DevBuf levels, ids, out_ids, out_d, status;
    InsertArgs a{};
    int alloc(const HostIndex &host, uint32_t bmax) {
        const uint32_t m = (uint32_t)host.params.m, L = host.nb_layers();
        int rc;
        if ((rc = levels.alloc(host.len())) || (rc = ids.alloc(bmax * 4)) || (rc = out_ids.alloc((size_t)bmax * L * m * 4)) ||
            (rc = out_d.alloc((size_t)bmax * L * m * 4)) || (rc = status.alloc(bmax * 4)))
            return rc;
        HIP_TRY(hipMemcpy(levels.p, host.levels.data(), host.len(), hipMemcpyHostToDevice));
        a.point_ids = ids.as<uint32_t>();
        a.levels = levels.as<uint8_t>();
        a.ef_cons = (uint32_t)host.params.ef_cons;
        a.m = m;
        a.max_layers = L;
        a.out_ids = out_ids.as<uint32_t>();
        a.out_dists = out_d.as<float>();
        a.out_status = status.as<int32_t>();
        return HNSW_OK;
    }
};
int check_build_params(const HostIndex &host) {
    if (host.params.m <= 128 && host.params.ef_cons <= 512) return HNSW_OK;
    set_error("on-device build supports m <= 128 and ef_construction <= 512");
    return HNSW_ERR_ARG;
}
// the device snapshot a build starts from: without the search-only extras (inline rows)
int upload_for_build(const BuildTarget &t, const std::function<int()> &meanwhile = {}) {
    const int saved_inline = t.dev.inline_rows;
    t.dev.inline_rows = 0;
    t.dev.release();
    const int rc = t.dev.upload(t.host, t.device, meanwhile);
    t.dev.inline_rows = saved_inline;
    if (rc != HNSW_OK) return rc;
    t.device = t.dev.device;
    HIP_TRY(hipSetDevice(t.dev.device));
    return HNSW_OK;
}

// ---------------------------------------------------------------------------------------------
// On-device index build: batch-synchronous insert_bulk.
//   per batch:  GPU  hx_insert_kernel -- one wave per point: entry point, greedy descent, and for
//                    every layer of the point search_layer(ef_cons) + select_heuristic
//                    (inserter.rs:40-126) against the graph as it stands in HBM
//               host connect_point   -- the reference's make_connections / prune_connections /
//                    make_pruned_connections (template.rs:196-251) on `nb_threads` threads with the
//                    per-row locks of the CPU build
//               GPU  hx_scatter_rows -- the adjacency rows that changed go back to HBM
// The first points (and any point whose search reports an error) take the CPU path, batches grow
// with the graph (a batch never exceeds 1/8 of the points already connected, at most 4096): points
// of one batch do not see each other, like the racing threads of the reference's own multi-threaded
// insert_bulk.  The result is a valid HNSW graph judged by recall, not by identity.
// ---------------------------------------------------------------------------------------------
// Insertion order of the reference: layers top-down, ids ascending inside a level (template.rs:403-416); the
// entry point is already in.  Levels are bytes: one counting pass instead of a sort of tens of millions of ids.
std::vector<NodeID> insertion_order(const HostIndex &host, const std::vector<NodeID> &ids) {
    size_t count[257] = {0};
    for (NodeID id : ids)
        if (id != host.params.ep) count[host.levels[id]]++;
    size_t start[256], at = 0;
    for (int l = 255; l >= 0; l--) {
        start[l] = at;
        at += count[l];
    }
    std::vector<NodeID> order(at);
    for (NodeID id : ids)
        if (id != host.params.ep) order[start[host.levels[id]]++] = id;
    return order;
}

// the changed rows back to HBM (truncated to the stride; the final upload is exact) through staging buffers that the
// batches reuse (the device ones grow)
int scatter_dirty_rows(const HostIndex &host, DeviceIndex &dev, const std::vector<std::vector<uint64_t>> &dirty_t,
                       uint32_t nb_threads, std::vector<uint32_t> &row_idx, std::vector<uint32_t> &row_data, DevBuf &dRowIdx,
                       DevBuf &dRowData, size_t &row_cap) {
    const DevView &v = dev.view;
    std::vector<uint64_t> dirty0, dirty_up;  // already unique (per-row stamps)
    for (auto &dv : dirty_t)
        for (uint64_t key : dv) ((key >> 32) == 0 ? dirty0 : dirty_up).push_back(key);
    for (int pass = 0; pass < 2; pass++) {  // pass 0: layer 0 rows, pass 1: upper-layer rows
        const std::vector<uint64_t> &dirty = pass == 0 ? dirty0 : dirty_up;
        if (dirty.empty()) continue;
        const uint32_t S = pass == 0 ? v.S0 : v.S1;
        row_idx.resize(dirty.size());
        row_data.resize(dirty.size() * (size_t)S);
        const unsigned nt = (unsigned)std::min<size_t>(nb_threads, std::max<size_t>(1, dirty.size() / 4096));
        for_ranges(nt, 0, dirty.size(), [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++) {
                const uint32_t layer = (uint32_t)(dirty[i] >> 32);
                const NodeID id = (NodeID)dirty[i];
                const std::vector<NodeID> &r = host.row(layer, id);
                row_idx[i] = layer == 0 ? id : host.upper_base[id] + layer - 1;
                uint32_t *o = &row_data[i * (size_t)S];
                const size_t k = std::min<size_t>(r.size(), S);
                std::copy(r.begin(), r.begin() + k, o);
                std::fill(o + k, o + S, UINT32_MAX);
            }
        });
        int rc;
        if (row_idx.size() > row_cap) {
            row_cap = row_idx.size() * 2;
            if (dRowIdx.p) (void)hipFree(dRowIdx.p);
            if (dRowData.p) (void)hipFree(dRowData.p);
            dRowIdx.p = dRowData.p = nullptr;
            if ((rc = dRowIdx.alloc(row_cap * 4)) || (rc = dRowData.alloc(row_cap * (size_t)std::max(v.S0, v.S1) * 4)))
                return rc;
        }
        HIP_TRY(hipMemcpy(dRowIdx.p, row_idx.data(), row_idx.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dRowData.p, row_data.data(), row_data.size() * 4, hipMemcpyHostToDevice));
        rc = launch_scatter_rows(pass == 0 ? dev.adj0_mut() : dev.adj_up_mut(), S, dRowIdx.as<uint32_t>(),
                                 dRowData.as<uint32_t>(), (uint32_t)row_idx.size(), nullptr);
        if (rc != HNSW_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());  // the staging buffers are reused by the next pass
    }
    return sync_device();
}

}  // namespace

int gpu_insert_bulk(const BuildTarget &t, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                    const uint8_t *levels) {
    HostIndex &host = t.host;
    if (nb_threads == 0) nb_threads = 1;
    int rc = check_build_params(host);
    if (rc != HNSW_OK) return rc;
    const uint64_t n_before = host.len();
    std::vector<NodeID> ids;
    if ((rc = host.store_points(rows, n, levels, &ids, nb_threads))) return rc;
    host.prepare_build();
    const std::vector<NodeID> order = insertion_order(host, ids);
    // ---- seed on the CPU: the first points must be inserted one after the other ----
    const uint64_t SEED = 2048;
    size_t pos = 0;
    if (n_before < SEED) {
        // sequential (one Inserter) so that the seed graph is the reference's single-thread graph
        InserterPtr ins = make_inserter(host);
        for (const size_t take = std::min<size_t>(order.size(), SEED - n_before); pos < take; pos++)
            if ((rc = host.insert(order[pos], *ins))) return rc;
    }
    if (pos == order.size()) {
        host.version++;
        return HNSW_OK;
    }
    if ((rc = upload_for_build(t))) return rc;
    const DevView v = t.dev.view;
    const uint32_t m = (uint32_t)host.params.m, L = host.nb_layers();
    const uint32_t BMAX = 4096;
    InsertBuffers ib;
    DevBuf dRowIdx, dRowData;
    if ((rc = ib.alloc(host, BMAX))) return rc;
    std::vector<uint32_t> o_ids((size_t)BMAX * L * m);
    std::vector<float> o_d((size_t)BMAX * L * m);
    std::vector<int32_t> o_st(BMAX);
    size_t row_cap = 0;
    std::vector<uint32_t> row_idx, row_data;
    std::vector<std::vector<uint64_t>> dirty_t(nb_threads);
    DirtyStamps stamps(host.adj0.size(), host.adj_up.size());
    uint64_t connected = n_before + pos;
    const auto t_start = Clock::now();
    double t_gpu = 0, t_host = 0, t_sync = 0;
    size_t n_fallback = 0, n_batches = 0;
    while (pos < order.size()) {
        const size_t B = t.batches.next(order.size() - pos, connected, BMAX);
        const NodeID *batch = &order[pos];
        auto t0 = Clock::now();
        HIP_TRY(hipMemcpy(ib.ids.p, batch, B * 4, hipMemcpyHostToDevice));
        if ((rc = launch_insert(v, ib.a, (uint32_t)B, nullptr))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(o_ids.data(), ib.out_ids.p, B * L * m * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(o_d.data(), ib.out_d.p, B * L * m * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(o_st.data(), ib.status.p, B * 4, hipMemcpyDeviceToHost));
        auto t1 = Clock::now();
        // ---- host: connect the batch (reference semantics), collect the rows that changed ----
        std::atomic<size_t> next{0};
        std::atomic<int> err{HNSW_OK};
        std::vector<NodeID> fallback;
        std::mutex fb_mu;
        for (auto &dv : dirty_t) dv.clear();
        stamps.next_batch();
        auto work = [&](unsigned t) {
            std::vector<std::vector<Dist>> nbrs(L);
            for (size_t i = next.fetch_add(1); i < B && err.load() == HNSW_OK; i = next.fetch_add(1)) {
                const NodeID p = batch[i];
                if (o_st[i] != HNSW_OK) {
                    std::lock_guard<std::mutex> g(fb_mu);
                    fallback.push_back(p);
                    continue;
                }
                for (uint32_t l = 0; l < L; l++) {
                    nbrs[l].clear();
                    for (uint32_t k = 0; k < m; k++) {
                        const uint32_t id = o_ids[(i * L + l) * m + k];
                        if (id != UINT32_MAX) nbrs[l].push_back(Dist{id, o_d[(i * L + l) * m + k]});
                    }
                }
                const int r = host.connect_point(p, nbrs, &dirty_t[t], &stamps);
                if (r != HNSW_OK) err.store(r);
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < std::min<size_t>(nb_threads, B); t++) th.emplace_back(work, t);
        work(0);  // thread 0 is this one
        for (auto &x : th) x.join();
        if (err.load() != HNSW_OK) return err.load();
        if (!fallback.empty()) {  // e.g. visited-table overflow: the CPU path serves those points
            n_fallback += fallback.size();
            std::sort(fallback.begin(), fallback.end());
            InserterPtr ins = make_inserter(host);
            DirtyScope scope(&dirty_t[0], &stamps);
            for (NodeID p : fallback)
                if ((rc = host.insert(p, *ins))) return rc;
        }
        auto t2 = Clock::now();
        if ((rc = scatter_dirty_rows(host, t.dev, dirty_t, nb_threads, row_idx, row_data, dRowIdx, dRowData, row_cap))) return rc;
        t_gpu += secs(t0, t1);
        t_host += secs(t1, t2);
        t_sync += secs(t2, Clock::now());
        pos += B;
        connected += B;
        n_batches++;
        if (verbose && (n_batches % 16 == 0 || pos == order.size()))
            fprintf(stderr, "\rBuilding HNSW index on the GPU %zu/%zu", pos, order.size());
    }
    if (verbose)
        fprintf(stderr,
                "\non-device build: %zu batches in %.2f s (insert kernel + copies %.2f s, host connect %.2f s, "
                "row scatter %.2f s), %zu points took the CPU path\n",
                n_batches, secs(t_start, Clock::now()), t_gpu, t_host, t_sync, n_fallback);
    host.version++;  // the search snapshot (overflow CSR, inline rows) is rebuilt by the next upload
    return HNSW_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------
// On-device build, connect step on the GPU as well (option "gpu_build" = 2).  Per batch:
//   phase 1  hx_insert_kernel  -- as above; additionally writes the new point's own rows and appends
//                                 one reverse-edge request (target n, source p, layer, d) per selected
//                                 neighbour
//   host     sort the requests by (layer, target)                       [a few ms per batch]
//   phase 2  hx_connect_kernel -- one wave per target row: append, or prune to the cap's nearest;
//                                 reports the edges that fell out
//   host     sort the removals by (layer, x)
//   phase 3  hx_remove_kernel  -- one wave per row that lost a reverse edge (keeps a last edge)
// Every adjacency row is owned by one wave per phase: no locks, deterministic for a given batch
// schedule.  The host graph is rebuilt from the device arrays once, at the end.
// ---------------------------------------------------------------------------------------------
// The device rows of the full on-device build hold at most `cap` neighbours.  A row the CPU path left
// longer than that (the reference's transient overflow) is pruned here the way the next
// prune_connections would: nearest `cap` by (dist, id), reverse edges removed.  Where the dropped
// edge is the other node's last one it stays on that side (graph.rs:85-94); the pruned side gets it
// back after the build (`restore`: hx_edge_key(layer, x, node)), exactly like a refusal of hx_remove_kernel.
void clamp_rows_to_cap(HostIndex &host, std::vector<uint64_t> *restore) {
    for (uint32_t l = 0; l < host.nb_layers(); l++) {
        const size_t cap = (size_t)host.layer_m(l);
        for (NodeID id : host.layer_nodes[l]) {
            std::vector<NodeID> &row = host.row(l, id);
            if (row.size() <= cap) continue;
            PointView a, b;
            host.get_point(id, &a);
            std::vector<Dist> ds;
            for (NodeID x : row) {
                host.get_point(x, &b);
                ds.push_back(Dist{x, host.dist2other(a, b)});
            }
            std::sort(ds.begin(), ds.end(), dist_lt);
            for (size_t i = cap; i < ds.size(); i++) {
                std::vector<NodeID> &back = host.row(l, ds[i].id);
                if (back.size() == 1 && back[0] == id)
                    restore->push_back(hx_edge_key(l, ds[i].id, id));
                else
                    back.erase(std::remove(back.begin(), back.end(), id), back.end());
            }
            row.clear();
            for (size_t i = 0; i < cap; i++) row.push_back(ds[i].id);
        }
    }
}

// Sharded build (BASELINE configs[4]): every rank holds the full replica.  The insertion searches of a batch are
// split over the ranks by position, and what they produce travels as edge records through an all-gather (the
// caller's collective, RCCL in production); the record list carries the whole batch (own rows included,
// InsertArgs::emit_own) and its sort makes the order canonical.  Phases 2 / 3 are split by ROW: every rank sees
// every record, the rank that owns a row (node id % world) appends / prunes / drops in it -- each row's outcome
// depends on that row and its records alone, so the split changes nothing -- the removals phase 2 files are
// all-gathered between the two phases, and the rows an owner changed travel to the other replicas as whole rows of
// ids at the end of the batch (hx_pack_rows_kernel / hx_apply_rows_kernel).  Five collectives per batch (records;
// removal counts + removals; row counts + rows -- the count exchanges are 64 B per rank and carry the rank's status,
// so the ranks stop together), the replicas identical after each.  HNSW_MI355X_SHARD_CONNECT=0: phases 2 / 3 on
// every rank in full, as before round 4 (one collective per batch).
// Between two collectives no rank returns on a condition only it can see (the others would wait in the next
// all-gather): a rank-local failure is the status the rank files in the next collective -- the record slot's header
// or an exchange()'s -- and every rank returns the first failing rank's status from there.
// SH_BCAP: the largest batch (option gpu_build_batch_max, default 8192); buffers and exchange slots are sized for it
constexpr uint32_t SH_HEADER = 64, SH_FAILCAP = 1024, SH_BCAP = 32768;
// the record slot's header words: records written, failed points, first failing reservation, status
enum { REC_COUNT, REC_NFAIL, REC_FAIL_BASE, REC_STATUS };
inline uint32_t shard_slot_records(uint32_t m, uint32_t world) {
    return ((SH_BCAP + world - 1) / world) * m * 4;  // both directions, 2 x slack for upper layers
}
inline uint64_t shard_record_bytes(uint32_t m, uint32_t world) {  // the records' part of a slot: [header][failed ids][keys][vals]
    return ((uint64_t)SH_HEADER + SH_FAILCAP * 4 + (uint64_t)shard_slot_records(m, world) * 12 + 255) & ~255ull;
}
// rows one rank may change in a batch (its share of the targets of every rank's records, plus the rows it drops from)
inline uint32_t shard_slot_rows(uint32_t m, uint32_t world) { return 2 * shard_slot_records(m, world); }
inline uint32_t shard_ship_slots(uint32_t m) { return adj_stride(2ull * m, 32); }  // ids per shipped row: a layer-0 row

struct EvPair {  // the build's kernels are timed with HIP events on their stream
    hipEvent_t a = nullptr, b = nullptr;
    ~EvPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    int create() {
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        return HNSW_OK;
    }
    int add_ms(double *sum) const {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, a, b));
        *sum += ms;
        return HNSW_OK;
    }
};

// The device-connect build after the seed: buffers, counters and timers, one member function per step.  Sharded,
// the functions that take a status `st` are (or end in) a collective; the others are rank-local.
struct FullBuild {
    HostIndex &host;
    DeviceIndex &dev;
    const ShardCtx *sh;
    const uint32_t nb_threads, verbose;
    static constexpr uint32_t BMAX = SH_BCAP, REF_CAP = 1u << 20;  // REF_CAP: kept-last-edge records of the whole build
    DevView v{};
    uint32_t m = 0, L = 0, W = 1, SLOT_REC = 0, REQ_CAP = 0, CHG_CAP = 0, CHG_LIST_CAP = 0, SHIP = 0;
    uint64_t SHIP_UNIT = 0, REC_BYTES = 0;
    size_t temp_bytes = 0;
    bool own_rows = false;  // sharded: phases 2 / 3 by row ownership (above)
    InsertBuffers ib;
    InsertArgs &a = ib.a;  // phase 1's and phases 2 / 3's arguments: the same in every batch but for the records
    DevBuf dCnt, dKeyA, dKeyB, dValA, dValB, dTemp, dRef, dRead, dChg, dChgCnt, dAdjD0, dAdjDUp;
    uint32_t *cnt = nullptr;  // dCnt: [0] requests, [1] removals, [2] refusals (accumulate over the build), [3] status
    ConnectArgs ca{};
    int first_adjust = 0;
    EvPair ev, ev_conn, ev_rem;
    bool rem_pending = false;
    std::vector<int32_t> o_st;
    std::vector<NodeID> failed;      // points that filed nothing: CPU path after the build
    int carry = HNSW_OK;             // sharded: a rank-local failure after a batch's last collective, for the next one
    std::vector<uint32_t> rec_hdr;   // the record all-gather: every rank's slot header
    std::vector<uint32_t> x_counts;  // the last exchange(): every rank's count; rank r's data at d_recv + r * x_stride + SH_HEADER
    uint64_t x_stride = 0, x_bytes = 0;
    uint32_t nreq = 0, nreq_all = 0, nrem = 0, nrem_all = 0;  // records / removals this rank sorts and applies, of the batch
    uint32_t counts[4] = {0, 0, 0, 0};
    double t_kernel_ms = 0, t_conn_kernel_ms = 0, t_exchange = 0, t_ins = 0, t_conn = 0;
    size_t n_batches = 0, n_req = 0, n_rem = 0, n_again = 0, n_shipped = 0, n_owned = 0;
    std::thread row_reserve;  // reserves the new points' host rows while the batches run (joined before the read-back)
    FullBuild(const BuildTarget &t, const ShardCtx *sh_, uint32_t nb_threads_, int verbose_)
        : host(t.host), dev(t.dev), sh(sh_), nb_threads(nb_threads_), verbose(verbose_ != 0) {}
    ~FullBuild() {
        if (row_reserve.joinable()) row_reserve.join();
    }
    // capacities, allocations, the edge-distance arrays, events, the launch arguments
    int setup(const BatchSchedule &sched, const std::vector<NodeID> &order, size_t pos, uint64_t connected) {
        v = dev.view;
        m = (uint32_t)host.params.m;
        L = host.nb_layers();
        // a point has 1 + 1/(m-1) layers on average; sharded: records in both directions
        W = sh ? sh->world : 1;
        SLOT_REC = sh ? shard_slot_records(m, W) : 0;
        // Record capacity: what the largest batch of this build can file, (level + 1) * m per point (twice
        // that with records in both directions) -- not an average: a batch of high-level points files more than
        // 2 m each.  Sharded: the caller's slots are sized by m and the world alone; a point whose records do
        // not fit its rank's slot fails cleanly on the device (nothing reserved) and takes the CPU path.
        uint64_t need_max = 0;
        for (size_t q = pos; !sh && q < order.size();) {
            const size_t Bq = sched.next(order.size() - q, connected, BMAX);
            uint64_t need = 0;
            for (size_t i = 0; i < Bq; i++) need += ((uint64_t)host.levels[order[q + i]] + 1) * m;
            need_max = std::max(need_max, need);
            q += Bq;
            connected += Bq;
        }
        if (need_max >= (1ull << 31)) {
            set_error("on-device build: a batch would file %llu edge records", (unsigned long long)need_max);
            return HNSW_ERR_ARG;
        }
        REQ_CAP = sh ? W * SLOT_REC : (uint32_t)std::max<uint64_t>(need_max, (uint64_t)BMAX * m * 2);
        if (sh && (sh->slot_bytes < shard_slot_bytes(m, W) || sh->rank >= W || !sh->d_send || !sh->d_recv || !sh->allgather)) {
            set_error("sharded build: exchange buffers too small or bad rank / world");
            return HNSW_ERR_ARG;
        }
        temp_bytes = sort_temp_bytes(REQ_CAP);
        REC_BYTES = sh ? shard_record_bytes(m, W) : 0;
        own_rows = sh && W > 1 && sw::shard_connect();
        CHG_CAP = own_rows ? shard_slot_rows(m, W) : 0;
        SHIP = shard_ship_slots(m);
        SHIP_UNIT = 8 + 4ull * SHIP;
        if (own_rows && (v.S0 > SHIP || v.S1 > SHIP)) {
            set_error("sharded build: adjacency rows of %u / %u slots, exchange entries of %u", v.S0, v.S1, SHIP);
            return HNSW_ERR_ARG;
        }
        // the file of changed rows: HX_CHG_LISTS lists (ConnectArgs), each with room for twice its even share
        CHG_LIST_CAP = own_rows ? 2 * ((CHG_CAP + HX_CHG_LISTS - 1) / HX_CHG_LISTS) : 0;
        int rc;
        if (own_rows && ((rc = dChg.alloc((size_t)CHG_LIST_CAP * HX_CHG_LISTS * 8)) || (rc = dChgCnt.alloc(HX_CHG_LISTS * 4)))) return rc;
        x_counts.assign(W, 0);
        if ((rc = ev.create()) || (rc = ev_conn.create()) || (rc = ev_rem.create()) || (rc = dRead.alloc(32))) return rc;
        HIP_TRY(hipMemset(dRead.p, 0, 32));
        if ((rc = ib.alloc(host, BMAX)) || (rc = dCnt.alloc(64)) || (rc = dKeyA.alloc((size_t)REQ_CAP * 8)) ||
            (rc = dKeyB.alloc((size_t)REQ_CAP * 8)) || (rc = dValA.alloc((size_t)REQ_CAP * 4)) ||
            (rc = dValB.alloc((size_t)REQ_CAP * 4)) || (rc = dTemp.alloc(temp_bytes)) ||
            (rc = dRef.alloc((size_t)REF_CAP * 8)))
            return rc;
        // the edges' distances beside the adjacency for the length of this build (ConnectArgs: a prune then evaluates
        // nothing); 0xFFFFFFFF = not known yet (the rows that predate this build: evaluated at their first prune).  128 B
        // per point at m = 16; without the memory for it the build runs as before
        const size_t b0 = (size_t)host.len() * v.S0 * 4, b1 = std::max<size_t>(1, host.adj_up.size()) * v.S1 * 4;
        if (sw::build_edge_dists() && hipMalloc(&dAdjD0.p, b0) == hipSuccess && hipMalloc(&dAdjDUp.p, b1) == hipSuccess &&
            hipMemset(dAdjD0.p, 0xFF, b0) == hipSuccess && hipMemset(dAdjDUp.p, 0xFF, b1) == hipSuccess) {
            a.adjd0_mut = ca.adjd0_mut = dAdjD0.as<uint32_t>();
            a.adjd_up_mut = ca.adjd_up_mut = dAdjDUp.as<uint32_t>();
        } else {
            (void)hipGetLastError();
        }
        cnt = dCnt.as<uint32_t>();
        HIP_TRY(hipMemset(dCnt.p, 0, 64));
        o_st.resize(BMAX);
        ca.m = m;
        a.adj0_mut = ca.adj0_mut = dev.adj0_mut();
        a.adj_up_mut = ca.adj_up_mut = dev.adj_up_mut();
        a.counters = dRead.as<unsigned long long>();
        uint32_t *hdr = sh ? reinterpret_cast<uint32_t *>(sh->d_send) : nullptr;  // the slot: [header][failed ids][keys][vals]
        a.req_keys = sh ? reinterpret_cast<uint64_t *>(sh->d_send + SH_HEADER + SH_FAILCAP * 4) : dKeyA.as<uint64_t>();
        a.req_vals = sh ? reinterpret_cast<uint32_t *>(sh->d_send + SH_HEADER + SH_FAILCAP * 4 + (size_t)SLOT_REC * 8) : dValA.as<uint32_t>();
        a.req_count = sh ? hdr + REC_COUNT : cnt + 0;
        a.req_fail_base = sh ? hdr + REC_FAIL_BASE : cnt + 4;
        a.req_cap = sh ? SLOT_REC : REQ_CAP;
        a.emit_own = sh ? 1 : 0;
        first_adjust = insert_table_first_adjust(v, a);
        ca.status = reinterpret_cast<int32_t *>(cnt + 3);
        if (own_rows) {
            ca.own_rank = sh->rank;
            ca.own_world = W;
            ca.chg_keys = dChg.as<uint64_t>();
            ca.chg_count = dChgCnt.as<uint32_t>();
            ca.chg_cap = CHG_LIST_CAP;
        }
        return HNSW_OK;
    }
    int timed_insert(uint32_t nblocks, int adjust) {
        HIP_TRY(hipEventRecord(ev.a, nullptr));
        const int r = launch_insert(v, a, nblocks, nullptr, adjust);
        if (r != HNSW_OK) return r;
        HIP_TRY(hipEventRecord(ev.b, nullptr));
        HIP_TRY(hipEventSynchronize(ev.b));
        return ev.add_ms(&t_kernel_ms);
    }
    // Phase 1 on `ids` (the batch, or this rank's slice): records behind the counter d_hdr[0].  A point that filled its
    // visited table filed nothing and runs again with a larger one (a search's result does not depend on the table's
    // size) -- unless a reservation failed (d_hdr[fail_word] set: the counter is past the capacity).  Other failures go
    // to `fail`.  *written: the records written, up to the first reservation that did not fit.
    int insert_points(const NodeID *ids, size_t nb, const uint32_t *d_hdr, uint32_t fail_word, std::vector<NodeID> &fail,
                      uint32_t *written) {
        uint32_t w[5] = {0, 0, 0, 0, 0};  // d_hdr[0 .. fail_word]
        w[fail_word] = UINT32_MAX;
        int rc;
        if (nb) {
            HIP_TRY(hipMemcpy(ib.ids.p, ids, nb * 4, hipMemcpyHostToDevice));
            if ((rc = timed_insert((uint32_t)nb, first_adjust))) return rc;
            HIP_TRY(hipMemcpy(w, d_hdr, (fail_word + 1) * 4, hipMemcpyDeviceToHost));  // synchronises
            HIP_TRY(hipMemcpy(o_st.data(), ib.status.p, nb * 4, hipMemcpyDeviceToHost));
        }
        std::vector<NodeID> again;
        for (size_t i = 0; i < nb; i++)
            if (o_st[i] != HNSW_OK) (o_st[i] == HNSW_ERR_OVERFLOW && w[fail_word] == UINT32_MAX ? again : fail).push_back(ids[i]);
        if (!again.empty()) {
            HIP_TRY(hipMemcpy(ib.ids.p, again.data(), again.size() * 4, hipMemcpyHostToDevice));
            if ((rc = timed_insert((uint32_t)again.size(), std::max(first_adjust, 0) + 1))) return rc;
            HIP_TRY(hipMemcpy(w, d_hdr, (fail_word + 1) * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(o_st.data(), ib.status.p, again.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < again.size(); i++)
                if (o_st[i] != HNSW_OK) fail.push_back(again[i]);
            n_again += again.size();
        }
        *written = std::min(w[0], w[fail_word]);
        return HNSW_OK;
    }
    // phase 1 alone: the records stay in dKeyA / dValA
    int phase1(const NodeID *batch, size_t B) {
        HIP_TRY(hipMemset(cnt + 4, 0xFF, 4));  // no reservation has failed yet
        const int rc = insert_points(batch, B, cnt, 4, failed, &nreq);
        if (rc != HNSW_OK) return rc;
        if (nreq > REQ_CAP) {
            set_error("on-device build: record counter %u beyond the capacity %u", nreq, REQ_CAP);
            return HNSW_ERR_OVERFLOW;
        }
        nreq_all = nreq;
        return HNSW_OK;
    }
    // phase 1 of a rank: its slice of the batch; the records, the failed points and the header in its slot
    int shard_phase1(const NodeID *batch, size_t B) {
        uint32_t *hdr = reinterpret_cast<uint32_t *>(sh->d_send), h2[2];
        HIP_TRY(hipMemset(hdr, 0, SH_HEADER));
        HIP_TRY(hipMemset(hdr + REC_FAIL_BASE, 0xFF, 4));
        const size_t s_lo = B * sh->rank / W, s_hi = B * (sh->rank + 1) / W;
        std::vector<NodeID> myfail;
        // the count the other ranks read: the records really written (see hx_insert_kernel's reservation)
        const int rc = insert_points(batch + s_lo, s_hi - s_lo, hdr, REC_FAIL_BASE, myfail, &h2[REC_COUNT]);
        if (rc != HNSW_OK) return rc;
        if (myfail.size() > SH_FAILCAP) {
            set_error("sharded build: %zu points of one batch failed on the device", myfail.size());
            return HNSW_ERR_OVERFLOW;
        }
        h2[REC_NFAIL] = (uint32_t)myfail.size();
        HIP_TRY(hipMemcpy(hdr, h2, 8, hipMemcpyHostToDevice));
        if (h2[REC_NFAIL]) HIP_TRY(hipMemcpy(hdr + SH_HEADER / 4, myfail.data(), h2[REC_NFAIL] * 4, hipMemcpyHostToDevice));
        return HNSW_OK;
    }
    // The record all-gather, a batch's first collective: `st`, this rank's status so far, goes in its slot's status
    // word, and every rank returns the first failing rank's status.  (Its own copies and the callback: as exchange().)
    int gather_records(int st) {
        const uint32_t failed_hdr[4] = {0, 0, UINT32_MAX, (uint32_t)st};
        if (st) HIP_TRY(hipMemcpy(sh->d_send, failed_hdr, 16, hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());
        const int r = sh->allgather(sh->ctx, REC_BYTES);
        if (r != 0) {
            set_error("sharded build: the all-gather callback failed (%d)", r);
            return HNSW_ERR_RCCL;
        }
        rec_hdr.resize(W * 4);
        for (uint32_t k = 0; k < W; k++)
            HIP_TRY(hipMemcpy(&rec_hdr[k * 4], sh->d_recv + (size_t)k * REC_BYTES, 16, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < W; k++) {
            const int32_t ks = (int32_t)rec_hdr[k * 4 + REC_STATUS];
            if (ks == 0) continue;
            if (k != sh->rank || st == 0) set_error("sharded build: rank %u reported status %d in the records phase", k, ks);
            return ks;
        }
        return HNSW_OK;
    }
    // concatenate the slots' records (every rank sees the same list) and failed points; with row ownership this
    // rank's share of the records alone: the rows it owns (the others' never reach its sort)
    int concat_records() {
        const size_t o_keys = SH_HEADER + SH_FAILCAP * 4, o_vals = o_keys + (size_t)SLOT_REC * 8;
        nreq = 0;
        for (uint32_t r = 0; r < W; r++) {
            const unsigned char *rs = sh->d_recv + (size_t)r * REC_BYTES;
            const uint32_t count = rec_hdr[r * 4 + REC_COUNT], nfail = rec_hdr[r * 4 + REC_NFAIL];
            if (count > SLOT_REC || nfail > SH_FAILCAP || nreq + count > REQ_CAP) {
                set_error("sharded build: malformed slot from rank %u", r);
                return HNSW_ERR_ARG;
            }
            if (nfail) {
                const size_t at = failed.size();
                failed.resize(at + nfail);
                HIP_TRY(hipMemcpy(&failed[at], rs + SH_HEADER, nfail * 4, hipMemcpyDeviceToHost));
            }
            if (count && own_rows) {
                const int rc = filter_edge_records(reinterpret_cast<const uint64_t *>(rs + o_keys), reinterpret_cast<const uint32_t *>(rs + o_vals),
                                                   count, sh->rank, W, dKeyA.as<uint64_t>(), dValA.as<uint32_t>(), cnt + 0, REQ_CAP,
                                                   reinterpret_cast<int32_t *>(cnt + 3), nullptr);
                if (rc != HNSW_OK) return rc;
            } else if (count) {
                HIP_TRY(hipMemcpyAsync(dKeyA.as<uint64_t>() + nreq, rs + o_keys, (size_t)count * 8, hipMemcpyDeviceToDevice, nullptr));
                HIP_TRY(hipMemcpyAsync(dValA.as<uint32_t>() + nreq, rs + o_vals, (size_t)count * 4, hipMemcpyDeviceToDevice, nullptr));
            }
            nreq += count;
        }
        nreq_all = nreq;
        if (own_rows) HIP_TRY(hipMemcpy(&nreq, cnt + 0, 4, hipMemcpyDeviceToHost));  // (the counter was zeroed with the batch)
        return HNSW_OK;
    }
    // phase 2: group by target row (radix sort), append / prune
    int connect() {
        int rc = sort_edge_pairs(dTemp.p, temp_bytes, dKeyA.as<uint64_t>(), dKeyB.as<uint64_t>(), dValA.as<uint32_t>(),
                                 dValB.as<uint32_t>(), nreq, L, nullptr);
        if (rc != HNSW_OK) return rc;
        ca.keys = dKeyB.as<uint64_t>();
        ca.vals = dValB.as<uint32_t>();
        ca.count = nreq;
        ca.out_keys = dKeyA.as<uint64_t>();  // the unsorted requests are dead by now
        ca.out_count = cnt + 1;
        ca.out_cap = REQ_CAP;
        HIP_TRY(hipEventRecord(ev_conn.a, nullptr));
        if ((rc = launch_connect(v, ca, nullptr))) return rc;
        HIP_TRY(hipEventRecord(ev_conn.b, nullptr));
        HIP_TRY(hipMemcpy(counts, dCnt.p, 16, hipMemcpyDeviceToHost));
        if ((rc = ev_conn.add_ms(&t_conn_kernel_ms))) return rc;
        if (counts[3] != 0 && !own_rows) {  // (with row ownership the removals exchange carries it)
            set_error("on-device build: connect kernel reported status %d in batch %zu", (int)counts[3], n_batches);
            return (int)counts[3];
        }
        nrem = nrem_all = counts[1];
        return HNSW_OK;
    }
    // One variable-size exchange: 64 B per rank first ([count, status]: every rank learns every count and stops with
    // the others when one of them failed), then the largest count's worth of bytes per rank.  `d_src` is copied behind
    // the header (nullptr: the data is in the slot already).  Rank r's data: d_recv + r * x_stride + SH_HEADER.
    // Three failures cannot be made collective and return at once, the other ranks may then wait in the next
    // collective: the all-gather callback's; a failing copy of this function's own (the header out, the counts back);
    // and a fault of an earlier kernel that the synchronisation before the all-gather reports (the device is lost then,
    // and the header could not go out either).  Any other failure a rank meets between two collectives travels as the
    // `status` of the next one.
    int exchange(uint32_t count, uint64_t unit, int32_t status, const void *d_src, const char *what) {
        const auto tx0 = Clock::now();
        if ((uint64_t)SH_HEADER + count * unit > sh->slot_bytes && status == 0) status = HNSW_ERR_OVERFLOW;
        uint32_t hdr[SH_HEADER / 4] = {0};
        hdr[0] = status ? 0 : count;
        hdr[1] = (uint32_t)status;
        HIP_TRY(hipMemcpy(sh->d_send, hdr, SH_HEADER, hipMemcpyHostToDevice));
        if (d_src && hdr[0])
            HIP_TRY(hipMemcpyAsync(sh->d_send + SH_HEADER, d_src, hdr[0] * unit, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        int r = sh->allgather(sh->ctx, SH_HEADER);
        if (r != 0) {
            set_error("sharded build: the all-gather callback failed (%d) on the %s counts", r, what);
            return HNSW_ERR_RCCL;
        }
        std::vector<uint32_t> all((size_t)W * SH_HEADER / 4);
        HIP_TRY(hipMemcpy(all.data(), sh->d_recv, (size_t)W * SH_HEADER, hipMemcpyDeviceToHost));
        uint32_t maxc = 0;
        for (uint32_t k = 0; k < W; k++) {
            const int32_t ks = (int32_t)all[k * (SH_HEADER / 4) + 1];
            if (ks != 0) {  // (the failing rank keeps its own text)
                if (k != sh->rank || status == 0) set_error("sharded build: rank %u reported status %d in the %s phase", k, ks, what);
                return ks;
            }
            x_counts[k] = all[k * (SH_HEADER / 4)];
            maxc = std::max(maxc, x_counts[k]);
        }
        x_stride = (SH_HEADER + maxc * unit + 63) & ~63ull;
        if (x_stride > sh->slot_bytes) {  // cannot happen with honest peers (each checked its own count above)
            set_error("sharded build: a rank announced %u %s, beyond the slot", maxc, what);
            return HNSW_ERR_OVERFLOW;
        }
        if (maxc) {
            r = sh->allgather(sh->ctx, x_stride);
            if (r != 0) {
                set_error("sharded build: the all-gather callback failed (%d) on the %s", r, what);
                return HNSW_ERR_RCCL;
            }
            x_bytes += x_stride * W;
        }
        t_exchange += secs(tx0, Clock::now());
        return HNSW_OK;
    }
    // the removals of every owner's prunes, in every rank's list (phase 3 filters by the owner of the row that loses
    // the edge); the sort below makes the order canonical.  `st`: this rank's status since the record all-gather
    int exchange_removals(int st) {
        if (st == 0) st = counts[3] != 0 ? (int32_t)counts[3] : (counts[1] > REQ_CAP ? HNSW_ERR_OVERFLOW : 0);
        const int rc = exchange(st ? 0 : counts[1], 8, st, dKeyA.p, "removals");
        if (rc != HNSW_OK) return rc;
        uint64_t tot = 0;
        for (uint32_t r = 0; r < W; r++) tot += x_counts[r];
        if (tot > REQ_CAP) {
            set_error("sharded build: %llu removals in one batch, room for %u", (unsigned long long)tot, REQ_CAP);
            return HNSW_ERR_OVERFLOW;
        }
        nrem_all = (uint32_t)tot;
        return HNSW_OK;
    }
    // ... of which this rank sorts and applies those that drop from a row it owns
    int filter_removals() {
        HIP_TRY(hipMemset(cnt + 1, 0, 4));
        for (uint32_t r = 0; r < W; r++) {
            if (x_counts[r] == 0) continue;
            const int rc = filter_edge_records(reinterpret_cast<const uint64_t *>(sh->d_recv + (size_t)r * x_stride + SH_HEADER), nullptr,
                                               x_counts[r], sh->rank, W, dKeyA.as<uint64_t>(), nullptr, cnt + 1, REQ_CAP,
                                               reinterpret_cast<int32_t *>(cnt + 3), nullptr);
            if (rc != HNSW_OK) return rc;
        }
        HIP_TRY(hipMemcpy(&nrem, cnt + 1, 4, hipMemcpyDeviceToHost));
        return HNSW_OK;
    }
    // phase 3: group the removals by row, drop the reverse edges (nothing waits for it in-batch)
    int remove() {
        int rc = sort_edge_keys(dTemp.p, temp_bytes, dKeyA.as<uint64_t>(), dKeyB.as<uint64_t>(), nrem, L, nullptr);
        if (rc != HNSW_OK) return rc;
        ca.keys = dKeyB.as<uint64_t>();
        ca.vals = nullptr;
        ca.count = nrem;
        ca.out_keys = dRef.as<uint64_t>();
        ca.out_count = cnt + 2;
        ca.out_cap = REF_CAP;
        HIP_TRY(hipEventRecord(ev_rem.a, nullptr));
        if ((rc = launch_remove(v, ca, nullptr))) return rc;
        HIP_TRY(hipEventRecord(ev_rem.b, nullptr));
        rem_pending = true;
        return HNSW_OK;
    }
    int collect_remove_time() {  // the drop kernel of the previous batch
        if (!rem_pending) return HNSW_OK;
        HIP_TRY(hipEventSynchronize(ev_rem.b));
        rem_pending = false;
        return ev_rem.add_ms(&t_conn_kernel_ms);
    }
    // the rows this rank changed, to the other replicas.  `st`: this rank's status since the removals exchange
    int ship_rows(int st) {
        uint32_t nchg = 0;
        uint32_t c4[4], lists[HX_CHG_LISTS];
        if (st == 0) st = copy_to_host(lists, dChgCnt.p, sizeof(lists));  // synchronises
        if (st == 0) st = copy_to_host(c4, dCnt.p, 16);
        if (st == 0) {
            st = (int32_t)c4[3];
            uint64_t nchg64 = 0;
            uint32_t longest = 0;
            for (uint32_t c : lists) {
                nchg64 += c;
                longest = std::max(longest, c);
            }
            if (st == 0 && (longest > CHG_LIST_CAP || nchg64 > CHG_CAP || (uint64_t)SH_HEADER + nchg64 * SHIP_UNIT > sh->slot_bytes))
                st = HNSW_ERR_OVERFLOW;
            if (st == 0) {
                nchg = (uint32_t)nchg64;
                st = launch_pack_rows(v, dev.adj0_mut(), dev.adj_up_mut(), dChg.as<uint64_t>(), dChgCnt.as<uint32_t>(),
                                      CHG_LIST_CAP, longest, SHIP, sh->d_send + SH_HEADER, nullptr);
            }
        }
        const int rc = exchange(st ? 0 : nchg, SHIP_UNIT, st, nullptr, "changed rows");
        if (rc != HNSW_OK) return rc;
        n_owned += nchg;
        return HNSW_OK;
    }
    int apply_rows() {  // ... and the other owners' rows into this replica
        for (uint32_t r = 0; r < W; r++) {
            if (r == sh->rank || x_counts[r] == 0) continue;
            const int rc = launch_apply_rows(v, dev.adj0_mut(), dev.adj_up_mut(), sh->d_recv + (size_t)r * x_stride + SH_HEADER,
                                             x_counts[r], SHIP, reinterpret_cast<int32_t *>(cnt + 3), nullptr);
            if (rc != HNSW_OK) return rc;
            n_shipped += x_counts[r];
        }
        // the receive buffer is read by those launches: they finish before the next batch's exchange overwrites it
        return sync_device();
    }
    int clear_counters() {
        HIP_TRY(hipMemset(dCnt.p, 0, 8));                                    // requests, removals
        if (own_rows) HIP_TRY(hipMemset(dChgCnt.p, 0, HX_CHG_LISTS * 4));  // rows this rank changed
        return HNSW_OK;
    }
    // One batch.  Alone, a failure returns at once.  Sharded, `st` keeps a rank-local failure until the next
    // collective, which returns the same status on every rank (after the batch's last collective: in `carry`).
    int batch(const NodeID *ids, size_t B) {
        const auto t0 = Clock::now();
        int st = carry, rc;
        carry = HNSW_OK;
        if (st == 0) st = collect_remove_time();
        if (st == 0) st = clear_counters();
        if (!sh) {
            if (st || (st = phase1(ids, B))) return st;
        } else {
            if (st == 0) st = shard_phase1(ids, B);
            if ((rc = gather_records(st))) return rc;
            st = concat_records();
        }
        const auto t1 = Clock::now();
        if (st == 0) st = connect();
        if (own_rows) {
            if ((rc = exchange_removals(st))) return rc;
            st = filter_removals();
        }
        if (st == 0) st = remove();
        if (own_rows) {
            if ((rc = ship_rows(st))) return rc;
            st = apply_rows();
        }
        if (st == 0 && verbose) st = sync_device();  // only to attribute the time
        if (st != 0 && !sh) return st;
        carry = st;
        t_ins += secs(t0, t1);
        t_conn += secs(t1, Clock::now());
        n_req += nreq_all;
        n_rem += nrem_all;
        n_batches++;
        return HNSW_OK;
    }
    int add_stats(BuildStats &bs, size_t points) {  // what the build read and how long its kernels ran
        unsigned long long rd[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(rd, dRead.p, 32, hipMemcpyDeviceToHost));
        bs.points += points;
        bs.batches += n_batches;
        bs.rows_read += rd[0];
        bs.adj_rows += rd[1];
        bs.adj_ids += rd[2];
        bs.records += n_req;
        bs.removals += n_rem;
        bs.insert_kernel_s += t_kernel_ms * 1e-3;
        bs.connect_kernel_s += t_conn_kernel_ms * 1e-3;
        bs.insert_phase_s += t_ins;
        bs.connect_s += t_conn;
        bs.rows_owned += n_owned;
        bs.rows_received += n_shipped;
        bs.exchange_bytes += x_bytes;
        bs.exchange_s += t_exchange;
        return HNSW_OK;
    }
    // The edges the drop kernel kept because they were a row's last one.  With row ownership every owner's, on every
    // rank, through the build's last collective.  `st`: this rank's status since the last batch's collectives
    int kept_last_edges(int st, std::vector<uint64_t> &refusals) {
        if (st == 0) st = copy_to_host(counts, dCnt.p, 16);
        if (st == 0) {
            if (counts[3] != 0 || counts[2] > REF_CAP) {
                set_error("on-device build: status %d, %u kept-last-edge records", (int)counts[3], counts[2]);
                st = HNSW_ERR_OVERFLOW;
            }
        }
        if (!own_rows) {
            if (st != 0) return st;
            refusals.resize(counts[2]);
            if (counts[2]) HIP_TRY(hipMemcpy(refusals.data(), dRef.p, (size_t)counts[2] * 8, hipMemcpyDeviceToHost));
            return HNSW_OK;
        }
        const int rc = exchange(st ? 0 : counts[2], 8, st, dRef.p, "kept-last-edge records");
        if (rc != HNSW_OK) return rc;
        for (uint32_t r = 0; r < W; r++) {
            const size_t at = refusals.size();
            refusals.resize(at + x_counts[r]);
            if (x_counts[r])
                HIP_TRY(hipMemcpy(&refusals[at], sh->d_recv + (size_t)r * x_stride + SH_HEADER, (size_t)x_counts[r] * 8,
                                  hipMemcpyDeviceToHost));
        }
        if (verbose)
            fprintf(stderr, "\nsharded build, rank %u of %u: phases 2 / 3 on the rows it owns; %zu rows received, %.1f MB through the "
                            "variable-size exchanges in %.2f s\n", sh->rank, W, n_shipped, x_bytes / 1e6, t_exchange);
        return HNSW_OK;
    }
    // The host graph from the device arrays, then the mirror edges: an edge x -> nb that stayed because it was x's
    // last one gets nb -> x back (graph.rs:85-94 keeps both).  `touched`: rows changed since, (layer << 32) | id
    int read_graph(const std::vector<uint64_t> &refusals, std::vector<uint64_t> &touched) {
        for (int pass = 0; pass < 2; pass++) {
            std::vector<std::vector<NodeID>> &rowsv = pass == 0 ? host.adj0 : host.adj_up;
            const uint32_t S = pass == 0 ? v.S0 : v.S1;
            if (rowsv.empty()) continue;
            // pieces of the array arrive through pinned buffers; the threads turn each into the host's rows while
            // the next one is on the wire
            const int rc = dev.read_adjacency(pass, rowsv.size(), [&](uint64_t plo, uint64_t phi, const uint32_t *data) {
                const unsigned nt = (unsigned)std::min<uint64_t>(nb_threads, std::max<uint64_t>(1, (phi - plo) / 16384));
                for_ranges(nt, plo, phi, [&](uint64_t lo, uint64_t hi) {
                    std::vector<NodeID> ids_of_row(S);
                    for (uint64_t r = lo; r < hi; r++) {
                        const uint32_t *src = data + (r - plo) * (size_t)S;
                        uint32_t deg = 0;
                        for (uint32_t k = 0; k < S; k++)
                            if (src[k] != UINT32_MAX) ids_of_row[deg++] = src[k];
                        rowsv[r].assign(ids_of_row.begin(), ids_of_row.begin() + deg);  // one allocation of the row's size
                    }
                });
            });
            if (rc != HNSW_OK) return rc;
        }
        const uint64_t id_mask = (1ull << HX_EDGE_ID_BITS) - 1;
        for (uint64_t key : refusals) {
            const uint32_t layer = (uint32_t)(key >> (2 * HX_EDGE_ID_BITS));
            const NodeID x = (NodeID)((key >> HX_EDGE_ID_BITS) & id_mask), nb = (NodeID)(key & id_mask);
            std::vector<NodeID> &row = host.row(layer, nb);
            const std::vector<NodeID> &back = host.row(layer, x);
            if (std::find(back.begin(), back.end(), nb) != back.end() && std::find(row.begin(), row.end(), x) == row.end()) {
                row.push_back(x);
                touched.push_back(((uint64_t)layer << 32) | nb);
            }
        }
        return HNSW_OK;
    }
};

}  // namespace

uint64_t shard_slot_bytes(uint32_t m, uint32_t world) {
    const uint64_t rows = (uint64_t)SH_HEADER + (uint64_t)shard_slot_rows(m, world) * (8 + 4ull * shard_ship_slots(m));
    return (std::max(shard_record_bytes(m, world), rows) + 255) & ~255ull;
}

int gpu_insert_bulk_full(const BuildTarget &t, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                         const uint8_t *levels, const ShardCtx *sh) {
    HostIndex &host = t.host;
    if (nb_threads == 0) nb_threads = 1;
    int rc = check_build_params(host);
    if (rc != HNSW_OK) return rc;
    if (host.len() + n >= (1ull << HX_EDGE_ID_BITS)) {  // edge records carry 30-bit ids
        if (!sh) return gpu_insert_bulk(t, rows, n, nb_threads, verbose, levels);
        set_error("sharded build: ids must stay below 2^30");
        return HNSW_ERR_ARG;
    }
    const uint64_t n_before = host.len();
    std::vector<NodeID> ids;
    const auto t_enter = Clock::now();
    if ((rc = host.store_points(rows, n, levels, &ids, nb_threads, /*reserve_rows=*/false))) return rc;
    const auto t_stored = Clock::now();
    host.prepare_build();
    const auto t_prep = Clock::now();
    const std::vector<NodeID> order = insertion_order(host, ids);
    const auto t_ordered = Clock::now();
    const uint64_t SEED = 2048;
    InserterPtr ins = make_inserter(host);
    if (verbose)
        fprintf(stderr, "host phases before the seed: store_points %.2f s, locks %.2f s, order %.2f s, inserter %.2f s\n",
                secs(t_enter, t_stored), secs(t_stored, t_prep), secs(t_prep, t_ordered), secs(t_ordered, Clock::now()));
    // The first points are inserted one after the other on the host (the graph depends on it).  Unless they are all
    // there is to insert, that runs WHILE the vector rows travel to HBM (DeviceIndex::upload's side job): the rows are
    // immutable once stored, the adjacency -- which the seed writes -- is packed after the seed has finished.
    const size_t take = n_before < SEED ? std::min<size_t>(order.size(), SEED - n_before) : 0;
    std::vector<uint64_t> restore;
    auto seed_and_clamp = [&]() -> int {
        for (size_t i = 0; i < take; i++)
            if (int r = host.insert(order[i], *ins)) return r;
        clamp_rows_to_cap(host, &restore);
        return HNSW_OK;
    };
    if (take == order.size() || host.nb_layers() > 16) {  // nothing for the device (edge records carry 4-bit layers)
        for (NodeID p : order)
            if ((rc = host.insert(p, *ins))) return rc;
        host.version++;
        return HNSW_OK;
    }
    size_t pos = take;
    const auto t_start = Clock::now();
    if ((rc = upload_for_build(t, seed_and_clamp))) return rc;
    const auto t_uploaded = Clock::now();
    FullBuild b(t, sh, nb_threads, verbose);
    uint64_t connected = n_before + pos;
    if ((rc = b.setup(t.batches, order, pos, connected))) return rc;
    // the capacity of the new points' host rows (one small allocation each) is reserved by other threads while the
    // GPU runs the batches: nothing touches the host graph until the read-back below
    {
        HostIndex *hp = &host;
        const NodeID first_new = (NodeID)n_before;
        const uint32_t threads = std::max(1u, nb_threads / 2);
        b.row_reserve = std::thread([hp, first_new, n, threads] { hp->reserve_layer0_rows(first_new, n, threads); });
    }
    const auto t_loop0 = Clock::now();
    while (pos < order.size()) {
        const size_t B = t.batches.next(order.size() - pos, connected, FullBuild::BMAX);
        if ((rc = b.batch(&order[pos], B))) return rc;
        pos += B;
        connected += B;
        if (verbose && (b.n_batches % 64 == 0 || pos == order.size()))
            fprintf(stderr, "\rBuilding HNSW index on the GPU %zu/%zu", pos, order.size());
    }
    // ---- finish: statistics, the kept-last-edge records, the host graph, the points the device could not serve ----
    int st = b.carry;
    if (st == 0) st = b.collect_remove_time();
    if (st == 0) st = b.add_stats(t.stats, order.size());
    if (b.row_reserve.joinable()) b.row_reserve.join();
    const auto t_sync0 = Clock::now();
    std::vector<uint64_t> refusals, touched;
    if ((rc = b.kept_last_edges(st, refusals))) return rc;
    t.stats.cpu_path_points += b.failed.size();
    t.stats.rerun_points += b.n_again;
    t.stats.kept_last_edges += refusals.size() + restore.size();  // sharded: every owner's refusals, on every rank
    refusals.insert(refusals.end(), restore.begin(), restore.end());
    if ((rc = b.read_graph(refusals, touched))) return rc;
    const bool device_is_the_graph = b.failed.empty();
    std::sort(b.failed.begin(), b.failed.end());  // points the kernel could not serve take the CPU path
    for (NodeID p : b.failed)
        if ((rc = host.insert(p, *ins))) return rc;
    if (verbose) {
        fprintf(stderr,
                "\non-device build (device connect): %zu batches in %.2f s (insert kernel %.2f s, sort + connect + "
                "remove %.2f s, graph read-back %.2f s); %zu requests, %zu removals, %u kept-last-edge, %zu points "
                "ran again with a larger visited table, %zu took the CPU path\n",
                b.n_batches, secs(t_start, Clock::now()), b.t_ins, b.t_conn, secs(t_sync0, Clock::now()), b.n_req, b.n_rem,
                b.counts[2], b.n_again, b.failed.size());
        fprintf(stderr,
                "host phases: store_points %.2f s, levels + order %.2f s, first %llu points on the CPU beside the upload %.2f s, "
                "buffers %.2f s, batch loop %.2f s\n",
                secs(t_enter, t_stored), secs(t_stored, t_start), (unsigned long long)SEED, secs(t_start, t_uploaded),
                secs(t_uploaded, t_loop0), secs(t_loop0, t_sync0));
    }
    host.version++;
    // the adjacency in HBM is the graph just read back: patch the few rows changed since and keep the snapshot
    // (a build of tens of GB is otherwise followed by an upload of the same tens of GB)
    if (device_is_the_graph && !sw::reupload())
        (void)t.dev.refresh_rows(host, touched);
    return HNSW_OK;
}

}  // namespace hx
