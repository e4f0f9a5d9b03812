// capi.cpp -- the extern "C" surface of libhnsw_mi355x.so (include/hnsw_mi355x.h): argument checks, dispatch,
// accessors and persistence.  Host logic only; the search entry points upload the index snapshot to HBM on demand and
// hand over to search_host.cpp / filter_host.cpp (batches) or coalesce.cpp (hnsw_search), which launch the HIP kernels.  There is no CPU
// search path.  Options and statistics are options.cpp's tables, the ground-truth scans ground_truth.cpp's, snapshot
// replication snapshot.cpp's.  (The two entry points of partitioned search are partition.cpp's.)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "handle.h"
#include "search_host.h"
#include "switches.h"

using hx::check_search_args;
using hx::cosine_queries;
using hx::DevBuf;
using hx::ensure_uploaded;
using hx::index_len;
using hx::is_replica;
using hx::reject_replica;
using hx::set_error;

namespace hx {  // what handle.h declares

int reject_replica(const hnsw_index *h, const char *what) {
    if (!is_replica(h)) return HNSW_OK;
    set_error("%s: this handle is a device-only replica (hnsw_snapshot_adopt); it holds no host copy of the index", what);
    return HNSW_ERR_ARG;
}

int ensure_uploaded(hnsw_index *h) {
    std::lock_guard<std::mutex> g(h->mu);
    if (is_replica(h) && !h->dev.valid) {
        set_error("replica snapshot not committed (hnsw_snapshot_commit)");
        return HNSW_ERR_ARG;
    }
    if (!h->dev.current(*h->host)) {
        int rc = h->dev.upload(*h->host, h->device);
        if (rc != HNSW_OK) return rc;
        h->device = h->dev.device;
        h->n_uploads.fetch_add(1, std::memory_order_relaxed);
        // searches above ef 320 take their visited set's second level from the device's stream-ordered pool, launch after
        // launch: the pool keeps what is given back instead of returning it to the driver at every synchronisation
        hipMemPool_t pool = nullptr;
        if (hipDeviceGetDefaultMemPool(&pool, h->dev.device) == hipSuccess && pool != nullptr) {
            uint64_t keep = 1ull << 30;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        (void)hipGetLastError();
    }
    hipError_t e = hipSetDevice(h->dev.device);
    if (e != hipSuccess) {
        set_error("hipSetDevice(%d): %s", h->dev.device, hipGetErrorString(e));
        return HNSW_ERR_HIP;
    }
    return HNSW_OK;
}

int check_search_args(const hnsw_index *h, uint32_t ef) {
    if (!h) {
        set_error("null handle");
        return HNSW_ERR_ARG;
    }
    if (h->incomplete_build) {
        set_error("an on-device build on this handle failed half way; the index is incomplete, discard it");
        return HNSW_ERR_ARG;
    }
    if (index_len(h) == 0) {
        set_error("index is empty");
        return HNSW_ERR_EMPTY;
    }
    // no limit on ef (template.rs:306-311): up to 1024 the list lives in a wave's registers, beyond that in HBM
    // scratch (hx_search_spill_kernel: exact, slow).  2^26 entries only bounds the scratch arithmetic.
    if (ef > (1u << 26)) {
        set_error("ef = %u is above 2^26", ef);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

}  // namespace hx

namespace {

// what the on-device builds read and change
hx::BuildTarget build_target(hnsw_index *h) {
    return {*h->host, h->dev, h->device, {h->build_batch_max, h->build_batch_div}, h->build};
}

// The cosine option on the way in: a unit-length copy of n rows, by the same operations in the same order as
// hx_normalise_rows_kernel (metric.hip) -- one left-to-right f32 sum of squares, correctly rounded sqrt and
// division, no FMA (this file is compiled with -ffp-contract=off).  Returns rows itself when the option is off.
int cosine_rows(const hnsw_index *h, const float *&rows, uint64_t n, std::vector<float> &keep, uint32_t nb_threads = 1) {
    if (!h->cosine || !rows) return HNSW_OK;
    const uint32_t d = h->host->dim;
    keep.resize((size_t)n * d);
    std::atomic<uint64_t> bad{UINT64_MAX};
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const float *x = rows + i * d;
            float s = 0.0f;
            for (uint32_t e = 0; e < d; e++) {
                const float t = x[e] * x[e];
                s += t;
            }
            const float nrm = sqrtf(s);
            // a row without a direction (all zero, or a sum of squares that under- / overflows f32) cannot be put on
            // the unit sphere: refused here by name instead of poisoning distances with inf - inf later
            if (!(nrm > 0.0f) || !std::isfinite(nrm)) {
                uint64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {
                }
                return;
            }
            float *y = &keep[(size_t)i * d];
            for (uint32_t e = 0; e < d; e++) y[e] = x[e] / nrm;
        }
    };
    const unsigned nt = (unsigned)std::min<uint64_t>(std::max(1u, nb_threads), std::max<uint64_t>(1, n / 4096));
    if (nt <= 1) {
        work(0, n);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
        for (auto &t : th) t.join();
    }
    if (bad.load() != UINT64_MAX) {
        set_error("row %llu has no direction (zero, NaN, or a norm outside f32's range): the cosine metric cannot place it",
                  (unsigned long long)bad.load());
        return HNSW_ERR_NAN_INPUT;
    }
    rows = keep.data();
    return HNSW_OK;
}

const uint64_t kNoWords = 0;  // the mask of a filtered call with allow_bits 0 (never read)

// An on-device build that returns an error after it stored the points leaves some of them unconnected
// (and, in the device-connect form, the graph only in HBM): the handle is marked and refuses further use.
// Errors raised before anything was stored (bad rows, bad arguments) leave the index as it was.
template <class F>
int device_build_guard(hnsw_index *h, F &&build) {
    const uint64_t n_before = h->host->len();
    const int rc = build();
    if (rc != HNSW_OK && h->host->len() != n_before) h->incomplete_build = true;
    return rc;
}

}  // namespace

extern "C" {

const char *hnsw_last_error(void) { return hx::get_error(); }
const char *hnsw_version(void) { return "hnsw_mi355x 0.1 (gfx950)"; }

int hnsw_create(uint32_t m, uint32_t ef_cons, uint32_t dim, int vec_kind, hnsw_index **out) {
    if (!out || m < 2 || dim == 0 || (vec_kind != HNSW_VEC_QUANT8 && vec_kind != HNSW_VEC_F32)) {
        set_error("hnsw_create: need m >= 2, dim >= 1 and a valid vector kind");
        return HNSW_ERR_ARG;
    }
    hnsw_index *h = new (std::nothrow) hnsw_index();
    if (!h) return HNSW_ERR_OOM;
    h->host.reset(new hx::HostIndex(m, ef_cons, dim, vec_kind));
    *out = h;
    return HNSW_OK;
}

void hnsw_free(hnsw_index *h) { delete h; }

int hnsw_clone(const hnsw_index *h, hnsw_index **out) {
    if (!h || !out) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_clone");
    hnsw_index *c = new (std::nothrow) hnsw_index();
    if (!c) return HNSW_ERR_OOM;
    c->host.reset(new hx::HostIndex(*h->host));
    c->device = h->device;
    // the handle's options travel with the clone, every one of them (a cosine index that forgot its metric would
    // stop normalising its queries)
    hx::copy_options(c, h);
    c->del.assign_host(h->del.words);
    c->lab.assign_host(h->lab.labels);
    *out = c;
    return HNSW_OK;
}

int hnsw_get_params(const hnsw_index *h, hnsw_params *out) {
    if (!h || !out) return HNSW_ERR_ARG;
    const hx::Params &p = h->host->params;
    memset(out, 0, sizeof(*out));
    out->ep = is_replica(h) ? h->dev.view.ep : p.ep;
    out->vec_kind = (uint32_t)h->host->kind;
    out->m = p.m;
    out->mmax = p.mmax;
    out->mmax0 = p.mmax0;
    out->ml = p.ml;
    out->ef_cons = p.ef_cons;
    out->dim = p.dim;
    return HNSW_OK;
}

int hnsw_set_ep(hnsw_index *h, uint32_t ep) {
    if (h && is_replica(h)) return reject_replica(h, "hnsw_set_ep");
    if (!h || ep >= h->host->len()) {
        set_error("entry point %u out of range", ep);
        return HNSW_ERR_ARG;
    }
    h->host->params.ep = ep;
    h->host->version++;
    return HNSW_OK;
}

int hnsw_insert_bulk(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads, int verbose) {
    return hnsw_insert_bulk_levels(h, rows, n, nb_threads, verbose, nullptr);
}
int hnsw_insert_bulk_levels(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads,
                            int verbose, const uint8_t *levels) {
    if (!h || !rows) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_insert_bulk");
    if (h->incomplete_build) return check_search_args(h, 1);
    std::vector<float> unit;
    if (int crc = cosine_rows(h, rows, n, unit, nb_threads)) return crc;
    if (h->gpu_build == 2) return device_build_guard(h, [&] { return hx::gpu_insert_bulk_full(build_target(h), rows, n, nb_threads, verbose, levels); });
    if (h->gpu_build) return device_build_guard(h, [&] { return hx::gpu_insert_bulk(build_target(h), rows, n, nb_threads, verbose, levels); });
    return h->host->insert_bulk(rows, n, nb_threads, verbose != 0, levels);
}
uint64_t hnsw_sharded_slot_bytes(const hnsw_index *h, uint32_t world) {
    if (!h || world == 0) return 0;
    return hx::shard_slot_bytes((uint32_t)h->host->params.m, world);
}
int hnsw_insert_bulk_sharded(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                             const uint8_t *levels, uint32_t rank, uint32_t world, void *d_send, void *d_recv,
                             uint64_t slot_bytes, hnsw_allgather_fn allgather, void *ctx) {
    if (!h || !rows || world == 0 || rank >= world) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_insert_bulk_sharded");
    std::vector<float> unit;
    if (int crc = cosine_rows(h, rows, n, unit, nb_threads)) return crc;
    hx::ShardCtx sh{rank, world, static_cast<unsigned char *>(d_send), static_cast<unsigned char *>(d_recv), slot_bytes,
                allgather, ctx};
    if (h->incomplete_build) return check_search_args(h, 1);
    return device_build_guard(h, [&] { return hx::gpu_insert_bulk_full(build_target(h), rows, n, nb_threads, verbose, levels, &sh); });
}
int hnsw_insert_bulk_device(hnsw_index *h, const float *rows, uint64_t n, uint32_t nb_threads,
                            int verbose, const uint8_t *levels) {
    if (!h || !rows) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_insert_bulk_device");
    if (h->incomplete_build) return check_search_args(h, 1);
    std::vector<float> unit;
    if (int crc = cosine_rows(h, rows, n, unit, nb_threads)) return crc;
    if (h->gpu_build == 1) return device_build_guard(h, [&] { return hx::gpu_insert_bulk(build_target(h), rows, n, nb_threads, verbose, levels); });
    return device_build_guard(h, [&] { return hx::gpu_insert_bulk_full(build_target(h), rows, n, nb_threads, verbose, levels); });
}
int hnsw_insert_vec(hnsw_index *h, const float *v, uint32_t *out_id) {
    return hnsw_insert_vec_level(h, v, -1, out_id);
}
int hnsw_insert_vec_level(hnsw_index *h, const float *v, int level, uint32_t *out_id) {
    if (!h || !v || level > 255) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_insert_vec");
    if (h->incomplete_build) return check_search_args(h, 1);
    std::vector<float> unit;
    if (int crc = cosine_rows(h, v, 1, unit)) return crc;
    // The reference's callers search right after an insert_vec (eval_glove/src/main.rs:37-41).  When the HBM snapshot
    // was current before the insertion it is patched -- the new row and the adjacency rows the insertion touched --
    // instead of being thrown away and uploaded again by the next search (DeviceIndex::append_point).
    std::lock_guard<std::mutex> g(h->mu);
    const bool live = h->dev.valid && h->dev.current(*h->host) && !hx::sw::reupload();
    std::vector<uint64_t> touched;
    uint32_t id = 0;
    int rc;
    {
        hx::DirtyScope scope(live ? &touched : nullptr);
        rc = h->host->insert_vec(v, level, &id);
    }
    if (rc != HNSW_OK) return rc;
    if (out_id) *out_id = id;
    if (live) {
        if (h->dev.append_point(*h->host, id, touched))
            h->n_point_patches.fetch_add(1, std::memory_order_relaxed);
        else
            h->n_patch_fallbacks.fetch_add(1, std::memory_order_relaxed);
    }
    return HNSW_OK;
}
int hnsw_import_points(hnsw_index *h, const float *rows, uint64_t n, const uint8_t *levels) {
    if (!h || !rows) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_import_points");
    std::vector<float> unit;
    if (int crc = cosine_rows(h, rows, n, unit)) return crc;
    return h->host->import_points(rows, n, levels);
}
int hnsw_import_layer(hnsw_index *h, uint32_t layer, uint64_t n_nodes, const uint32_t *node_ids,
                      const uint64_t *offsets, const uint32_t *nbrs) {
    if (!h || !node_ids || !offsets) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_import_layer");
    return h->host->import_layer(layer, n_nodes, node_ids, offsets, nbrs);
}

// ---- query -------------------------------------------------------------------------------------
int hnsw_search(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, uint32_t *ids,
                uint32_t *count) {
    // concurrent callers are gathered into one launch (coalesce.h); ef beyond the register-resident list
    // (the HBM-spill kernel) and result lists of thousands of ids go by themselves
    if (h && q && ids && n > 0 && n <= 1024 && ef <= 1024 && h->co.window_us.load(std::memory_order_relaxed) >= 0) {
        const int rc = check_search_args(h, ef);
        if (rc != HNSW_OK) return rc;
        return hx::search_coalesced(h, q, n, ef, ids, count);
    }
    return hnsw_search_batch(h, q, 1, n, ef, ids, nullptr, count, nullptr);
}

int hnsw_search_batch(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                      uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || !ids || nq > 0x7FFFFFFFull) return HNSW_ERR_ARG;
    if (n == 0) {
        if (counts) memset(counts, 0, nq * 4);
        return HNSW_OK;
    }
    if (h->del.count) {  // ids are deleted: the filtered search over the undeleted ones (include/hnsw_mi355x.h)
        return hx::search_filtered_checked(h, Q, nq, n, ef, hx::Filter{}, false, ids, dists, counts, stats, nullptr);
    }
    hx::DevView dummy{};
    dummy.nb_layers = hnsw_layer_count(h);  // the host index's, or the adopted snapshot's for a replica
    hx::SearchArgs a = hx::ann_args(dummy, nullptr, n, ef, nullptr, nullptr, nullptr, nullptr);
    return hx::search_host(h, a, Q, nq, ids, dists, counts, stats, nullptr);
}

// ---- filtered searches -------------------------------------------------------------------------------------------
// Every entry point states its Filter (search_host.h) and the text of its own missing-argument error, if it has one to
// report; the two helpers below run the checks in one order -- the handle, the set, an empty call, the entry point's
// own arguments, the length of a range list -- and make the one call.
#define HX_STR2(x) #x
#define HX_STR(x) HX_STR2(x)
static const char *const kNeedsMask = "filtered search: needs queries, an id buffer, a mask when allow_bits > 0 and n <= " HX_STR(HX_FILT_MAX_N);
static const char *const kNeedsMaskOf = "filtered search: needs the mask of every query";
static const char *const kNeedsRange = "filtered search: needs the label range (lo and hi) of every query";
static const char *const kNeedsRanges = "filtered search: needs the label ranges (lo and hi) of every query";

static int check_set(const hnsw_index *h, const hnsw_mask_set *set) {
    if (!set || set->owner != h) {
        set_error(set ? "filtered search: the mask set belongs to another handle" : "filtered search: needs a mask set");
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

static int check_range_list(uint32_t n_ranges) {
    if (n_ranges == 0 || n_ranges > HNSW_RANGES_MAX) {
        set_error("filtered search: needs 1 to %d label ranges per query, got %u", HNSW_RANGES_MAX, n_ranges);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

static hx::Filter make_filter(hx::Filter::Family family, hx::Filter::Rows rows, hnsw_mask_set *set, const uint32_t *mask_of,
                              uint32_t K = 0, const uint32_t *lo = nullptr, const uint32_t *hi = nullptr) {
    hx::Filter f;
    f.family = family, f.rows = rows, f.set = set, f.mask_of = mask_of, f.K = K, f.lo = lo, f.hi = hi;
    return f;
}

static int filtered_host(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef, hx::Filter f, const char *missing,
                         uint32_t *ids, float *dists, uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK || (f.rows == hx::Filter::SET && (rc = check_set(h, f.set)))) return rc;
    if (nq == 0) return HNSW_OK;
    if (missing) {
        set_error("%s", missing);
        return HNSW_ERR_ARG;
    }
    if (f.family == hx::Filter::RANGES && (rc = check_range_list(f.K))) return rc;
    std::vector<uint32_t> row0;
    if (f.rows == hx::Filter::SET && !f.mask_of && nq <= 0x7FFFFFFFull) {  // every query under row 0 (more queries are refused below)
        row0.assign(nq, 0);
        f.mask_of = row0.data();
    }
    return hx::search_filtered_checked(h, Q, nq, n, ef, f, false, ids, dists, counts, stats, paths);
}

// ... of a device-pointer call: mask_of, lo and hi are the caller's device memory (ranged: the entry point takes ranges)
static int filtered_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef, hx::Filter f, bool ranged,
                           uint32_t *d_ids, float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream,
                           bool finish, uint8_t *paths) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK || (f.rows == hx::Filter::SET && (rc = check_set(h, f.set)))) return rc;
    if (nq == 0 || n == 0) return HNSW_OK;
    if (!d_Q || !d_ids || !d_stats || (ranged && (!f.lo || !f.hi)) || nq > 0x7FFFFFFFull) {
        set_error(ranged ? "filtered device search: needs queries, their label ranges, an id buffer and a stats buffer in HBM"
                         : "filtered device search: needs queries, an id buffer and a stats buffer in HBM");
        return HNSW_ERR_ARG;
    }
    if (f.family == hx::Filter::RANGES && (rc = check_range_list(f.K))) return rc;
    f.on_device = true;
    return hx::search_device_filtered(h, f, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats, static_cast<hipStream_t>(stream),
                                      finish, paths);
}

int hnsw_search_batch_filtered(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                               const uint64_t *allow, uint64_t allow_bits, uint32_t *ids, float *dists,
                               uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    // (a call without a mask allows nothing: kNoWords stands for its empty mask)
    hx::Filter f = make_filter(hx::Filter::MASK, hx::Filter::ONE, nullptr, nullptr);
    f.masks = allow ? allow : &kNoWords;
    f.allow_bits = allow ? allow_bits : 0;
    return filtered_host(h, Q, nq, n, ef, f, !allow && allow_bits != 0 ? kNeedsMask : nullptr, ids, dists, counts, stats, paths);
}

int hnsw_search_batch_filtered_multi(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                     const uint64_t *masks, uint32_t n_masks, uint64_t allow_bits,
                                     const uint32_t *mask_of, uint32_t *ids, float *dists, uint32_t *counts,
                                     hnsw_query_stats *stats, uint8_t *paths) {
    hx::Filter f = make_filter(hx::Filter::MULTI, hx::Filter::MANY, nullptr, mask_of);
    f.masks = masks, f.allow_bits = allow_bits, f.n_masks = n_masks;
    return filtered_host(h, Q, nq, n, ef, f, !mask_of ? kNeedsMaskOf : nullptr, ids, dists, counts, stats, paths);
}

// ---- searches under a resident mask set (mask_set.h) --------------------------------------------------------
int hnsw_search_batch_filtered_set(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                   hnsw_mask_set *set, const uint32_t *mask_of, uint32_t *ids, float *dists,
                                   uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    return filtered_host(h, Q, nq, n, ef, make_filter(hx::Filter::OF_SET, hx::Filter::SET, set, mask_of), nullptr, ids, dists,
                         counts, stats, paths);
}

int hnsw_search_batch_filtered_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                      hnsw_mask_set *set, const uint32_t *d_mask_of, uint32_t *d_ids, float *d_dists,
                                      uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::OF_SET, hx::Filter::SET, set, d_mask_of), false, d_ids,
                           d_dists, d_counts, d_stats, stream, false, nullptr);
}

int hnsw_search_batch_filtered_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                             hnsw_mask_set *set, const uint32_t *d_mask_of, uint32_t *d_ids,
                                             float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream,
                                             uint8_t *paths) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::OF_SET, hx::Filter::SET, set, d_mask_of), false, d_ids,
                           d_dists, d_counts, d_stats, stream, true, paths);
}

// ---- searches under a label range (labels.h) -----------------------------------------------------------------
int hnsw_search_batch_filtered_range(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                     const uint32_t *lo, const uint32_t *hi, uint32_t *ids, float *dists,
                                     uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    return filtered_host(h, Q, nq, n, ef, make_filter(hx::Filter::RANGE, hx::Filter::ALL, nullptr, nullptr, 1, lo, hi),
                         !lo || !hi ? kNeedsRange : nullptr, ids, dists, counts, stats, paths);
}

int hnsw_search_batch_filtered_range_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                            const uint32_t *d_lo, const uint32_t *d_hi, uint32_t *d_ids,
                                            float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                            void *stream) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::RANGE, hx::Filter::ALL, nullptr, nullptr, 1, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, false, nullptr);
}

int hnsw_search_batch_filtered_range_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                   uint32_t ef, const uint32_t *d_lo, const uint32_t *d_hi,
                                                   uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                                   hnsw_query_stats *d_stats, void *stream, uint8_t *paths) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::RANGE, hx::Filter::ALL, nullptr, nullptr, 1, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, true, paths);
}

// ---- searches under a label range AND a row of a resident mask set ------------------------------------------------
int hnsw_search_batch_filtered_set_range(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                         hnsw_mask_set *set, const uint32_t *mask_of, const uint32_t *lo,
                                         const uint32_t *hi, uint32_t *ids, float *dists, uint32_t *counts,
                                         hnsw_query_stats *stats, uint8_t *paths) {
    return filtered_host(h, Q, nq, n, ef, make_filter(hx::Filter::SET_RANGE, hx::Filter::SET, set, mask_of, 1, lo, hi),
                         !lo || !hi ? kNeedsRange : nullptr, ids, dists, counts, stats, paths);
}

int hnsw_search_batch_filtered_set_range_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                                hnsw_mask_set *set, const uint32_t *d_mask_of, const uint32_t *d_lo,
                                                const uint32_t *d_hi, uint32_t *d_ids, float *d_dists,
                                                uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::SET_RANGE, hx::Filter::SET, set, d_mask_of, 1, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, false, nullptr);
}

int hnsw_search_batch_filtered_set_range_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                       uint32_t ef, hnsw_mask_set *set, const uint32_t *d_mask_of,
                                                       const uint32_t *d_lo, const uint32_t *d_hi, uint32_t *d_ids,
                                                       float *d_dists, uint32_t *d_counts, hnsw_query_stats *d_stats,
                                                       void *stream, uint8_t *paths) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::SET_RANGE, hx::Filter::SET, set, d_mask_of, 1, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, true, paths);
}

// ---- one query under a row of a resident set AND a label range, gathered with its concurrent callers (coalesce.h) -------
int hnsw_search_filtered(hnsw_index *h, const float *q, uint32_t n, uint32_t ef, hnsw_mask_set *set, uint32_t row,
                         uint32_t lo, uint32_t hi, uint32_t *ids, float *dists, uint32_t *count, uint8_t *path) {
    // every argument error before the device is touched
    if (!h || !q || !ids || !count) {
        set_error("filtered search: needs a handle, a query, an id buffer and a count");
        return HNSW_ERR_ARG;
    }
    if (n > HX_FILT_MAX_N) {
        set_error("filtered search: needs n <= %d", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    if (!set && row != HNSW_MASK_NONE) {
        set_error("filtered search: a row needs its mask set");
        return HNSW_ERR_ARG;
    }
    int rc;
    if (set && (rc = check_set(h, set))) return rc;
    if (set && row != HNSW_MASK_NONE && row >= set->n_masks) {
        set_error("filtered search: query 0 names mask %u of %u", row, set->n_masks);
        return HNSW_ERR_ARG;
    }
    if ((rc = check_search_args(h, ef)) != HNSW_OK) return rc;
    *count = 0;
    if (n == 0) return HNSW_OK;
    // alone: the window is off, or ef' is beyond the graph path's maximum -- an error of the calls on the graph path only,
    // which the exact-path calls of the same batch must not see
    const bool alone = h->co.window_us.load(std::memory_order_relaxed) < 0 || std::max(ef, n) > HX_FILT_MAX_EF;
    return hx::search_filtered_coalesced(h, q, n, ef, set, row, lo, hi, ids, dists, count, path, alone);
}

// ---- searches under a list of label ranges per query ---------------------------------------------------------------
int hnsw_search_batch_filtered_ranges(hnsw_index *h, const float *Q, uint64_t nq, uint32_t n, uint32_t ef,
                                      uint32_t n_ranges, const uint32_t *lo, const uint32_t *hi, uint32_t *ids,
                                      float *dists, uint32_t *counts, hnsw_query_stats *stats, uint8_t *paths) {
    return filtered_host(h, Q, nq, n, ef, make_filter(hx::Filter::RANGES, hx::Filter::ALL, nullptr, nullptr, n_ranges, lo, hi),
                         !lo || !hi ? kNeedsRanges : nullptr, ids, dists, counts, stats, paths);
}

int hnsw_search_batch_filtered_ranges_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                             uint32_t n_ranges, const uint32_t *d_lo, const uint32_t *d_hi,
                                             uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                             hnsw_query_stats *d_stats, void *stream) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::RANGES, hx::Filter::ALL, nullptr, nullptr, n_ranges, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, false, nullptr);
}

int hnsw_search_batch_filtered_ranges_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n,
                                                    uint32_t ef, uint32_t n_ranges, const uint32_t *d_lo,
                                                    const uint32_t *d_hi, uint32_t *d_ids, float *d_dists,
                                                    uint32_t *d_counts, hnsw_query_stats *d_stats, void *stream,
                                                    uint8_t *paths) {
    return filtered_device(h, d_Q, nq, n, ef, make_filter(hx::Filter::RANGES, hx::Filter::ALL, nullptr, nullptr, n_ranges, d_lo, d_hi),
                           true, d_ids, d_dists, d_counts, d_stats, stream, true, paths);
}

int hnsw_count_labels_in_ranges(const hnsw_index *h, const uint32_t *lo, const uint32_t *hi, uint32_t k,
                                uint64_t *count) {
    if (!h || !count || (k && (!lo || !hi)) || k > HNSW_RANGES_MAX) {
        set_error("hnsw_count_labels_in_ranges: needs a handle, a result and at most %d ranges", HNSW_RANGES_MAX);
        return HNSW_ERR_ARG;
    }
    // the planner's count: the sorted copy of the undeleted ids' labels, the disjoint members' slices summed
    hnsw_index *hm = const_cast<hnsw_index *>(h);  // (the sorted copy is a cache, made under its mutex)
    std::lock_guard<std::mutex> lg(hm->lab.mu);
    hm->lab.sort_for(hm->del, index_len(h));
    uint64_t A = 0;
    for (uint64_t m : hx::LabelColumn::canonical(lo, hi, k)) A += hm->lab.count((uint32_t)(m >> 32), (uint32_t)m);
    *count = A;
    return HNSW_OK;
}

int hnsw_search_batch_device(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                             uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                             hnsw_query_stats *d_stats, void *stream) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0 || n == 0) return HNSW_OK;
    if (!d_Q || !d_ids || !d_stats || nq > 0x7FFFFFFFull) return HNSW_ERR_ARG;
    if (h->del.count)
        return hx::search_device_filtered(h, hx::Filter{}, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats,
                                          static_cast<hipStream_t>(stream), false, nullptr);
    rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    hx::DeviceQueries dq;
    if ((rc = dq.prepare(h, d_Q, nq, static_cast<hipStream_t>(stream)))) return rc;
    hx::SearchArgs a = hx::ann_args(h->dev.view, dq.q, n, ef, d_ids, d_dists, d_counts, d_stats);
#ifdef HX_STAMPS
    a.dbg = reinterpret_cast<unsigned long long *>(hx::sw::dbg_ptr());
#endif
    return hx::launch_search(h->dev.view, a, (uint32_t)nq, 0, static_cast<hipStream_t>(stream));
}

// Completes a hnsw_search_batch_device call (search_host.h: search_device_finish, search_device_filtered)
int hnsw_search_batch_device_finish(hnsw_index *h, const float *d_Q, uint64_t nq, uint32_t n, uint32_t ef,
                                    uint32_t *d_ids, float *d_dists, uint32_t *d_counts,
                                    hnsw_query_stats *d_stats, void *stream_v) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (nq == 0 || n == 0) return HNSW_OK;
    if (!d_Q || !d_ids || !d_stats || nq > 0x7FFFFFFFull) return HNSW_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (h->del.count)
        return hx::search_device_filtered(h, hx::Filter{}, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats, stream, true, nullptr);
    return hx::search_device_finish(h, d_Q, nq, n, ef, d_ids, d_dists, d_counts, d_stats, stream);
}

int hnsw_distance_batch(hnsw_index *h, const float *q, const uint32_t *ids, uint64_t k, float *out) {
    int rc = check_search_args(h, 1);
    if (rc != HNSW_OK) return rc;
    if (k == 0) return HNSW_OK;
    if (!q || !ids || !out) return HNSW_ERR_ARG;
    rc = ensure_uploaded(h);
    if (rc != HNSW_OK) return rc;
    const hx::DevView &v = h->dev.view;
    DevBuf dq, dids, dout, dst;
    if ((rc = dq.alloc(v.dim * 4)) || (rc = dids.alloc(k * 4)) || (rc = dout.alloc(k * 4)) ||
        (rc = dst.alloc(4)))
        return rc;
    HIP_TRY(hipMemcpy(dq.p, q, v.dim * 4, hipMemcpyHostToDevice));
    if ((rc = cosine_queries(h, dq.p, 1, nullptr))) return rc;
    HIP_TRY(hipMemcpy(dids.p, ids, k * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dst.p, 0, 4));
    rc = hx::launch_distance_batch(v, dq.as<float>(), dids.as<uint32_t>(), k, dout.as<float>(),
                                   dst.as<int32_t>(), nullptr);
    if (rc != HNSW_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    int32_t st = 0;
    HIP_TRY(hipMemcpy(&st, dst.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out, dout.p, k * 4, hipMemcpyDeviceToHost));
    if (st != HNSW_OK) {
        set_error(st == HNSW_ERR_NAN_INPUT ? "NaN in the query" : "point id out of range");
        return st;
    }
    return HNSW_OK;
}

int hnsw_search_layer(hnsw_index *h, uint32_t layer, const float *q, const uint32_t *entry_ids,
                      uint32_t n_entry, uint32_t ef, uint32_t *out_ids, float *out_dists,
                      uint32_t *out_count, hnsw_query_stats *stats) {
    int rc = check_search_args(h, ef);
    if (rc != HNSW_OK) return rc;
    if (!q || !entry_ids || !out_ids || !out_count || n_entry == 0 || ef == 0) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_search_layer (the seam checks its entry set against the host graph)");
    if (layer >= hnsw_layer_count(h)) {
        set_error("Layer %u not found in the structure.", layer);  // layers.rs:25-30 panics
        return HNSW_ERR_ARG;
    }
    if (n_entry > ef) {
        set_error("search_layer seam: the entry set (%u) may not be larger than ef (%u)", n_entry, ef);
        return HNSW_ERR_ARG;
    }
    for (uint32_t i = 0; i < n_entry; i++) {
        if (!h->host->in_layer(layer, entry_ids[i])) {
            set_error("entry %u is not in layer %u", entry_ids[i], layer);
            return HNSW_ERR_NODE_NOT_IN_GRAPH;
        }
        for (uint32_t j = 0; j < i; j++)
            if (entry_ids[j] == entry_ids[i]) {
                set_error("duplicate entry %u", entry_ids[i]);
                return HNSW_ERR_ARG;
            }
    }
    hx::SearchArgs a{};
    a.n_entry = n_entry;
    a.layer_hi = a.layer_lo = (int32_t)layer;
    a.ef_upper = 1;
    a.ef_bottom = ef;
    a.n = ef;
    std::vector<uint32_t> ids(ef);
    std::vector<float> dists(ef);
    uint32_t count = 0;
    hnsw_query_stats st{};
    rc = hx::search_host(h, a, q, 1, ids.data(), dists.data(), &count, &st, entry_ids);
    if (rc != HNSW_OK) return rc;
    for (uint32_t i = 0; i < count; i++) {
        out_ids[i] = ids[i];
        if (out_dists) out_dists[i] = dists[i];
    }
    *out_count = count;
    if (stats) *stats = st;
    return HNSW_OK;
}

// ---- ground truth (ground_truth.cpp) ----------------------------------------------------------------------------
int hnsw_brute_force(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists) {
    int rc = check_search_args(h, 1);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    if (!Q || !ids || k == 0 || k > 64) {
        set_error("brute force supports 1 <= k <= 64");
        return HNSW_ERR_ARG;
    }
    return hx::exact_scan(h, Q, nq, k, ids, dists);
}

int hnsw_brute_force_fast(hnsw_index *h, const float *Q, uint64_t nq, uint32_t k, uint32_t *ids, float *dists) {
    int rc = check_search_args(h, 1);
    if (rc != HNSW_OK) return rc;
    if (nq == 0) return HNSW_OK;
    const uint32_t K2 = hx::brute_mfma_k2();
    if (!Q || !ids || k == 0 || k + 8 > K2) {
        set_error("the MFMA scan supports 1 <= k <= %u", K2 - 8);
        return HNSW_ERR_ARG;
    }
    return hx::mfma_scan(h, Q, nq, k, ids, dists);
}

// ---- accessors -----------------------------------------------------------------------------------
uint64_t hnsw_len(const hnsw_index *h) { return h ? index_len(h) : 0; }

int hnsw_distance(const hnsw_index *h, uint32_t a, uint32_t b, float *out) {
    if (!h || !out) return HNSW_ERR_ARG;
    hx::PointView pa, pb;
    if (!h->host->get_point(a, &pa) || !h->host->get_point(b, &pb)) return HNSW_ERR_ARG;  // None
    *out = h->host->dist2other(pa, pb);
    return HNSW_OK;
}

int hnsw_get_vector(const hnsw_index *h, uint32_t id, float *out) {
    if (!h || !out) return HNSW_ERR_ARG;
    hx::PointView p;
    if (!h->host->get_point(id, &p)) return HNSW_ERR_ARG;
    const uint32_t d = h->host->dim;
    if (h->host->kind == HNSW_VEC_QUANT8)
        for (uint32_t i = 0; i < d; i++) out[i] = ((float)p.codes[i] * p.delta) + p.min;  // quant.rs:79-83
    else
        memcpy(out, p.vals, 4 * (size_t)d);
    return HNSW_OK;
}

int hnsw_get_level(const hnsw_index *h, uint32_t id, uint32_t *out) {
    if (!h || !out || id >= h->host->len()) return HNSW_ERR_ARG;
    *out = h->host->levels[id];
    return HNSW_OK;
}

int hnsw_get_quant(const hnsw_index *h, uint32_t id, uint8_t *codes, float *min_out, float *delta_out) {
    if (!h || h->host->kind != HNSW_VEC_QUANT8 || id >= h->host->len()) return HNSW_ERR_ARG;
    if (codes) memcpy(codes, &h->host->codes[(size_t)id * h->host->dim], h->host->dim);
    if (min_out) *min_out = h->host->mins[id];
    if (delta_out) *delta_out = h->host->deltas[id];
    return HNSW_OK;
}

uint32_t hnsw_layer_count(const hnsw_index *h) {
    if (!h) return 0;
    return is_replica(h) ? h->dev.view.nb_layers : h->host->nb_layers();
}
uint64_t hnsw_layer_nb_nodes(const hnsw_index *h, uint32_t layer) {
    return (h && layer < h->host->nb_layers()) ? h->host->layer_nodes[layer].size() : 0;
}
uint32_t hnsw_layer_m(const hnsw_index *h, uint32_t layer) {
    return (h && layer < h->host->nb_layers()) ? (uint32_t)h->host->layer_m(layer) : 0;
}

int hnsw_layer_nodes(const hnsw_index *h, uint32_t layer, uint32_t *out, uint64_t cap, uint64_t *n) {
    if (!h || layer >= h->host->nb_layers()) return HNSW_ERR_ARG;
    const std::vector<hx::NodeID> &ids = h->host->layer_nodes[layer];
    if (n) *n = ids.size();
    if (out)
        for (uint64_t i = 0; i < ids.size() && i < cap; i++) out[i] = ids[i];
    return HNSW_OK;
}

int hnsw_neighbors(const hnsw_index *h, uint32_t layer, uint32_t id, uint32_t *buf, uint32_t cap,
                   uint32_t *deg) {
    if (!h) return HNSW_ERR_ARG;
    if (!h->host->in_layer(layer, id)) {
        set_error("node %u not in graph (layer %u)", id, layer);
        return HNSW_ERR_NODE_NOT_IN_GRAPH;
    }
    std::vector<hx::NodeID> nb = h->host->row(layer, id);
    std::sort(nb.begin(), nb.end());
    if (deg) *deg = (uint32_t)nb.size();
    if (buf)
        for (uint32_t i = 0; i < nb.size() && i < cap; i++) buf[i] = nb[i];
    return HNSW_OK;
}

int hnsw_export_layer(const hnsw_index *h, uint32_t layer, uint32_t *node_ids, uint64_t *offsets,
                      uint32_t *nbrs, uint64_t *n_nodes, uint64_t *nnz) {
    if (!h || layer >= h->host->nb_layers()) return HNSW_ERR_ARG;
    const std::vector<hx::NodeID> &ids = h->host->layer_nodes[layer];
    uint64_t total = 0;
    for (hx::NodeID id : ids) total += h->host->row(layer, id).size();
    if (n_nodes) *n_nodes = ids.size();
    if (nnz) *nnz = total;
    if (!node_ids || !offsets || !nbrs) return HNSW_OK;
    uint64_t off = 0;
    for (uint64_t i = 0; i < ids.size(); i++) {
        node_ids[i] = ids[i];
        offsets[i] = off;
        const std::vector<hx::NodeID> &r = h->host->row(layer, ids[i]);
        std::copy(r.begin(), r.end(), nbrs + off);
        std::sort(nbrs + off, nbrs + off + r.size());
        off += r.size();
    }
    offsets[ids.size()] = off;
    return HNSW_OK;
}

int hnsw_check_param_compliance(const hnsw_index *h, int *ok) {
    if (!h || !ok) return HNSW_ERR_ARG;
    *ok = h->host->check_param_compliance() ? 1 : 0;
    return HNSW_OK;
}

// ---- deletion ---------------------------------------------------------------------------------------------
static int set_deleted(hnsw_index *h, const uint32_t *ids, uint64_t k, bool on) {
    if (!h || (k && !ids)) return HNSW_ERR_ARG;
    const uint64_t len = index_len(h);
    for (uint64_t i = 0; i < k; i++)  // every id checked before anything changes
        if (ids[i] >= len) {
            set_error("id %u is not a point of the index (len %llu)", ids[i], (unsigned long long)len);
            return HNSW_ERR_ARG;
        }
    std::lock_guard<std::mutex> g(h->mu);
    h->del.set(ids, k, on, len);
    return HNSW_OK;
}
int hnsw_mark_deleted(hnsw_index *h, const uint32_t *ids, uint64_t k) { return set_deleted(h, ids, k, true); }
int hnsw_unmark_deleted(hnsw_index *h, const uint32_t *ids, uint64_t k) { return set_deleted(h, ids, k, false); }
int hnsw_is_deleted(const hnsw_index *h, uint32_t id, int *out) {
    if (!h || !out) return HNSW_ERR_ARG;
    if (id >= index_len(h)) {
        set_error("id %u is not a point of the index", id);
        return HNSW_ERR_ARG;
    }
    *out = h->del.test(id) ? 1 : 0;
    return HNSW_OK;
}
uint64_t hnsw_deleted_count(const hnsw_index *h) { return h ? h->del.count : 0; }
int hnsw_get_deleted(const hnsw_index *h, uint32_t *ids, uint64_t cap, uint64_t *n) {
    if (!h) return HNSW_ERR_ARG;
    if (n) *n = h->del.count;
    if (ids && cap) {
        uint64_t j = 0;
        for (uint64_t w = 0; w < h->del.words.size() && j < cap; w++)
            for (uint64_t x = h->del.words[w]; x && j < cap; x &= x - 1) ids[j++] = (uint32_t)(w * 64 + __builtin_ctzll(x));
    }
    return HNSW_OK;
}

// ---- labels -------------------------------------------------------------------------------------------------
int hnsw_set_labels(hnsw_index *h, const uint32_t *ids, const uint32_t *labels, uint64_t k) {
    if (!h || (k && !labels)) return HNSW_ERR_ARG;
    const uint64_t len = index_len(h);
    if (!ids && k > len) {
        set_error("%llu labels for the ids 0..k-1 of an index of %llu points", (unsigned long long)k, (unsigned long long)len);
        return HNSW_ERR_ARG;
    }
    for (uint64_t i = 0; ids && i < k; i++)  // every id checked before anything changes
        if (ids[i] >= len) {
            set_error("id %u is not a point of the index (len %llu)", ids[i], (unsigned long long)len);
            return HNSW_ERR_ARG;
        }
    std::lock_guard<std::mutex> g(h->mu);
    std::lock_guard<std::mutex> lg(h->lab.mu);
    h->lab.set(ids, labels, k, len);
    return HNSW_OK;
}
int hnsw_get_labels(const hnsw_index *h, const uint32_t *ids, uint64_t k, uint32_t *out) {
    if (!h || (k && !out)) return HNSW_ERR_ARG;
    const uint64_t len = index_len(h);
    if (!ids && k > len) {
        set_error("%llu labels asked of an index of %llu points", (unsigned long long)k, (unsigned long long)len);
        return HNSW_ERR_ARG;
    }
    for (uint64_t i = 0; ids && i < k; i++)
        if (ids[i] >= len) {
            set_error("id %u is not a point of the index (len %llu)", ids[i], (unsigned long long)len);
            return HNSW_ERR_ARG;
        }
    std::lock_guard<std::mutex> lg(h->lab.mu);  // (a range search may be growing the mirror to the index length)
    for (uint64_t i = 0; i < k; i++) out[i] = h->lab.get(ids ? ids[i] : i);
    return HNSW_OK;
}

// ---- persistence -----------------------------------------------------------------------------------
int hnsw_save(const hnsw_index *h, const char *dir) {
    if (!h || !dir) return HNSW_ERR_ARG;
    if (is_replica(h)) return reject_replica(h, "hnsw_save");
    if (h->incomplete_build) {  // an index whose on-device build stopped half way must not be written as if it were whole
        set_error("an on-device build on this handle failed half way; the index is incomplete, not saved");
        return HNSW_ERR_ARG;
    }
    int rc = hx::save_index(*h->host, dir);
    if (rc != HNSW_OK) return rc;
    if ((rc = hx::save_deleted(dir, h->del.ids()))) return rc;
    return hx::save_labels(dir, h->lab.labels);
}
int hnsw_load(const char *dir, hnsw_index **out) {
    if (!dir || !out) return HNSW_ERR_ARG;
    std::unique_ptr<hx::HostIndex> idx;
    int rc = hx::load_index(dir, &idx);
    if (rc != HNSW_OK) return rc;
    std::vector<uint64_t> deleted;
    if ((rc = hx::load_deleted(dir, idx->len(), &deleted))) return rc;
    std::vector<uint32_t> labels;
    if ((rc = hx::load_labels(dir, idx->len(), &labels))) return rc;
    hnsw_index *h = new (std::nothrow) hnsw_index();
    if (!h) return HNSW_ERR_OOM;
    h->host = std::move(idx);
    h->del.assign_host(deleted);
    h->lab.assign_host(labels);
    *out = h;
    return HNSW_OK;
}

// ---- device management -------------------------------------------------------------------------------
int hnsw_device_count(int *count) {
    if (!count) return HNSW_ERR_ARG;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return HNSW_OK;
}
int hnsw_set_device(hnsw_index *h, int device) {
    if (!h) return HNSW_ERR_ARG;
    std::lock_guard<std::mutex> g(h->mu);
    if (is_replica(h) && device != h->device) return reject_replica(h, "hnsw_set_device (a replica stays on the device it was received on)");
    if (device != h->device) {
        h->dev.release();
        h->del.release_device();  // (the host set stays; the next search copies it to the new device)
        h->lab.release_device();  // (and so the label column)
        // a leaderless batch the coalescer keeps open was made ready for the old device (stream, device arena): retire
        // it; the next caller opens one on the new device (no search may be in flight during this call)
        hx::Coalescer &co = h->co;
        std::lock_guard<hx::SpinLock> cg(co.mu);
        co.retire_unjoined();
        co.fast.store(nullptr, std::memory_order_release);
    }
    h->device = device;
    return HNSW_OK;
}
int hnsw_upload(hnsw_index *h) {
    if (!h) return HNSW_ERR_ARG;
    return ensure_uploaded(h);
}
int hnsw_set_option(hnsw_index *h, const char *key, int64_t value) { return h && key ? hx::set_option(h, key, value) : HNSW_ERR_ARG; }
int hnsw_device_bytes(const hnsw_index *h, uint64_t *bytes) {
    if (!h || !bytes) return HNSW_ERR_ARG;
    *bytes = h->dev.valid ? h->dev.bytes : 0;
    return HNSW_OK;
}
int hnsw_get_stat(const hnsw_index *h, const char *key, uint64_t *out) { return h && key && out ? hx::get_stat(h, key, out) : HNSW_ERR_ARG; }

// ---- snapshot replication ------------------------------------------------------------------------------
int hnsw_snapshot_describe(hnsw_index *h, hnsw_snapshot_desc *out) {
    if (!h || !out) return HNSW_ERR_ARG;
    const int rc = check_search_args(h, 1);
    return rc != HNSW_OK ? rc : hx::snapshot_describe(h, out);
}
int hnsw_snapshot_adopt(hnsw_index *h, hnsw_snapshot_desc *d) { return h && d ? hx::snapshot_adopt(h, d) : HNSW_ERR_ARG; }
int hnsw_snapshot_commit(hnsw_index *h) { return h ? hx::snapshot_commit(h) : HNSW_ERR_ARG; }

// ---- harness helpers -----------------------------------------------------------------------------------
int hnsw_synth_rows(int recipe, uint64_t seed, uint64_t first_row, uint64_t n, uint32_t d, float *out,
                    uint32_t nb_threads) {
    if (!out) return HNSW_ERR_ARG;
    return hx::synth_rows(recipe, seed, first_row, n, d, out, nb_threads);
}
int hnsw_draw_levels(uint32_t m, uint64_t n, uint8_t *out) {
    if (!out || m < 2) return HNSW_ERR_ARG;
    hx::stdrng_levels(0, hx::default_ml(m), n, out);
    return HNSW_OK;
}

}  // extern "C"
