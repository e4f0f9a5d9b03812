// handle.h -- the handle behind include/hnsw_mi355x.h's hnsw_index and what every host file asks of it (internal)
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "coalesce.h"
#include "deleted.h"
#include "device_build.h"
#include "device_index.h"
#include "hip_util.h"
#include "host_index.h"
#include "labels.h"
#include "scratch.h"

struct hnsw_index {
    std::unique_ptr<hx::HostIndex> host;
    hx::DeviceIndex dev;
    int device = -1;
    int gpu_build = 0;  // option "gpu_build": insert_bulk runs the on-device build (1 host connect, 2 device connect)
    // The on-device build inserts its points in batches of min(build_batch_max, max(64, connected /
    // build_batch_div)): the points of a batch do not see one another.  The defaults
    // build 1M points in 0.7 s; smaller batches stand closer to the reference's one-at-a-time insertion
    // (options "gpu_build_batch_max", "gpu_build_batch_div": 256 and 64 take 4 s per 1M points and lift
    // recall@10 at efSearch 64 from 0.9894 to 0.9901 on the bench's index).
    uint32_t build_batch_max = 8192, build_batch_div = 8;
    // set when an on-device build stopped half way (HIP error, failed exchange): the new points are stored
    // but not all of them are connected, so every later search or build on this handle fails loudly
    // instead of answering from an incomplete graph
    bool incomplete_build = false;
    // option "metric_cosine" (an extension, the reference is Euclidean only): rows are normalised to unit
    // length as they are inserted and queries as they arrive, so the L2 order behind is the cosine order
    bool cosine = false;
    std::mutex mu;
    std::mutex pool_mu;
    std::vector<std::unique_ptr<hx::SearchScratch>> pool;
    hx::Coalescer co;
    // counters behind hnsw_get_stat
    std::atomic<uint64_t> n_uploads{0}, n_point_patches{0}, n_patch_fallbacks{0};
    // filtered search (hnsw_search_batch_filtered): a call whose allow-list holds at most filter_exact_max ids is
    // answered by the exact scan ("Filtered search", for the measured crossover); queries per path
    int64_t filter_exact_max = 65536;
    // option "filter_exact_grouped": the batch entry points run a call's exact-path groups in the grouped form (three
    // launches for all of them, filter_exact.cpp) instead of group by group; hnsw_search_filtered always does
    int filter_exact_grouped = 0;
    std::atomic<uint64_t> n_filt_graph{0}, n_filt_exact{0}, n_filt_overflow{0};
    // hnsw_search_batch_filtered_multi: calls, and the masks their queries referenced (no mask counts as one)
    std::atomic<uint64_t> n_filt_multi_calls{0}, n_filt_multi_masks{0};
    // deleted ids (hnsw_mark_deleted), on the host and in HBM; while any is deleted the unfiltered entry points answer
    // by the filtered search over the undeleted ids and count their queries per path here
    hx::DeletedSet del;
    std::atomic<uint64_t> n_del_graph{0}, n_del_exact{0}, n_del_overflow{0};
    // resident mask sets (hnsw_mask_set, mask_set.h) of this handle, summed: words of any set copied to HBM, rows whose
    // admissible ids the host counted, compactions launched for rows of a set, searches under a set; the budget of a
    // set's compacted lists in HBM (option "mask_set_cache_mb")
    std::atomic<uint64_t> n_set_words_uploaded{0}, n_set_recounts{0}, n_set_compactions{0}, n_filt_set_calls{0};
    int64_t mask_set_cache_mb = 64;
    // the label column (hnsw_set_labels, labels.h), on the host and in HBM, and hnsw_search_batch_filtered_range's
    // calls (host calls and completed device calls) and the distinct ranges they named
    hx::LabelColumn lab;
    std::atomic<uint64_t> n_filt_range_calls{0}, n_filt_range_ranges{0};
    // ... and hnsw_search_batch_filtered_set_range's: calls, and the distinct (row, lo, hi) triples they named
    std::atomic<uint64_t> n_filt_set_range_calls{0}, n_filt_set_range_groups{0};
    // hnsw_search_batch_filtered_ranges: calls, and the distinct canonical range lists they named
    std::atomic<uint64_t> n_filt_ranges_calls{0}, n_filt_ranges_groups{0};
    // hnsw_search_filtered: calls answered, and the launches of their leaders (coalesce.h)
    std::atomic<uint64_t> n_filt_one_calls{0}, n_filt_one_batches{0};
    // hnsw_search_batch_shards with this handle as shard 0: calls whose shards were all searched, and their merges launched
    std::atomic<uint64_t> n_shard_calls{0}, n_shard_merges{0};
    // grouped search: hnsw_search_batch_grouped calls answered, and the collapses launched (hnsw_group_by_label_device's too)
    std::atomic<uint64_t> n_grouped_calls{0}, n_grouped_launches{0};
    // radius search: hnsw_search_batch_radius calls answered, the search rungs they launched, and their cuts launched
    std::atomic<uint64_t> n_radius_calls{0}, n_radius_rungs{0}, n_radius_launches{0};
    // diversified search: hnsw_search_batch_diverse calls answered, and the selections launched (hnsw_diversify_device's too)
    std::atomic<uint64_t> n_diverse_calls{0}, n_diverse_launches{0};
    // search from stored rows: hnsw_search_batch_from_rows / _by_id calls answered, the compose launches (those of
    // hnsw_compose_rows_device too) and the drop launches of those calls (hnsw_drop_ids_device takes no handle)
    std::atomic<uint64_t> n_from_rows_calls{0}, n_from_rows_compose{0}, n_from_rows_drop{0};
    // multi-vector search: hnsw_search_batch_multi calls answered, and the fusions launched (hnsw_fuse_lists_device's too)
    std::atomic<uint64_t> n_multi_calls{0}, n_multi_fuse{0};
    // late-interaction search: hnsw_search_batch_late calls answered, and the late interactions launched
    // (hnsw_late_interaction_device's too)
    std::atomic<uint64_t> n_late_calls{0}, n_late_launches{0};
    // exact document scoring: hnsw_search_batch_late_exact calls answered, and the scorings launched
    // (hnsw_score_documents_device's too)
    std::atomic<uint64_t> n_docs_calls{0}, n_docs_launches{0};
    // refined search: hnsw_search_batch_refined calls answered and the refinements they launched (hnsw_refine_device takes
    // no handle), and the writes that reached a row table of this handle
    std::atomic<uint64_t> n_refine_calls{0}, n_refine_launches{0}, n_row_table_writes{0};
    // hybrid search: hnsw_search_batch_hybrid calls answered, and the rank fusions launched (hnsw_fuse_ranked_device's too)
    std::atomic<uint64_t> n_hybrid_calls{0}, n_hybrid_fuse{0};
    // boosted search: hnsw_search_batch_boosted calls answered and the boosts they launched (hnsw_boost_device takes no
    // handle: its launches are counted for the process, boost.cpp, and "boost_launches" reads the sum)
    std::atomic<uint64_t> n_boost_calls{0}, n_boost_launches{0};
    hx::BuildStats build;  // the on-device builds of this handle, summed (hnsw_get_stat "build_*")
};

namespace hx {

// the launches of hnsw_boost_device, which takes no handle, in this process (boost.cpp)
uint64_t boost_device_launches();

// a device-only replica (hnsw_snapshot_adopt / _commit) has no host index behind its snapshot
inline bool is_replica(const hnsw_index *h) { return h->dev.replica; }
inline uint64_t index_len(const hnsw_index *h) { return is_replica(h) ? h->dev.view.n_points : h->host->len(); }
int reject_replica(const hnsw_index *h, const char *what);
// what every search entry point checks first: a handle, a complete build, a non-empty index, ef <= 2^26
int check_search_args(const hnsw_index *h, uint32_t ef);
// the HBM snapshot is what the host index holds (uploaded if not) and its device is the calling thread's
int ensure_uploaded(hnsw_index *h);

// options.cpp: one table of the options, one of the statistics; a clone takes every option as its parent stores it
int set_option(hnsw_index *h, const char *key, int64_t value);
void copy_options(hnsw_index *to, const hnsw_index *from);
int get_stat(const hnsw_index *h, const char *key, uint64_t *out);
// snapshot.cpp: hnsw_snapshot_describe (of a handle that passed check_search_args), _adopt and _commit
int snapshot_describe(hnsw_index *h, hnsw_snapshot_desc *out);
int snapshot_adopt(hnsw_index *h, hnsw_snapshot_desc *d);
int snapshot_commit(hnsw_index *h);

struct ScratchLease {  // takes a scratch from the handle's pool, gives it back at scope exit
    hnsw_index *h;
    std::unique_ptr<SearchScratch> s;
    explicit ScratchLease(hnsw_index *hh) : h(hh) {
        std::lock_guard<std::mutex> g(h->pool_mu);
        if (!h->pool.empty()) {
            s = std::move(h->pool.back());
            h->pool.pop_back();
        }
    }
    ~ScratchLease() {
        if (!s) return;
        std::lock_guard<std::mutex> g(h->pool_mu);
        if (h->pool.size() < 16) h->pool.push_back(std::move(s));
    }
    int prepare(int device, size_t dev_bytes, size_t pin_bytes) {
        if (!s) s.reset(new SearchScratch());
        return s->reserve(device, dev_bytes, pin_bytes, true);
    }
};

// the cosine option for queries already copied to the device (cosine_rows, capi.cpp, is the host form)
inline int cosine_queries(const hnsw_index *h, void *d_Q, uint64_t nq, hipStream_t stream) {
    if (!h->cosine) return HNSW_OK;
    return launch_normalise_rows(static_cast<float *>(d_Q), nq, h->dev.view.dim, stream);
}

// a stream-ordered temporary in HBM, freed in stream order at scope exit
struct StreamTmp {
    void *p = nullptr;
    hipStream_t st = nullptr;
    int alloc(size_t bytes, hipStream_t stream) {
        st = stream;
        HIP_TRY(hipMallocAsync(&p, bytes, stream));
        return HNSW_OK;
    }
    ~StreamTmp() {
        if (p) (void)hipFreeAsync(p, st);
    }
};

// ... and for queries the caller keeps in HBM (const to us): a stream-ordered unit-length copy
struct DeviceQueries {
    const float *q = nullptr;
    StreamTmp tmp;
    int prepare(const hnsw_index *h, const float *d_Q, uint64_t nq, hipStream_t stream) {
        q = d_Q;
        if (!h->cosine) return HNSW_OK;
        const size_t bytes = (size_t)nq * h->dev.view.dim * 4;
        if (int rc = tmp.alloc(bytes, stream)) return rc;
        HIP_TRY(hipMemcpyAsync(tmp.p, d_Q, bytes, hipMemcpyDeviceToDevice, stream));
        q = static_cast<const float *>(tmp.p);
        return launch_normalise_rows(static_cast<float *>(tmp.p), nq, h->dev.view.dim, stream);
    }
};

}  // namespace hx
