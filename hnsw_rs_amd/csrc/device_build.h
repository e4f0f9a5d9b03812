// device_build.h -- the on-device builds of device_build.cpp, behind capi.cpp's hnsw_insert_bulk* (internal)
#pragma once

#include <algorithm>
#include <cstdint>

#include "device_index.h"
#include "host_index.h"

namespace hx {

// the on-device builds of one handle, summed (hnsw_get_stat "build_*"): what the insert kernel read -- the build's
// algorithmic bytes -- and how long it and the connect phases ran
struct BuildStats {
    uint64_t points = 0, batches = 0, rows_read = 0, adj_rows = 0, adj_ids = 0, records = 0, removals = 0;
    uint64_t rows_owned = 0, rows_received = 0, exchange_bytes = 0;  // sharded build, phases 2 / 3 by row ownership
    // the device-connect build's paths: points that took the CPU path after it, points whose insertion search ran again
    // with a larger visited table, edges kept because they were a row's last one (phase 3 refusals + seed clamp restores)
    uint64_t cpu_path_points = 0, rerun_points = 0, kept_last_edges = 0;
    double insert_kernel_s = 0, insert_phase_s = 0, connect_s = 0, exchange_s = 0, connect_kernel_s = 0;
};

// options "gpu_build_batch_max" / "_div" (the points of one batch do not see one another): the next batch is at most
// what is left, `bmax` (what the build's buffers hold), `max`, and 1 / `div` of the points connected (but 64 at least)
struct BatchSchedule {
    uint32_t max, div;
    size_t next(size_t rest, uint64_t connected, uint32_t bmax) const {
        return std::min<size_t>(rest, std::min<uint64_t>(std::min<uint64_t>(bmax, max), std::max<uint64_t>(64, connected / div)));
    }
};

struct BuildTarget {  // what a build reads and changes besides the points it inserts (a handle's parts)
    HostIndex &host;
    DeviceIndex &dev;  // uploaded again by the build
    int &device;       // set to the device the snapshot went to
    BatchSchedule batches;
    BuildStats &stats;  // the device-connect build adds to it
};

struct ShardCtx {  // hnsw_insert_bulk_sharded: this rank, the world, the caller's exchange slots and all-gather
    uint32_t rank, world;
    unsigned char *d_send, *d_recv;  // one slot / world slots of slot_bytes
    uint64_t slot_bytes;
    hnsw_allgather_fn allgather;
    void *ctx;
};
uint64_t shard_slot_bytes(uint32_t m, uint32_t world);  // one rank's exchange slot (hnsw_sharded_slot_bytes)

// "gpu_build" = 1: insertion searches on the device, connect on the host
int gpu_insert_bulk(const BuildTarget &t, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                    const uint8_t *levels);
// "gpu_build" = 2 (and hnsw_insert_bulk_device, _sharded with `sh`): connect on the device as well
int gpu_insert_bulk_full(const BuildTarget &t, const float *rows, uint64_t n, uint32_t nb_threads, int verbose,
                         const uint8_t *levels, const ShardCtx *sh = nullptr);

}  // namespace hx
