// row_table.h -- hnsw_row_table (include/hnsw_mi355x.h, "refined search"): a table of full rows that lives with a
// handle, in HBM ONLY: rows x full_dim elements of f32 or IEEE binary16, row id = index id, what the refinement
// (hx_distance_kernel's sixth source form, exact_scan.hip) scores a candidate list against.  The host keeps no copy: the
// caller owns the full rows.  The table is not saved by hnsw_save, not cloned by hnsw_clone and not part of the snapshot
// exchange; hnsw_row_table_save / _load carry it in a file of its own.  With full_dim <= 32 it is the attribute table of
// boosted search (the kernel's ninth form).  Host logic only (row_table.cpp).
//
// Create touches no device; the first write allocates on the handle's device and fixes it.  A write past the capacity
// grows the array by a device-to-device copy (capacity + 1/8, as DeviceIndex::append_point grows its arrays).  Writes are
// serialised by `mu`; a write must not run while a search names the table.
#pragma once

#include <cstdint>
#include <mutex>

struct hnsw_index;

struct hnsw_row_table {
    hnsw_index *owner = nullptr;  // the handle that created it: no other may search with it
    uint32_t full_dim = 0, dtype = 0;
    int device = -1;        // where d_rows lives; -1: nothing allocated yet
    void *d_rows = nullptr;
    uint64_t rows = 0, cap = 0;  // rows written (ids 0 .. rows - 1, no holes), rows allocated
    std::mutex mu;

    hnsw_row_table() = default;
    hnsw_row_table(const hnsw_row_table &) = delete;
    hnsw_row_table &operator=(const hnsw_row_table &) = delete;
    ~hnsw_row_table();

    uint64_t row_bytes() const { return (uint64_t)full_dim * (dtype ? 2 : 4); }
};

namespace hx {

// IEEE binary16 <-> f32 on the host: round to nearest even, and the exact widening
uint16_t f16_from_f32(float f);
float f32_from_f16(uint16_t h);

}  // namespace hx
