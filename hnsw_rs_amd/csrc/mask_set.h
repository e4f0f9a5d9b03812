// mask_set.h -- hnsw_mask_set (include/hnsw_mi355x.h): allow-lists that live with a handle.  n_masks rows of
// W = ceil(allow_bits / 64) words on the host, their copy in HBM, and what a search would otherwise work out per call
// for every row it names: the row's admissible ids (count and word offsets) and, for a row on the exact path, the
// compacted id list in HBM.  Host logic only (mask_set.cpp); the HBM copy is HbmWords' (deleted.h), as the deleted
// set's.
//
// Create, write, update, read and count touch the host words only and list the words they changed; the next search
// that names the set brings the HBM copy up to date.  Everything a search does to the set (that update, the caches) is
// serialised by `mu`; write and update must not run while a search names the set.
#pragma once

#include <cstdint>
#include <mutex>
#include <vector>

#include "deleted.h"

struct hnsw_index;

struct hnsw_mask_set {
    hnsw_index *owner = nullptr;  // the handle that created it: no other may search under it
    uint32_t n_masks = 0;
    uint64_t allow_bits = 0, W = 0;
    std::vector<uint64_t> words;  // n_masks x W; bits of a row's last word beyond allow_bits are 0
    hx::HbmWords hbm;             // the HBM copy on the owner's snapshot device
    std::mutex mu;

    // What is cached of a row, valid while the row, the owner's deleted set and its length are those it was made for
    struct Row {
        uint64_t version = 1;                     // advances when the row's words change
        uint64_t c_version = 0, c_del = 0, c_len = 0;  // ... what the cache below was made for (c_version 0: nothing)
        uint64_t A = 0;                           // admissible ids
        std::vector<uint32_t> wbase;              // admissible ids before every block of 64 words
        uint32_t *d_ids = nullptr;                // the ascending admissible ids in HBM (hx_filt_compact_kernel's output)
        uint64_t d_cap = 0;                       // ids d_ids has room for
        bool list_valid = false;
    };
    std::vector<Row> rows;
    uint64_t list_bytes = 0;  // HBM the lists hold, bounded by the option "mask_set_cache_mb"

    hnsw_mask_set() = default;
    hnsw_mask_set(const hnsw_mask_set &) = delete;
    hnsw_mask_set &operator=(const hnsw_mask_set &) = delete;
    ~hnsw_mask_set() { drop_lists(); }

    uint64_t *row_words(uint32_t row) { return words.data() + (uint64_t)row * W; }
    const uint64_t *row_words(uint32_t row) const { return words.data() + (uint64_t)row * W; }
    void row_changed(uint32_t row) { rows[row].version++; }

    // ---- what a search asks (mu held) ----
    // the HBM copy on the owner's snapshot device, brought up to date on a stream of the handle's own (the lists go
    // when the device changed); counts "mask_set_words_uploaded"
    int sync(hnsw_index *h);
    // the row's cache entry with A and wbase valid (counted on the host when it is not: "mask_set_recounts")
    Row &counted(hnsw_index *h, uint32_t row);
    // room for the row's A ids in its list within the budget; false: the budget is used up (nothing is evicted)
    bool reserve_list(Row &r, uint64_t budget_bytes);
    void drop_lists();
    // the rows in HBM (nullptr for rows without words: allow_bits == 0)
    const uint64_t *d_rows() const { return W && n_masks ? hbm.d_words : nullptr; }
};
