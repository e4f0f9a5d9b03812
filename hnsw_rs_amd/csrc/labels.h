// labels.h -- the label column of a handle (hnsw_set_labels): one uint32 per id on the host, its copy in HBM, the
// sorted copy the range planner counts with, and the sidecar file "labels" of hnsw_save.  The filtered kernels read
// the HBM copy as FilterArgs::labels (search_filtered.h) and admit an id whose label lies in the query's range
// (hnsw_search_batch_filtered_range).
//
// Setting labels touches the host mirror only and lists the 64-bit words (two labels each) it changed; the next range
// search brings the HBM copy up to date by HbmWords (deleted.h): the changed words scattered, or one whole copy.  An
// id whose label was never set has label 0, on the host and in the kernels (an id at or beyond the copy's length
// reads as 0), so points inserted later need no call.
#pragma once

#include <cstdint>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "deleted.h"

namespace hx {

// The document index in HBM (docs.cpp): a copy of LabelColumn::sorted, 8 bytes per undeleted id, made whole whenever the
// (label version, deleted version, length) it was made for is no longer the sorted copy's.  Derived from the column and
// the deleted set: not saved, no part of the snapshot exchange.
struct DocIndex {
    uint64_t *d_keys = nullptr;
    uint64_t cap = 0, n = 0;  // keys allocated, keys held
    int device = -1;
    uint64_t version = ~0ull, del = 0, len = 0;  // what the copy was made for
    uint64_t uploads = 0, keys_uploaded = 0;     // hnsw_get_stat "doc_index_uploads", "doc_index_keys_uploaded"
    DocIndex() = default;
    DocIndex(const DocIndex &) = delete;
    DocIndex &operator=(const DocIndex &) = delete;
    ~DocIndex() { release(); }
    void release() {
        if (d_keys) (void)hipFree(d_keys);
        d_keys = nullptr;
        cap = n = 0;
        device = -1;
    }
};

struct LabelColumn : HbmWords {
    // label of id i is labels[i], 0 at and beyond labels.size(); the size is even: word w of the HBM copy is
    // labels[2 w] | labels[2 w + 1] << 32 (little-endian), so the device reads the copy as a plain uint32 array
    std::vector<uint32_t> labels;
    uint64_t version = 0;  // advances whenever a label changes: what `sorted` below is valid for
    // (HbmWords::words_uploaded is hnsw_get_stat "label_words_uploaded")

    uint32_t get(uint64_t id) const { return id < labels.size() ? labels[id] : 0u; }
    // labels[i] for ids[i] (nullptr: id i), all below n_points (checked by the caller); the mirror grows to cover
    // n_points; an unchanged label lists no word
    void set(const uint32_t *ids, const uint32_t *values, uint64_t k, uint64_t n_points);
    // grows the mirror to cover n_points ids (labels of 0: no label changes, no word is listed)
    void cover(uint64_t n_points);
    // the column of another handle (hnsw_clone) or of a file (hnsw_load); the HBM copy is made afresh
    void assign_host(const std::vector<uint32_t> &l);
    bool any_nonzero() const;
    uint64_t n_words() const { return labels.size() / 2; }
    // brings the HBM copy on `device` up to date; synchronises `stream` before returning
    int sync(int device, hipStream_t stream) {
        // (the mirror's buffer as words: little-endian, even length, and operator new aligns it for uint64_t)
        return sync_words(reinterpret_cast<const uint64_t *>(labels.data()), n_words(), n_words() / 8 + 16, device,
                          stream);  // room for later inserts
    }
    const uint32_t *d_labels() const { return reinterpret_cast<const uint32_t *>(d_words); }
    // both HBM copies go (hnsw_set_device, assign_host): each is made afresh on its first use
    void release_device() {
        HbmWords::release_device();
        doc.release();
    }

    // ---- the range planner's view (mu held): the keys label << 32 | id of the undeleted ids below len, ascending.
    // Made by one sort when the column, the deleted set or the length changed; then the admissible ids of a range are
    // a contiguous slice, found by two binary searches. ----
    mutable std::mutex mu;
    std::vector<uint64_t> sorted;
    uint64_t s_version = ~0ull, s_del = 0, s_len = 0;
    void sort_for(const DeletedSet &del, uint64_t len);
    DocIndex doc;  // the HBM copy of `sorted` (mu held)
    // admissible ids of [lo, hi] (sort_for first): the slice [first, first + A) of `sorted`
    uint64_t count(uint32_t lo, uint32_t hi, uint64_t *first = nullptr) const;
    // ... and how many of them lie before every block of 64 words (4096 ids): the compaction kernel's offsets
    void word_base(uint64_t first, uint64_t A, uint64_t len, std::vector<uint32_t> &wbase) const;
    // ... the same for the union of several disjoint ranges: the slices (first, A) of `sorted`, accumulated
    void word_base(const std::vector<std::pair<uint64_t, uint64_t>> &slices, uint64_t len, std::vector<uint32_t> &wbase) const;
    // the disjoint union of up to k closed ranges, ascending: empty members (lo > hi) dropped, the others sorted and
    // merged where they overlap or touch ([1, 2], [3, 4] -> [1, 4]; hi = UINT32_MAX touches nothing above it).  The
    // canonical form of a query's range list (hnsw_search_batch_filtered_ranges): members as (lo << 32) | hi
    static std::vector<uint64_t> canonical(const uint32_t *lo, const uint32_t *hi, uint32_t k);
};

// the sidecar file <dir>/labels: u64 count, then the labels of ids 0..count-1 as u32, big-endian (trailing zero labels
// dropped).  save writes it only when some label is nonzero and removes a stale one otherwise; load leaves `labels`
// empty when the file is absent and returns HNSW_ERR_IO for a damaged one (short, longer than its count, count >
// n_points).
int save_labels(const std::string &dir, const std::vector<uint32_t> &labels);
int load_labels(const std::string &dir, uint64_t n_points, std::vector<uint32_t> *labels);

}  // namespace hx
