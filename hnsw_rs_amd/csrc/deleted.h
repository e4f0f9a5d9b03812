// deleted.h -- the deleted set of a handle (hnsw_mark_deleted): a bitmask over ids on the host, its copy in HBM,
// and the sidecar file "deleted" of hnsw_save.  The search kernels read the HBM copy as FilterArgs::deny
// (search_filtered.h).
//
// Marking and unmarking touch the host words only and list the words they changed; the next search that needs
// the HBM copy brings it up to date (DeletedSet::sync): the changed words travel as (word index, value) pairs in
// one copy and are scattered by a small kernel (deleted_mask.hip), or, when many words changed or the copy does
// not exist yet, the whole mask is copied.  That mechanism is HbmWords, which the resident mask sets (mask_set.h)
// share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace hx {

// The HBM copy of an array of 64-bit words the host owns, and the list of words the host changed since the copy was
// last brought up to date.
struct HbmWords {
    // words changed since the HBM copy was last brought up to date, each listed once
    std::vector<uint32_t> dirty;
    std::vector<uint8_t> dirty_flag;  // one per host word (the owner sizes it)
    // the HBM copy: d_cap words on device d_device; d_stage holds the pairs of one scatter
    uint64_t *d_words = nullptr, *d_stage = nullptr;
    uint64_t d_cap = 0, d_stage_cap = 0;
    int d_device = -1;
    uint64_t words_uploaded = 0;  // words copied to HBM so far

    HbmWords() = default;
    HbmWords(const HbmWords &) = delete;
    HbmWords &operator=(const HbmWords &) = delete;
    ~HbmWords() { release_device(); }

    void touch(uint64_t w) {  // host word w changed
        if (!dirty_flag[w]) {
            dirty_flag[w] = 1;
            dirty.push_back((uint32_t)w);
        }
    }
    bool current(int device) const { return d_words && d_device == device && dirty.empty(); }
    // brings the HBM copy of host[nw] on `device` up to date: the changed words as (index, value) pairs scattered by
    // hx_deleted_scatter_kernel, or one whole copy when there is no copy yet (made with room for `slack` more words,
    // zeroed), the device changed, the host words have outgrown it (d_cap < nw: made afresh, whether or not a word is
    // listed) or more than an eighth of the words changed.  Synchronises `stream` before returning.
    int sync_words(const uint64_t *host, uint64_t nw, uint64_t slack, int device, hipStream_t stream);
    void release_device();
};

struct DeletedSet : HbmWords {
    std::vector<uint64_t> words;  // id i is deleted iff bit i & 63 of words[i >> 6] is set; covers every marked id
    uint64_t count = 0;           // ids deleted
    // advances whenever the set of deleted ids changes: what a cache over the admissible ids (mask_set.h) is valid for
    uint64_t version = 0;
    // (HbmWords::words_uploaded is hnsw_get_stat "deleted_mask_words_uploaded")

    bool test(uint64_t id) const { return (id >> 6) < words.size() && ((words[id >> 6] >> (id & 63)) & 1ull) != 0; }
    // marks (on) or unmarks k ids, all below n_points (checked by the caller); the mask grows to cover n_points
    void set(const uint32_t *ids, uint64_t k, bool on, uint64_t n_points);
    // the deleted ids, ascending
    std::vector<uint32_t> ids() const;
    // the host set of another handle (hnsw_clone) or of a file (hnsw_load); the HBM copy is made afresh
    void assign_host(const std::vector<uint64_t> &w);
    // ids the mask covers (FilterArgs::deny_bits): ids beyond it are not deleted
    uint64_t deny_bits() const { return (uint64_t)words.size() * 64; }
    // brings the HBM copy on `device` up to date; synchronises `stream` before returning
    int sync(int device, hipStream_t stream) {
        return sync_words(words.data(), words.size(), words.size() / 8 + 16, device, stream);  // room for later inserts
    }
};

// the sidecar file <dir>/deleted: u64 count, then that many u32 ids in strictly ascending order, big-endian.
// save writes it only for a non-empty set and removes a stale one otherwise; load leaves `words` empty when the
// file is absent and returns HNSW_ERR_IO for a damaged one (short, long, unsorted, an id >= n_points).
int save_deleted(const std::string &dir, const std::vector<uint32_t> &ids);
int load_deleted(const std::string &dir, uint64_t n_points, std::vector<uint64_t> *words);

}  // namespace hx
