// mask_set.cpp -- hnsw_mask_set (mask_set.h): the C entry points that manage a set on the host, and what a search
// asks of it: the HBM copy brought up to date, a row's admissible ids counted once, room for its compacted list.
// Host logic only; the searches under a set are filter_host.cpp's, the counting of a row next to a range filter_plan.cpp's.

#include "mask_set.h"

#include <algorithm>
#include <cstring>
#include <new>

#include "handle.h"
#include "search_host.h"

using hx::set_error;

int hnsw_mask_set::sync(hnsw_index *h) {
    const int device = h->dev.device;
    if (hbm.current(device)) return HNSW_OK;
    if (hbm.d_device != device) drop_lists();  // (they live on the device of the copy)
    hx::ScratchLease lease(h);
    int rc = lease.prepare(device, 0, 0);
    if (rc != HNSW_OK) return rc;
    const uint64_t before = hbm.words_uploaded;
    rc = hbm.sync_words(words.data(), words.size(), 0, device, lease.s->stream);
    h->n_set_words_uploaded.fetch_add(hbm.words_uploaded - before, std::memory_order_relaxed);
    return rc;
}

hnsw_mask_set::Row &hnsw_mask_set::counted(hnsw_index *h, uint32_t row) {
    Row &r = rows[row];
    const uint64_t len = hx::index_len(h);
    if (r.c_version != r.version || r.c_del != h->del.version || r.c_len != len) {
        r.A = hx::count_admissible(h, row_words(row), std::min<uint64_t>(allow_bits, len), r.wbase);
        r.c_version = r.version;
        r.c_del = h->del.version;
        r.c_len = len;
        r.list_valid = false;
        h->n_set_recounts.fetch_add(1, std::memory_order_relaxed);
    }
    return r;
}

bool hnsw_mask_set::reserve_list(Row &r, uint64_t budget_bytes) {
    if (r.d_ids && r.d_cap >= r.A) return true;
    const uint64_t cap = std::max<uint64_t>(1, r.A);
    if (list_bytes - r.d_cap * 4 + cap * 4 > budget_bytes) return false;
    if (r.d_ids) (void)hipFree(r.d_ids);
    list_bytes -= r.d_cap * 4;
    r.d_ids = nullptr;
    r.d_cap = 0;
    if (hipMalloc(&r.d_ids, cap * 4) != hipSuccess) {  // no room in HBM: this call compacts in its scratch
        (void)hipGetLastError();
        r.d_ids = nullptr;
        return false;
    }
    r.d_cap = cap;
    list_bytes += cap * 4;
    return true;
}

void hnsw_mask_set::drop_lists() {
    for (Row &r : rows) {
        if (r.d_ids) (void)hipFree(r.d_ids);
        r.d_ids = nullptr;
        r.d_cap = 0;
        r.list_valid = false;
    }
    list_bytes = 0;
}

namespace {

int check_row(const hnsw_mask_set *s, uint32_t row, const void *buf) {
    if (!s || (!buf && s->W)) {
        set_error("mask set: needs a set and a buffer of its row's words");
        return HNSW_ERR_ARG;
    }
    if (row >= s->n_masks) {
        set_error("mask set: row %u of %u", row, s->n_masks);
        return HNSW_ERR_ARG;
    }
    return HNSW_OK;
}

// words[W] into a row: bits of the last word beyond allow_bits are dropped, only changed words are listed
bool store_row(hnsw_mask_set *s, uint32_t row, const uint64_t *words) {
    uint64_t *dst = s->row_words(row);
    bool changed = false;
    for (uint64_t w = 0; w < s->W; w++) {
        uint64_t x = words[w];
        if (w == s->W - 1 && s->allow_bits % 64) x &= (1ull << (s->allow_bits % 64)) - 1;
        if (dst[w] == x) continue;
        dst[w] = x;
        s->hbm.touch((uint64_t)row * s->W + w);
        changed = true;
    }
    return changed;
}

}  // namespace

extern "C" {

int hnsw_mask_set_create(hnsw_index *h, uint32_t n_masks, uint64_t allow_bits, const uint64_t *masks,
                         hnsw_mask_set **out) {
    if (!h || !out) {
        set_error("mask set: needs a handle and a place for the set");
        return HNSW_ERR_ARG;
    }
    const uint64_t W = (allow_bits + 63) / 64;
    if (allow_bits > (1ull << 32) || (W && (uint64_t)n_masks > 0xFFFFFFFFull / W)) {  // (a changed word is listed as u32)
        set_error("mask set: %u masks of %llu bits are more than 2^32 - 1 words", n_masks, (unsigned long long)allow_bits);
        return HNSW_ERR_ARG;
    }
    hnsw_mask_set *s = new (std::nothrow) hnsw_mask_set();
    if (!s) return HNSW_ERR_OOM;
    try {
        s->words.assign((uint64_t)n_masks * W, 0);
        s->hbm.dirty_flag.assign((uint64_t)n_masks * W, 0);
        s->rows.resize(n_masks);
    } catch (const std::bad_alloc &) {
        delete s;
        set_error("mask set: out of memory for %u masks of %llu bits", n_masks, (unsigned long long)allow_bits);
        return HNSW_ERR_OOM;
    }
    s->owner = h;
    s->n_masks = n_masks;
    s->allow_bits = allow_bits;
    s->W = W;
    if (masks)
        for (uint32_t g = 0; g < n_masks; g++) store_row(s, g, masks + (uint64_t)g * W);
    // (no HBM copy yet: the first search makes one whole copy, whatever is listed)
    *out = s;
    return HNSW_OK;
}

void hnsw_mask_set_free(hnsw_mask_set *s) { delete s; }

int hnsw_mask_set_info(const hnsw_mask_set *s, uint32_t *n_masks, uint64_t *allow_bits) {
    if (!s) return HNSW_ERR_ARG;
    if (n_masks) *n_masks = s->n_masks;
    if (allow_bits) *allow_bits = s->allow_bits;
    return HNSW_OK;
}

int hnsw_mask_set_write(hnsw_mask_set *s, uint32_t row, const uint64_t *words) {
    int rc = check_row(s, row, words);
    if (rc != HNSW_OK) return rc;
    std::lock_guard<std::mutex> g(s->mu);
    if (store_row(s, row, words)) s->row_changed(row);
    return HNSW_OK;
}

int hnsw_mask_set_update(hnsw_mask_set *s, uint32_t row, const uint32_t *ids, uint64_t k, int allow) {
    if (!s || (k && !ids)) {
        set_error("mask set: needs a set and the ids to update");
        return HNSW_ERR_ARG;
    }
    if (row >= s->n_masks) {
        set_error("mask set: row %u of %u", row, s->n_masks);
        return HNSW_ERR_ARG;
    }
    for (uint64_t i = 0; i < k; i++)  // every id checked before anything changes
        if (ids[i] >= s->allow_bits) {
            set_error("mask set: id %u is not below allow_bits (%llu)", ids[i], (unsigned long long)s->allow_bits);
            return HNSW_ERR_ARG;
        }
    std::lock_guard<std::mutex> g(s->mu);
    uint64_t *dst = s->row_words(row);
    bool changed = false;
    for (uint64_t i = 0; i < k; i++) {
        const uint64_t bit = 1ull << (ids[i] & 63);
        uint64_t &w = dst[ids[i] >> 6];
        if (((w & bit) != 0) == (allow != 0)) continue;  // idempotent: an unchanged word is not listed
        w ^= bit;
        s->hbm.touch((uint64_t)row * s->W + (ids[i] >> 6));
        changed = true;
    }
    if (changed) s->row_changed(row);
    return HNSW_OK;
}

int hnsw_mask_set_read(const hnsw_mask_set *s, uint32_t row, uint64_t *words) {
    int rc = check_row(s, row, words);
    if (rc != HNSW_OK) return rc;
    if (s->W) memcpy(words, s->row_words(row), s->W * 8);
    return HNSW_OK;
}

int hnsw_mask_set_count(const hnsw_mask_set *s, uint32_t row, uint64_t *allowed) {
    int rc = check_row(s, row, allowed);
    if (rc != HNSW_OK) return rc;
    if (!allowed) return HNSW_ERR_ARG;
    uint64_t c = 0;
    const uint64_t *src = s->row_words(row);
    for (uint64_t w = 0; w < s->W; w++) c += (uint64_t)__builtin_popcountll(src[w]);
    *allowed = c;
    return HNSW_OK;
}

}  // extern "C"
