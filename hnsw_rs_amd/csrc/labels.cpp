// labels.cpp -- the label column of a handle (labels.h): the host mirror and the sorted copy the range planner counts
// with.  Host logic only; the HBM copy is HbmWords' (deleted_mask.hip), the searches are filter_host.cpp's, their planner filter_plan.cpp.

#include "labels.h"

#include <algorithm>

namespace hx {

void LabelColumn::cover(uint64_t n_points) {
    const uint64_t nw = (n_points + 1) / 2;
    if (labels.size() < 2 * nw) {
        labels.resize(2 * nw, 0);
        dirty_flag.resize(nw, 0);
    }
}

void LabelColumn::set(const uint32_t *ids, const uint32_t *values, uint64_t k, uint64_t n_points) {
    cover(n_points);
    for (uint64_t i = 0; i < k; i++) {
        const uint64_t id = ids ? ids[i] : i;
        if (labels[id] == values[i]) continue;  // idempotent: an unchanged word is not listed
        labels[id] = values[i];
        version++;
        touch(id >> 1);
    }
}

void LabelColumn::assign_host(const std::vector<uint32_t> &l) {
    release_device();
    labels = l;
    if (labels.size() % 2) labels.push_back(0);
    version++;
    dirty.clear();
    dirty_flag.assign(labels.size() / 2, 0);
}

bool LabelColumn::any_nonzero() const {
    return std::any_of(labels.begin(), labels.end(), [](uint32_t x) { return x != 0; });
}

void LabelColumn::sort_for(const DeletedSet &del, uint64_t len) {
    if (s_version == version && s_del == del.version && s_len == len) return;
    sorted.clear();
    sorted.reserve(len - std::min(len, del.count));
    for (uint64_t id = 0; id < len; id++)
        if (!del.test(id)) sorted.push_back(((uint64_t)get(id) << 32) | id);
    std::sort(sorted.begin(), sorted.end());
    s_version = version;
    s_del = del.version;
    s_len = len;
}

uint64_t LabelColumn::count(uint32_t lo, uint32_t hi, uint64_t *first) const {
    if (first) *first = 0;
    if (lo > hi) return 0;  // an empty range
    const auto b = std::lower_bound(sorted.begin(), sorted.end(), (uint64_t)lo << 32);
    const auto e = std::upper_bound(b, sorted.end(), ((uint64_t)hi << 32) | 0xFFFFFFFFull);
    if (first) *first = (uint64_t)(b - sorted.begin());
    return (uint64_t)(e - b);
}

void LabelColumn::word_base(uint64_t first, uint64_t A, uint64_t len, std::vector<uint32_t> &wbase) const {
    word_base(std::vector<std::pair<uint64_t, uint64_t>>{{first, A}}, len, wbase);
}

void LabelColumn::word_base(const std::vector<std::pair<uint64_t, uint64_t>> &slices, uint64_t len,
                            std::vector<uint32_t> &wbase) const {
    const uint64_t n_words = (len + 63) / 64, n_wblk = (n_words + 63) / 64;
    wbase.assign(std::max<uint64_t>(1, n_wblk) + 1, 0);
    for (const auto &s : slices)
        for (uint64_t i = s.first; i < s.first + s.second; i++) wbase[((uint32_t)sorted[i] >> 12) + 1]++;  // ids per block, shifted by one
    for (size_t b = 1; b < wbase.size(); b++) wbase[b] += wbase[b - 1];
    wbase.pop_back();  // wbase[b] = admissible ids in the blocks before b
}

std::vector<uint64_t> LabelColumn::canonical(const uint32_t *lo, const uint32_t *hi, uint32_t k) {
    std::vector<uint64_t> in, out;
    for (uint32_t j = 0; j < k; j++)
        if (lo[j] <= hi[j]) in.push_back(((uint64_t)lo[j] << 32) | hi[j]);
    std::sort(in.begin(), in.end());  // ascending lo
    for (uint64_t m : in) {
        const uint64_t l = m >> 32, h = m & 0xFFFFFFFFull;
        // (64-bit: the end of the last member plus one does not wrap at UINT32_MAX)
        if (!out.empty() && l <= (out.back() & 0xFFFFFFFFull) + 1)
            out.back() = (out.back() & ~0xFFFFFFFFull) | std::max<uint64_t>(out.back() & 0xFFFFFFFFull, h);
        else
            out.push_back(m);
    }
    return out;
}

}  // namespace hx
