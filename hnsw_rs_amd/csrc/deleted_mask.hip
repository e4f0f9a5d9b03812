// deleted_mask.hip -- the deleted set of a handle (deleted.h): host bookkeeping and the update of an HBM copy of
// host words (HbmWords: the deleted set's, and the resident mask sets'), with its one kernel,
// hx_deleted_scatter_kernel (gfx950).

#include <algorithm>
#include <cstring>

#include "deleted.h"
#include "hip_util.h"
#include "launch.h"

namespace hx {

namespace {

// pairs[2 i] = word index, pairs[2 i + 1] = its value: one thread per changed word, plain vector stores
__global__ void __launch_bounds__(256) hx_deleted_scatter_kernel(uint64_t *mask, const uint64_t *pairs, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[pairs[2 * i]] = pairs[2 * i + 1];
}

}  // namespace

void DeletedSet::set(const uint32_t *ids, uint64_t k, bool on, uint64_t n_points) {
    const uint64_t nw = (n_points + 63) / 64;
    if (words.size() < nw) {
        words.resize(nw, 0);
        dirty_flag.resize(nw, 0);
    }
    for (uint64_t i = 0; i < k; i++) {
        const uint32_t id = ids[i];
        uint64_t &w = words[id >> 6];
        const uint64_t bit = 1ull << (id & 63);
        if (((w & bit) != 0) == on) continue;  // idempotent: an unchanged word is not listed
        w ^= bit;
        count = on ? count + 1 : count - 1;
        version++;
        touch(id >> 6);
    }
}

std::vector<uint32_t> DeletedSet::ids() const {
    std::vector<uint32_t> out;
    out.reserve(count);
    for (uint64_t w = 0; w < words.size(); w++)
        for (uint64_t x = words[w]; x; x &= x - 1) out.push_back((uint32_t)(w * 64 + __builtin_ctzll(x)));
    return out;
}

void DeletedSet::assign_host(const std::vector<uint64_t> &w) {
    release_device();
    words = w;
    count = 0;
    version++;
    for (uint64_t x : words) count += (uint64_t)__builtin_popcountll(x);
    dirty.clear();
    dirty_flag.assign(words.size(), 0);
}

void HbmWords::release_device() {
    if (d_words) (void)hipFree(d_words);
    if (d_stage) (void)hipFree(d_stage);
    d_words = d_stage = nullptr;
    d_cap = d_stage_cap = 0;
    d_device = -1;
}

int HbmWords::sync_words(const uint64_t *words, uint64_t nw, uint64_t slack, int device, hipStream_t stream) {
    if (d_words && (d_device != device || d_cap < nw)) release_device();
    // a whole copy when there is no HBM copy yet, or when more than an eighth of the words changed (a pair is
    // twice a word's bytes, and the scatter is one more launch)
    const bool whole = !d_words || dirty.size() * 8 > nw;
    if (!d_words) {
        const uint64_t cap = std::max<uint64_t>(1, nw + slack);
        HIP_TRY(hipMalloc(&d_words, cap * 8));
        d_cap = cap;
        d_device = device;
        HIP_TRY(hipMemsetAsync(d_words, 0, cap * 8, stream));
    } else if (dirty.empty()) {
        return HNSW_OK;
    }
    if (whole) {
        if (nw) HIP_TRY(hipMemcpyAsync(d_words, words, nw * 8, hipMemcpyHostToDevice, stream));
        words_uploaded += nw;
    } else {
        const uint64_t np = dirty.size();
        if (d_stage_cap < np) {
            if (d_stage) (void)hipFree(d_stage);
            d_stage = nullptr;
            d_stage_cap = 0;
            const uint64_t cap = np + np / 2 + 64;
            HIP_TRY(hipMalloc(&d_stage, cap * 16));
            d_stage_cap = cap;
        }
        std::vector<uint64_t> pairs(2 * np);
        for (uint64_t i = 0; i < np; i++) {
            pairs[2 * i] = dirty[i];
            pairs[2 * i + 1] = words[dirty[i]];
        }
        HIP_TRY(hipMemcpyAsync(d_stage, pairs.data(), np * 16, hipMemcpyHostToDevice, stream));
        if (int rc = launch_checked({"hipGetLastError() failed"}, hx_deleted_scatter_kernel, dim3((uint32_t)((np + 255) / 256)),
                                    dim3(256), 0, stream, d_words, (const uint64_t *)d_stage, np))
            return rc;
        words_uploaded += np;
    }
    // (`pairs` and `words` are read by the copies, and searches on other streams read the mask next)
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t w : dirty) dirty_flag[w] = 0;
    dirty.clear();
    return HNSW_OK;
}

}  // namespace hx
