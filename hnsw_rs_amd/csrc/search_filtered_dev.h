// search_filtered_dev.h -- the device pieces that the families of filtered-search kernels share (search_filtered.hip,
// search_filtered_wide.hip, search_filtered16.hip): the key of an empty lane, the wave's smallest key, the sorted
// register list FList, the LDS visited table, the admissibility test of an id under a FilterArgs block and the distance
// of a stored row.  gfx950 only; include from .hip files.
#pragma once

#include "search_common.h"
#include "search_filtered.h"

namespace hx {

constexpr u64 FKEY_INVALID = ~0ull;

__device__ __forceinline__ u64 wave_min64(u64 x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o);
        const u64 y = ((u64)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

// ---------------------------------------------------------------------------------------------
// A sorted register list of up to 64 R keys (list[64 r + lane]), FKEY_INVALID beyond n_cur.
// ---------------------------------------------------------------------------------------------
template <int R>
struct FList {
    u64 L[R];
    uint32_t n_cur;  // wave-uniform
    u64 last;        // the largest key when the list holds cap keys, else FKEY_INVALID

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int r = 0; r < R; r++) L[r] = FKEY_INVALID;
        n_cur = 0;
        last = FKEY_INVALID;
    }
    __device__ __forceinline__ bool full(uint32_t cap) const { return n_cur >= cap; }
    __device__ __forceinline__ u64 front() const { return readlane64(L[0], 0); }

    __device__ __forceinline__ void refresh_last(uint32_t cap) {
        u64 k = FKEY_INVALID;
        if (n_cur >= cap) {
            const uint32_t pos = cap - 1;
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((pos >> 6) == (uint32_t)r) k = readlane64(L[r], pos & 63);
        }
        last = k;
    }

    // Merge the wave's keys (FKEY_INVALID = none; distinct and not in the list) and keep the cap smallest:
    // rank of every survivor by ballot + popcount, scatter through the LDS buffer perm (64 R keys).
    __device__ __forceinline__ void merge(u64 key, uint32_t cap, u64 *perm, int lane) {
        const bool surv = key != FKEY_INVALID && (n_cur < cap || key < last);
        const u64 smask = __ballot(surv);
        if (smask == 0) return;
        const uint32_t m = (uint32_t)__popcll(smask);
        uint32_t shift[R];
#pragma unroll
        for (int r = 0; r < R; r++) shift[r] = 0;
        uint32_t my_rank = 0;
        u64 it = smask;
        while (it) {
            const int j = __ffsll((long long)it) - 1;
            it &= it - 1;
            const u64 e = readlane64(key, j);
            uint32_t below = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool lt = L[r] < e;  // invalid entries are the maximum
                below += (uint32_t)__popcll(__ballot(lt));
                shift[r] += lt ? 0u : 1u;
            }
            if (surv && e < key) my_rank++;
            if (lane == j) my_rank += below;
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            const uint32_t np = idx + shift[r];
            if (idx < n_cur && np < cap) perm[np] = L[r];
        }
        if (surv && my_rank < cap) perm[my_rank] = key;
        n_cur = min(n_cur + m, cap);
        wave_fence();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            L[r] = idx < n_cur ? perm[idx] : FKEY_INVALID;
        }
        wave_fence();
        refresh_last(cap);
    }

    // merge for keys that may repeat (result lists of shards that overlap): a key equal to one in the list, or to the
    // key of a lower lane, is dropped first, so that what merge sees is distinct and new -- its ranks are then dense and
    // every slot of perm it reads back was written in the same call
    __device__ __forceinline__ void merge_unique(u64 key, uint32_t cap, u64 *perm, int lane) {
        u64 it = __ballot(key != FKEY_INVALID && (n_cur < cap || key < last));
        bool dup = false;
        while (it) {
            const int j = __ffsll((long long)it) - 1;
            it &= it - 1;
            const u64 e = readlane64(key, j);
            bool known = lane < j && key == e;
#pragma unroll
            for (int r = 0; r < R; r++) known |= L[r] == e;
            const bool any = __ballot(known) != 0;
            if (lane == j) dup = any;
        }
        merge(dup ? FKEY_INVALID : key, cap, perm, lane);
    }

    // drop the head: every key moves one lane down, lane 63 of register r takes lane 0 of register r + 1
    __device__ __forceinline__ void pop_front(uint32_t cap, int lane) {
        const int src = ((lane + 1) & 63) << 2;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)L[r]);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(L[r] >> 32));
            u64 nx = FKEY_INVALID;
            if (r + 1 < R) nx = readlane64(L[r + 1 < R ? r + 1 : r], 0);
            L[r] = lane == 63 ? nx : (((u64)hi << 32) | lo);
        }
        n_cur--;
        refresh_last(cap);
    }
};

// LDS visited table: buckets of four slots, ds_read_b128 + one compare-and-swap (the generic kernel's table).
// Returns true when id was absent (and is now present).
__device__ __forceinline__ bool filt_visit(uint32_t *tab, uint32_t slots_log2, uint32_t id) {
    const uint32_t bmask = ((1u << slots_log2) - 1) >> 2;
    uint32_t b = (id * 0x9E3779B1u) >> (32 - (slots_log2 - 2));
    while (true) {
        const uint4 bk = *reinterpret_cast<const uint4 *>(tab + 4 * b);
        if (bk.x == id || bk.y == id || bk.z == id || bk.w == id) return false;
        int j = -1;
        if (bk.x == HX_EMPTY_SLOT)
            j = 0;
        else if (bk.y == HX_EMPTY_SLOT)
            j = 1;
        else if (bk.z == HX_EMPTY_SLOT)
            j = 2;
        else if (bk.w == HX_EMPTY_SLOT)
            j = 3;
        if (j < 0) {
            b = (b + 1) & bmask;
            continue;
        }
        if (atomicCAS(&tab[4 * b + j], HX_EMPTY_SLOT, id) == HX_EMPTY_SLOT) return true;
    }
}

// admissible: allowed (below the query's bound, its label in the query's range when the call has a label column, and
// its bit set when the query has a mask) and not deleted.  The pointer tests are uniform over the wave (a kernel
// argument, and the wave's own filter: one query per wave); a label or a mask word is read only for an id that got
// that far.  `filt` is the wave's one filter pointer: its mask row, or, with bit 0 set, the label column -- the kernel
// has no scalar register to spare for a second pointer or for the range, which the wave keeps in LDS (`range`: lo,
// hi - lo) and reads next to the label.  (Measured: the range in two more scalar registers costs the f32 100d and 128d
// kernels with one list register 6 and 2 vector registers, and the 128d one a wave of occupancy; DESIGN.md section
// 16.)  A wave under a range AND a mask row (hnsw_search_batch_filtered_set_range) keeps its row pointer in the other
// half of the LDS slot, nullptr without a row: one 16-byte read brings the range and the row, and the mask word is read
// for an id whose label passed.  The bound of an empty range is 0: no label is read under it.  The bound and the deleted
// set's (deny_n: 0 when nothing is deleted, so there is no pointer test) are 32 bits, as an id is, and one scalar register
// each: what the row costs in the prologue is paid for here.  A wave under K > 1 ranges
// (hnsw_search_batch_filtered_ranges; K is the kernel's argument, so the test is the wave's) has bit 1 of `filt` set as
// well -- the column's copy is aligned far beyond 4 bytes, and a third scalar register for K costs the 128d kernel the
// same wave of occupancy.  Its members (lo, hi - lo) are in LDS behind the slot, member j at
// range[4 + 2 j]; the slot holds member 0 and, where the row's pointer is otherwise (a list has no row), K: a label that
// member 0 refuses is tried against the others until one takes it.
__device__ __forceinline__ bool filt_allowed(const uint64_t *deny, uint32_t deny_n, const uint64_t *filt, uint32_t bound,
                                             const uint32_t *range, uint32_t id) {
    if (id >= bound) return false;
    if ((uintptr_t)filt & 1) {
        const uint32_t label = reinterpret_cast<const uint32_t *>((uintptr_t)filt & ~(uintptr_t)3)[id];
        const uint4 r = *reinterpret_cast<const uint4 *>(range);
        bool in = label - r.x <= r.y;  // lo <= label <= hi in one unsigned compare
        if ((uintptr_t)filt & 2) {
            for (uint32_t j = 1; j < r.z && !in; j++) {
                const uint2 m = *reinterpret_cast<const uint2 *>(range + 4 + 2 * j);
                in = label - m.x <= m.y;
            }
        } else {
            const uint64_t *row = reinterpret_cast<const uint64_t *>(((uint64_t)r.w << 32) | r.z);
            if (in && row) in = ((row[id >> 6] >> (id & 63)) & 1ull) != 0;
        }
        if (!in) return false;
    } else if (filt && ((filt[id >> 6] >> (id & 63)) & 1ull) == 0) {
        return false;
    }
    return !(id < deny_n && ((deny[id >> 6] >> (id & 63)) & 1ull) != 0);
}

// ---------------------------------------------------------------------------------------------
// Distance of one stored row to the staged query, in the reference's order of operations.
// P 16-byte pieces per (half) row and DS the dimension when known at compile time (0: runtime loops).
// QUANT8: a lane pair per row (lane h streams half h), the sum is valid on the even lane; F32: one lane per row.
// ---------------------------------------------------------------------------------------------
template <int KIND, int P, int DS>
__device__ __forceinline__ float filt_dist(const DevView &v, uint32_t id, bool active, int h, const float *yq) {
    if (KIND == HNSW_VEC_QUANT8) {
        const float *yh = yq + h * (v.half_bytes - 8);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active) {
            const uint4 *src =
                reinterpret_cast<const uint4 *>(v.rows + (size_t)id * v.row_stride + (size_t)h * v.half_bytes);
            if constexpr (P > 0 && DS > 0) {
                uint4 w[P];
#pragma unroll
                for (int p = 0; p < P; p++) w[p] = src[p];
                quant_half_sums<P, DS>(w, QLds{yh}, h, v.nch4, v.rem, acc);
            } else {
                const uint32_t np = v.half_bytes >> 4;
                const uint4 w0 = src[0];
                const float mn = __builtin_bit_cast(float, w0.x);
                const float delta = __builtin_bit_cast(float, w0.y);
                for (uint32_t p = 0; p < np; p++) {
                    const uint4 w = src[p];
                    const uint32_t dw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (p == 0 && j < 2) continue;  // header
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t e = 16 * p + 4 * j + k - 8;
                            const float x = ((float)((dw[j] >> (8 * k)) & 0xFFu) * delta) + mn;
                            const bool chunk = e < v.nch4;
                            const bool tail = !chunk && e < v.nch4 + v.rem && h == 0;
                            const float y = (chunk || tail) ? yh[e] : 0.0f;
                            const float t = x - y;
                            const float t2 = t * t;
                            if (k == 0) {
                                acc[0] += (chunk || tail) ? t2 : 0.0f;
                            } else {
                                acc[k] += chunk ? t2 : 0.0f;
                                acc[0] += tail ? t2 : 0.0f;
                            }
                        }
                    }
                }
            }
        }
        // acc.iter().sum(): ((((((a0+a1)+a2)+a3)+a4)+a5)+a6)+a7 with a4..a7 on the odd lane
        const float b0 = pair_swap(acc[0]), b1 = pair_swap(acc[1]), b2 = pair_swap(acc[2]), b3 = pair_swap(acc[3]);
        float s = 0.0f;
        s += acc[0];
        s += acc[1];
        s += acc[2];
        s += acc[3];
        s += b0;
        s += b1;
        s += b2;
        s += b3;
        return __builtin_sqrtf(s);  // valid on the even lane
    } else {
        // FullVec: one sequential sum (full.rs:24-28)
        float s = 0.0f;
        if (active) {
            const uint4 *src = reinterpret_cast<const uint4 *>(v.rows + (size_t)id * v.row_stride);
            if constexpr (P > 0 && DS > 0) {
                uint4 w[P];
#pragma unroll
                for (int p = 0; p < P; p++) w[p] = src[p];
                __builtin_amdgcn_sched_barrier(0);  // every piece requested before the chain starts
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (4 * p + j >= DS) continue;
                        const float t = __builtin_bit_cast(float, dw[j]) - yq[4 * p + j];
                        const float t2 = t * t;
                        s += t2;
                    }
                }
            } else {
                const uint32_t np = v.row_stride >> 4, d = v.dim;
                for (uint32_t p0 = 0; p0 < np; p0 += 8) {
                    uint4 w[8];
#pragma unroll
                    for (int p = 0; p < 8; p++) w[p] = (p0 + p < np) ? src[p0 + p] : make_uint4(0, 0, 0, 0);
#pragma unroll
                    for (int p = 0; p < 8; p++) {
                        const uint32_t dw[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const uint32_t e = 4 * (p0 + p) + j;
                            const bool in = e < d;
                            const float t = __builtin_bit_cast(float, dw[j]) - (in ? yq[e] : 0.0f);
                            const float t2 = t * t;
                            s += in ? t2 : 0.0f;  // +0.0 leaves a non-negative sum unchanged
                        }
                    }
                }
            }
        }
        return __builtin_sqrtf(s);
    }
}

}  // namespace hx
