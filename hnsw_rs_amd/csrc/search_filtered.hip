// search_filtered.hip -- filtered k-NN: k nearest among the ids of an allow-list, as hand-written HIP for gfx950.
//
// Graph path (hx_filt_graph_kernel): one 64-lane wave per query, as the generic kernel (search_kernels.hip).
// The upper layers are ann_by_vector's greedy ef = 1 walk, unfiltered.  Layer 0 keeps TWO sorted register
// lists of (dist_bits << 32 | id) keys instead of the one flagged list of the unfiltered search:
//   F, the frontier: unexpanded keys only, capacity ef' -- popping its head shifts the list one lane left;
//   R, the results: allowed keys only, capacity ef'.
// A key is admitted when R is not full or it is below R's largest; an admitted key enters F, and R as well
// when its id is allowed (one mask word is read per admitted key, and one word of the deleted set's mask when
// the handle has deleted ids and the key got past the allow test).  The loop stops when F is empty or its
// head lies above a full R's largest.  Keys of one pass over a row are admitted against the bound at the
// start of the pass and merged at once; that gives the expansions, counters and R of the one-key-at-a-time
// loop ("Filtered search").  One row per pass, read from the compact layout (adj0 + rows), so
// the inline-rows copy does not matter.
//
// With a label range instead of an allow-list (FilterArgs::labels) the allow test of a key is lo <= label(id) <= hi
// over the resident column, lo and hi the wave's own (picked once, as its mask pointer, and kept in LDS), one 4-byte
// read per key that got as far as a mask word is read otherwise.  With a label range AND a row of a resident mask set
// (FilterArgs::labels and ::allow together) a key is allowed when its label is in the wave's range and its bit is set in
// the wave's row, the row pointer kept in LDS next to the range.
//
// Exact path: hx_filt_compact_kernel lists the allowed, undeleted ids in ascending order (the allowed bits of a word
// read from the mask, or, under a label range, made from 64 coalesced reads of the column, or that word ANDed with the
// mask's under both); hx_filt_scan_kernel scans
// one segment of that list per block and keeps its n best (the shape of hx_brute_kernel),
// hx_filt_merge_kernel merges a query's segments.  The same kernel has a second source form (MergeLists,
// search_filtered.h): the result lists of the shards of a partitioned index, keyed by global id,
// merged the same way but for keys that two shards may both hold.
//
// Float fidelity as everywhere: -ffp-contract=off, the reference's accumulation order.

#include <algorithm>

#include "launch.h"
#include "search_common.h"
#include "search_filtered.h"

namespace hx {

namespace {

constexpr u64 FKEY_INVALID = ~0ull;

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

// ---------------------------------------------------------------------------------------------
// Graph path.  LDS: visited table (4 << slots_log2 bytes) | merge buffer (64 R keys) | query | under a label range,
// the wave's range (HX_FILT_RANGE_LDS bytes) | under K > 1 ranges, its K members (8 K bytes): filt_range_lds.
// ---------------------------------------------------------------------------------------------
template <int KIND, int P, int DS, int R>
__global__ void __launch_bounds__(64) hx_filt_graph_kernel(const DevView v, const FilterArgs a, const uint32_t slots_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    // the wave's mask and id bound, picked once (scalar: q is the block's)
    const uint32_t g = a.mask_of ? a.mask_of[q] : 0;
    // a row the set does not have (mask_of may be the caller's device memory, which the host never saw): the query's
    // own error, decided for the whole wave before a mask word is read: no walk (the status below), padded outputs,
    // and an id bound of 0, under which filt_allowed refuses every id before it touches the row pointer
    const bool bad_row = a.mask_of && g != HNSW_MASK_NONE && g >= a.n_masks;
    // (without rows a.allow is nullptr and g * a.mask_words is 0: no row)
    const uint64_t *row = g == HNSW_MASK_NONE ? nullptr : a.allow + (size_t)g * a.mask_words;
    // (bit 0: the label column; bit 1, set by the launcher: the queries are under lists of ranges, filt_allowed)
    const uint64_t *allow = a.labels ? reinterpret_cast<const uint64_t *>((uintptr_t)a.labels | 1) : row;
    // the wave's label range, picked once as well; an empty one (lo > hi) allows nothing: an id bound of 0.  Under a
    // column the bound is also the bound of the label read: the host keeps the HBM copy at least as long as the index
    // (zeros beyond the labels that were set), so label_len never is the smaller one
    uint32_t lo = 0u, hi = 0u;
    // (the query's size is the template's where the dimension is: the range's slot at a constant offset, no scalar kept)
    constexpr uint32_t YQ_BYTES = DS == 0 ? 0u : ((KIND == HNSW_VEC_QUANT8 ? 2u * (16u * P - 8u) * 4u : DS * 4u) + 15u) & ~15u;
    uint32_t *range = reinterpret_cast<uint32_t *>(smem + (4ull << slots_log2) + 64 * R * 8 + (YQ_BYTES ? YQ_BYTES : query_lds_bytes(v)));
    if ((uintptr_t)a.labels & 2) {
        // K ranges (the launcher set bit 1 of the column's pointer): lanes j < K read the query's members in one
        // coalesced read each of lo and hi.  An empty member (lo > hi) must never match, and `label - lo <= hi - lo`
        // has no such encoding: it becomes a copy of the first member that is not empty, which changes nothing under
        // any-of.  All empty: the empty range (1, 0), bound 0.  (The first such lane is found by a min-reduction in
        // vector registers: a ballot's scalar pair is one the kernel does not have here.)
        const uint32_t K = a.n_ranges;
        const bool mine = (uint32_t)lane < K;
        const size_t o = (size_t)q * K + lane;
        uint32_t l = mine ? a.range_lo[o] : 1u, h = mine ? a.range_hi[o] : 0u;
        uint32_t f = l <= h ? (uint32_t)lane : 64u;
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) f = min(f, (uint32_t)__shfl_xor((int)f, x));
        const int src = (int)((f & 63u) << 2);
        const uint32_t fl = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)l), fh = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)h);
        if (l > h) l = fl, h = fh;
        if (mine && f < 64u) *reinterpret_cast<uint2 *>(range + 4 + 2 * lane) = make_uint2(l, h - l);
        // the slot's member: any that is not empty serves
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(f < 64u ? fl : 1u));
        hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(f < 64u ? fh : 0u));
    } else if (a.labels) {
        lo = a.range_lo[q], hi = a.range_hi[q];
    }
    const uint64_t ids = g == HNSW_MASK_NONE ? a.none_bits : a.allow_bits;
    // (an id is below 2^32 - 1, HX_EMPTY_SLOT: the bound fits 32 bits)
    const uint32_t bound = bad_row || lo > hi ? 0u : (uint32_t)min(a.labels ? min(ids, a.label_len) : ids, (uint64_t)HX_EMPTY_SLOT);
    // the ids the deleted set's mask covers, as the bound of its test: 0 when nothing is deleted
    const uint32_t deny_n = a.deny ? (uint32_t)min(a.deny_bits, (uint64_t)HX_EMPTY_SLOT) : 0u;
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    u64 *perm = reinterpret_cast<u64 *>(smem + (4ull << slots_log2));
    float *yq = reinterpret_cast<float *>(perm + 64 * R);
    if (a.labels && lane == 0) {  // (read after the wave_fence of the first clear_visited)
        // the wave's mask row, when the call has rows as well, next to its range: one 16-byte read brings both
        // (under a list of ranges there is no row: K takes its place)
        const uintptr_t rw = (uintptr_t)a.labels & 2 ? (uintptr_t)a.n_ranges : (uintptr_t)row;
        *reinterpret_cast<uint4 *>(range) = make_uint4(lo, hi - lo, (uint32_t)rw, (uint32_t)(rw >> 32));
    }
    const uint32_t vis_limit = filt_visited_limit(slots_log2);

    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;  // lanes per candidate
    constexpr int CHUNK = 64 / LPC;                         // ids per pass
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;
    const uint32_t ef = a.ef;

    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0, n_vis = 0;
    int32_t status = stage_query<KIND>(v, a.Q + (size_t)q * v.dim, yq, lane) ? HNSW_OK : HNSW_ERR_NAN_INPUT;
    if (bad_row) status = HNSW_ERR_ARG;

    auto clear_visited = [&]() {
        for (uint32_t s = lane; s < (1u << (slots_log2 - 2)); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
        n_vis = 0;
    };
    // key of this lane group's id, FKEY_INVALID when not fresh; a NaN distance sets the status
    auto eval_key = [&](uint32_t id, bool fresh) -> u64 {
        const float dist = filt_dist<KIND, P, DS>(v, id, fresh, h, yq);
        if (!(fresh && h == 0)) return FKEY_INVALID;
        if (dist != dist) {
            status = HNSW_ERR_NAN_INPUT;
            return FKEY_INVALID;
        }
        return ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
    };
    // One pass over up to CHUNK ids of a row: visited filter, distances, then body(key) with the fresh keys.
    // The table's room is checked before the ids are inserted.
    auto pass = [&](uint32_t nb, bool valid, auto &&body) __attribute__((always_inline)) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
        if (cnt == 0) return;
        sum_deg += cnt;
        if (n_vis + cnt > vis_limit) {
            status = HNSW_ERR_OVERFLOW;
            return;
        }
        bool f = false;
        if (valid && h == 0) f = filt_visit(htab, slots_log2, nb);
        if (LPC == 2) f = (pair_swap_i(f ? 1 : 0) | (f ? 1 : 0)) != 0;
        const uint32_t nf = (uint32_t)__popcll(__ballot(f && h == 0));
        n_vis += nf;
        if (nf == 0) return;
        n_dist += nf;
        const u64 key = eval_key(nb, f);
        if (__ballot(status != HNSW_OK)) {
            status = HNSW_ERR_NAN_INPUT;
            return;
        }
        body(key);
    };
    // every neighbour of node cid on a layer, CHUNK ids per pass: the row, then its overflow list
    auto expand = [&](uint32_t cid, int layer, auto &&body) __attribute__((always_inline)) {
        const uint32_t *row;
        uint32_t S;
        if (layer == 0) {
            S = v.S0;
            row = v.adj0 + (size_t)cid * S;
        } else {
            S = v.S1;
            const uint32_t ub = v.upper_base[cid];
            if (ub == HX_EMPTY_SLOT) {  // Graph::neighbors_vec -> NodeNotInGraph
                status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                return;
            }
            row = v.adj_up + ((size_t)ub + layer - 1) * S;
        }
        n_exp++;
        uint32_t ovf = HX_EMPTY_SLOT;
        for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += CHUNK) {
            const uint32_t slot = c0 + cslot;
            const uint32_t nb = slot < S ? row[slot] : HX_EMPTY_SLOT;
            const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
            const u64 pm = __ballot(is_ptr);
            if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
            pass(nb, nb != HX_EMPTY_SLOT && !is_ptr, body);
        }
        if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of the row
            const uint32_t lo = v.ovf_off[ovf], hi = v.ovf_off[ovf + 1];
            for (uint32_t base = lo; base < hi && status == HNSW_OK; base += CHUNK) {
                const uint32_t i = base + cslot;
                pass(i < hi ? v.ovf_nbrs[i] : HX_EMPTY_SLOT, i < hi, body);
            }
        }
    };

    FList<R> F, Rl;
    F.clear();
    Rl.clear();
    if (status == HNSW_OK) {
        // ---- entry point and the upper layers: the greedy ef = 1 walk, unfiltered ----
        const u64 ek = eval_key(v.ep, (uint32_t)lane < (uint32_t)LPC);
        u64 best = readlane64(ek, 0);
        n_dist = 1;
        if (best == FKEY_INVALID) status = HNSW_ERR_NAN_INPUT;
        for (int layer = (int)v.nb_layers - 1; layer >= 1 && status == HNSW_OK; layer--) {
            clear_visited();
            if (lane == 0) filt_visit(htab, slots_log2, (uint32_t)best);
            wave_fence();
            n_vis = 1;
            while (status == HNSW_OK) {
                const u64 before = best;
                expand((uint32_t)before, layer, [&](u64 key) { best = min(best, wave_min64(key)); });
                if (best == before) break;
            }
        }
        // ---- layer 0: F and R ----
        if (status == HNSW_OK) {
            clear_visited();
            if (lane == 0) filt_visit(htab, slots_log2, (uint32_t)best);
            wave_fence();
            n_vis = 1;
            F.merge(lane == 0 ? best : FKEY_INVALID, ef, perm, lane);
            Rl.merge(lane == 0 && filt_allowed(a.deny, deny_n, allow, bound, range, (uint32_t)best) ? best : FKEY_INVALID, ef, perm, lane);
        }
        while (status == HNSW_OK && F.n_cur > 0) {
            const u64 c = F.front();
            if (Rl.full(ef) && c > Rl.last) break;
            F.pop_front(ef, lane);
            expand((uint32_t)c, 0, [&](u64 key) {
                // admitted against the bound at the start of the pass; R takes the allowed ones
                const bool adm = key != FKEY_INVALID && (!Rl.full(ef) || key < Rl.last);
                const bool alw = adm && filt_allowed(a.deny, deny_n, allow, bound, range, (uint32_t)key);
                F.merge(adm ? key : FKEY_INVALID, ef, perm, lane);
                Rl.merge(alw ? key : FKEY_INVALID, ef, perm, lane);
            });
        }
    }

    // ---- the first min(n, |R|) keys of R (n <= 64: register 0) ----
    const uint32_t count = status == HNSW_OK ? min(a.n, Rl.n_cur) : 0;
    if ((uint32_t)lane < a.n) {
        const bool have = (uint32_t)lane < count;
        a.out_ids[(size_t)q * a.n + lane] = have ? (uint32_t)Rl.L[0] : HX_EMPTY_SLOT;
        a.out_dists[(size_t)q * a.n + lane] =
            have ? __builtin_bit_cast(float, (uint32_t)(Rl.L[0] >> 32)) : __builtin_inff();
    }
    if (lane == 0) {
        a.out_counts[q] = count;
        hnsw_query_stats st;
        st.n_dist = n_dist;
        st.n_exp = n_exp;
        st.sum_deg = sum_deg;
        st.status = status;
        a.out_stats[q] = st;
    }
}

// ---------------------------------------------------------------------------------------------
// Exact path.  Compaction: one wave per 64 mask words; lane l owns word 64 b + l and writes its admissible ids at
// word_base[b] + (admissible ids of the wave's lower lanes).  Under a label range there is no mask word to read: the
// wave makes its 64 words together, word 64 b + j from the 64 consecutive labels of its ids -- one coalesced 256-byte
// read by the 64 lanes, the range test balloted, the ballot kept by lane j.  (A lane that read the 64 labels of its
// own word would touch 64 lines per wave instruction: the gather shape of DESIGN.md section 10.)  Under a range AND a
// mask (a.labels and a.allow) the word made from the labels is ANDed with the mask's.
// ---------------------------------------------------------------------------------------------
//
// The grouped form (gtab set; search_filtered.h): blockIdx.y is the group, and what a launch of the per-group form has in
// its arguments -- the row, the id bound, the range, the offsets and the list -- comes from the group's record, read once
// with scalar loads (the block's own).  A block at or beyond its group's words exits before it reads an offset.
struct CompactSite {
    const uint64_t *allow;
    const uint32_t *labels, *word_base;
    uint32_t *ids;
    uint64_t allow_bits, n_words;
    uint32_t lo, hi;
};
__global__ void __launch_bounds__(64) hx_filt_compact_kernel(const FilterArgs fa, uint64_t n_words,
                                                             const uint32_t *word_base, uint32_t *ids, const RangeList rl,
                                                             const ExactGroup *gtab) {
    const int lane = threadIdx.x;
    CompactSite a{fa.allow, fa.labels, word_base, ids, fa.allow_bits, n_words, fa.lo, fa.hi};
    if (gtab) {
        const ExactGroup g = gtab[blockIdx.y];
        a.allow = g.allow;
        a.labels = g.ranged ? fa.labels : nullptr;
        a.word_base = g.word_base;
        a.ids = g.ids;
        a.allow_bits = g.allow_bits;
        a.n_words = (g.allow_bits + 63) / 64;
        a.lo = g.lo, a.hi = g.hi;
        if ((uint64_t)blockIdx.x * 64 >= a.n_words) return;
    }
    n_words = a.n_words;
    const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
    u64 bits = 0;
    if (a.labels) {
        if (rl.n > 1) {  // a list of ranges (none of them empty): the label in any of them, inside the same ballot
            const uint64_t id0 = (uint64_t)blockIdx.x * 4096 + lane;
            for (int j = 0; j < 64; j++) {
                const uint64_t id = id0 + 64 * j;
                const uint32_t label = id < fa.label_len ? a.labels[id] : 0u;
                bool any = false;
                for (uint32_t k = 0; k < rl.n; k++) any |= label - rl.lo[k] <= rl.hi[k] - rl.lo[k];
                const u64 in = __ballot(any);
                if (lane == j) bits = in;
            }
        } else if (a.lo <= a.hi) {  // (an empty range reads no label)
            const uint64_t id0 = (uint64_t)blockIdx.x * 4096 + lane;
#pragma unroll 8
            for (int j = 0; j < 64; j++) {
                const uint64_t id = id0 + 64 * j;
                const uint32_t label = id < fa.label_len ? a.labels[id] : 0u;
                const u64 in = __ballot(label >= a.lo && label <= a.hi);
                if (lane == j) bits = in;
            }
        }
        if (w >= n_words)
            bits = 0;
        else if (a.allow)  // a range AND a mask row: the word made from the labels, ANDed with the row's
            bits &= a.allow[w];
    } else {
        bits = w < n_words ? (a.allow ? a.allow[w] : ~0ull) : 0;
    }
    if (w * 64 + 64 > a.allow_bits) {  // ids at and beyond allow_bits are not allowed
        const uint64_t keep = a.allow_bits > w * 64 ? a.allow_bits - w * 64 : 0;
        bits &= keep >= 64 ? ~0ull : ((1ull << keep) - 1);
    }
    if (fa.deny && w * 64 < fa.deny_bits) bits &= ~fa.deny[w];  // (deny_bits is a multiple of 64)
    const uint32_t c = (uint32_t)__popcll(bits);
    uint32_t incl = c;  // inclusive prefix over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += y;
    }
    uint32_t pos = a.word_base[blockIdx.x] + incl - c;
    while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        a.ids[pos++] = (uint32_t)(w * 64 + b);
    }
}

// Scan: block (seg, y) keeps the n best of query y's segment of the list; part[(y nseg + seg) n + i].  The grouped form
// (qtab set): the list, A and nseg are query y's own (its record, one 16-byte scalar read), its partial lists start at
// row rec.seg >> HX_FILT_SEG_BITS instead of y nseg, and a block beyond its query's segments exits.
template <int KIND>
__global__ void __launch_bounds__(64) hx_filt_scan_kernel(const DevView v, const FilterArgs a, const uint32_t *ids,
                                                          uint32_t A, uint32_t nseg, u64 *part, int32_t *part_status,
                                                          const ExactQuery *qtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *perm = reinterpret_cast<u64 *>(smem);
    float *yq = reinterpret_cast<float *>(perm + 64);
    const int lane = threadIdx.x;
    const uint32_t seg = blockIdx.x, y = blockIdx.y;
    size_t row = (size_t)y * nseg + seg;  // of part and part_status
    if (qtab) {
        const ExactQuery rec = qtab[y];
        ids = rec.ids;
        A = rec.A;
        nseg = rec.seg & ((1u << HX_FILT_SEG_BITS) - 1);
        if (seg >= nseg) return;
        row = (size_t)(rec.seg >> HX_FILT_SEG_BITS) + seg;
    }
    const uint32_t q = a.qsel ? a.qsel[y] : y;
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    bool bad = !stage_query<KIND>(v, a.Q + (size_t)q * v.dim, yq, lane);
    FList<1> wl;
    wl.clear();
    const uint32_t per = (A + nseg - 1) / nseg;
    const uint32_t lo = min(A, per * seg), hi = min(A, lo + per);
    for (uint32_t base = lo; base < hi && !bad; base += CHUNK) {
        const uint32_t i = base + lane / LPC;
        const bool active = i < hi;
        const uint32_t id = active ? ids[i] : 0;
        const float dist = filt_dist<KIND, 0, 0>(v, id, active, h, yq);
        u64 key = FKEY_INVALID;
        if (active && h == 0) {
            if (dist != dist)
                bad = true;
            else
                key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
        }
        bad = __ballot(bad) != 0;
        wl.merge(key, a.n, perm, lane);
    }
    if ((uint32_t)lane < a.n) part[row * a.n + lane] = wl.L[0];
    if (lane == 0) part_status[row] = bad ? HNSW_ERR_NAN_INPUT : HNSW_OK;
}

// The merge kernel's shard-list form (MergeLists, search_filtered.h): query blockIdx.x's lists of the m.n_shards shards,
// lane j holding entry j of a list, folded into its top a.n by (distance bits, global id).  The steps depend on one
// another only through the list: everything shard s + 1 holds for the query is requested before shard s is merged, the
// ids and distances of a whole row whatever its count says (the row exists: presence is decided when they are there).
__device__ __forceinline__ void merge_shard_lists(const FilterArgs &a, const MergeLists &m, u64 *perm, int lane) {
    const uint32_t q = blockIdx.x, n = a.n;
    const bool row = (uint32_t)lane < n;
    const uint32_t *dist_bits = reinterpret_cast<const uint32_t *>(m.dists);
    struct Piece {
        uint32_t id, bits, cnt;
        hnsw_query_stats st;
    };
    auto load = [&](uint32_t s) {
        const size_t o = (size_t)s * m.nq + q;
        Piece p;
        p.id = row ? m.ids[o * n + lane] : HX_EMPTY_SLOT;
        p.bits = row ? dist_bits[o * n + lane] : 0u;
        p.cnt = m.counts ? m.counts[o] : 0u;
        if (m.stats) {
            p.st = m.stats[o];
        } else {
            p.st.n_dist = p.st.n_exp = p.st.sum_deg = 0;
            p.st.status = HNSW_OK;
        }
        return p;
    };
    FList<1> wl;
    wl.clear();
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    Piece nx = load(0);
    for (uint32_t s = 0; s < m.n_shards; s++) {
        const Piece p = nx;
        if (s + 1 < m.n_shards) nx = load(s + 1);
        st.n_dist += p.st.n_dist;
        st.n_exp += p.st.n_exp;
        st.sum_deg += p.st.sum_deg;
        if (st.status == HNSW_OK) st.status = p.st.status;  // the lowest-numbered shard that failed
        const bool present = row && (m.counts ? (uint32_t)lane < p.cnt : p.id != HX_EMPTY_SLOT);
        const uint32_t gid = m.base[s] + m.stride[s] * p.id;  // (all 32 bits: the list has no flag bit)
        wl.merge_unique(present ? ((u64)p.bits << 32) | gid : FKEY_INVALID, n, perm, lane);
    }
    // a query some shard failed: the library's per-query error convention, count 0 and padded rows
    const uint32_t count = st.status == HNSW_OK ? wl.n_cur : 0;
    if (row) {
        const bool have = (uint32_t)lane < count;
        a.out_ids[(size_t)q * n + lane] = have ? (uint32_t)wl.L[0] : HX_EMPTY_SLOT;
        a.out_dists[(size_t)q * n + lane] = have ? __builtin_bit_cast(float, (uint32_t)(wl.L[0] >> 32)) : __builtin_inff();
    }
    if (lane == 0) {
        if (a.out_counts) a.out_counts[q] = count;
        if (a.out_stats) a.out_stats[q] = st;
    }
}

// The merge kernel's collapse form (MergeLists with per_group != 0, search_filtered.h): query
// blockIdx.x's candidate list of m.pool entries, lane l holding entries l, l + 64, l + 128 and l + 192, collapsed by label
// into its m.n_groups nearest groups of at most m.per_group entries.  Entry j has the rank r_j (present entries before
// it with its label) and the first member f_j (the first present entry with its label), found in one pass over the
// present entries with their labels broadcast from LDS; its group's number g_j is the number of first members before
// f_j, a popcount prefix of their ballots.  A kept entry (r_j < per_group, g_j < n_groups) puts its index into the slot
// table [n_groups][per_group] in LDS, and the lanes stream the table out, 64 slots at a time: every output word is
// written once, a pad where its slot is empty.
//   lab[256]  the entries' labels   slot[1024]  the slot table (HX_GROUP_NO_ENTRY: empty)   gsz[256]  the groups' sizes
#define HX_GROUP_LDS (HX_GROUP_POOL_MAX * 4 + HX_GROUP_SLOTS_MAX * 2 + HX_GROUP_POOL_MAX * 2)
#define HX_GROUP_NO_ENTRY 0xFFFFu
__device__ __forceinline__ void collapse_by_label(const FilterArgs &a, const MergeLists &m, unsigned char *lds, int lane) {
    uint32_t *lab = reinterpret_cast<uint32_t *>(lds);
    uint16_t *slot = reinterpret_cast<uint16_t *>(lds + HX_GROUP_POOL_MAX * 4);
    uint16_t *gsz = slot + HX_GROUP_SLOTS_MAX;
    const uint32_t q = blockIdx.x, pool = m.pool, G = m.n_groups, P = m.per_group, GP = G * P;
    if (pool > HX_GROUP_POOL_MAX || G > pool || P > pool || GP > HX_GROUP_SLOTS_MAX) return;  // (the launcher's limits)
    const uint32_t *dist_bits = reinterpret_cast<const uint32_t *>(m.dists);
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (m.stats) st = m.stats[q];
    const uint32_t cnt = m.counts ? min(m.counts[q], pool) : pool;
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0 and padded rows
    uint32_t id[4], bits[4], mylab[4];
    bool pres[4];
    u64 pm[4];  // the present entries, one ballot per register
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t j = 64u * k + lane;
        const bool in = j < pool;
        id[k] = in ? m.ids[(size_t)q * pool + j] : HX_EMPTY_SLOT;
        bits[k] = in ? dist_bits[(size_t)q * pool + j] : 0u;
        pres[k] = ok && in && (m.counts ? j < cnt : id[k] != HX_EMPTY_SLOT);
        mylab[k] = pres[k] && id[k] < m.label_len ? m.labels[id[k]] : 0u;  // (label_len is 0 without a column)
        lab[j] = mylab[k];
        pm[k] = __ballot(pres[k]);
    }
    for (uint32_t s = lane; s < GP; s += 64) slot[s] = HX_GROUP_NO_ENTRY;
    wave_fence();
    uint32_t r[4], f[4], tot[4];
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = tot[k] = 0, f[k] = ~0u;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        u64 it = pm[w];
        while (it) {  // (wave-uniform)
            const uint32_t i = 64u * w + (uint32_t)(__ffsll((long long)it) - 1);
            it &= it - 1;
            const uint32_t li = lab[i];  // one address for the wave: a broadcast
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool same = li == mylab[k];
                if (same && f[k] == ~0u) f[k] = i;
                r[k] += same && i < 64u * k + lane ? 1u : 0u;
                tot[k] += same ? 1u : 0u;
            }
        }
    }
    bool first[4];
    u64 fm[4];  // the first members, one ballot per register
    uint32_t before[4], n_all = 0;  // first members in the registers before w; groups in the pool
#pragma unroll
    for (int k = 0; k < 4; k++) {
        first[k] = pres[k] && r[k] == 0;
        fm[k] = __ballot(first[k]);
        before[k] = n_all;
        n_all += (uint32_t)__popcll(fm[k]);
    }
    const uint32_t count = min(n_all, G);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!pres[k]) continue;  // (f is an index below pool from here on)
        const uint32_t fw = f[k] >> 6, fb = f[k] & 63;
        const u64 mw = fw == 0 ? fm[0] : fw == 1 ? fm[1] : fw == 2 ? fm[2] : fm[3];
        const uint32_t bw = fw == 0 ? before[0] : fw == 1 ? before[1] : fw == 2 ? before[2] : before[3];
        const uint32_t g = bw + (uint32_t)__popcll(mw & ((1ull << fb) - 1));
        if (g >= G) continue;
        if (r[k] < P) slot[g * P + r[k]] = (uint16_t)(64u * k + lane);
        if (first[k]) gsz[g] = (uint16_t)min(tot[k], P);
    }
    wave_fence();
    // the table, streamed out: slot s of the query from entry slot[s]'s registers (every lane takes part in the shuffles)
    for (uint32_t base = 0; base < GP; base += 64) {
        const uint32_t s = base + lane;
        const uint32_t src = s < GP ? slot[s] : HX_GROUP_NO_ENTRY;
        uint32_t vi = HX_EMPTY_SLOT, vb = 0x7F800000u;  // the pads: no id, +inf
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t ti = (uint32_t)__shfl((int)id[k], (int)(src & 63));
            const uint32_t tb = (uint32_t)__shfl((int)bits[k], (int)(src & 63));
            if ((src >> 6) == (uint32_t)k) vi = ti, vb = tb;
        }
        if (s < GP) {
            a.out_ids[(size_t)q * GP + s] = vi;
            a.out_dists[(size_t)q * GP + s] = __builtin_bit_cast(float, vb);
        }
    }
    for (uint32_t s = lane; s < G; s += 64) {
        const bool have = s < count;
        const uint32_t src = have ? slot[s * P] : 0u;  // (a group's best member is always kept)
        m.group_labels[(size_t)q * G + s] = have ? lab[src & (HX_GROUP_POOL_MAX - 1)] : 0u;
        m.group_sizes[(size_t)q * G + s] = have ? (uint32_t)gsz[s] : 0u;
    }
    if (lane == 0) {
        if (a.out_counts) a.out_counts[q] = count;
        if (a.out_stats) a.out_stats[q] = st;
    }
}

// The merge kernel's cut form (MergeLists with cut_out != 0, search_filtered.h): the candidate
// list of m.pool entries of query a.qsel[blockIdx.x] (or blockIdx.x), walked 64 entries at a time with the next 64
// already requested, cut at the query's radius.  A kept entry's slot is the number kept before it: the running total of
// the steps behind plus the popcount of this step's ballot below the lane, so the kept entries stay in their input
// order.  Then the lanes stream the pad from the count to the end of the row: every output word is written once.  No
// LDS, no list registers.
__device__ __forceinline__ void cut_at_radius(const FilterArgs &a, const MergeLists &m, int lane) {
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    const uint32_t n_in = m.pool, n_out = m.cut_out;
    if (q >= m.nq || n_in > n_out || n_out > HX_RADIUS_MAX_N) return;  // (the launcher's limits; a selection's bound)
    const uint32_t *dist_bits = reinterpret_cast<const uint32_t *>(m.dists);
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (m.stats) st = m.stats[q];
    const float radius = m.radius[q];
    const uint32_t cnt = m.counts ? min(m.counts[q], n_in) : n_in;
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0, a padded row, no flag
    const size_t in0 = (size_t)q * n_in, out0 = (size_t)q * n_out;
    uint32_t w = 0, n_present = 0;  // wave-uniform
    uint32_t nx_id = (uint32_t)lane < n_in ? m.ids[in0 + lane] : HX_EMPTY_SLOT;
    uint32_t nx_bits = (uint32_t)lane < n_in ? dist_bits[in0 + lane] : 0u;
    for (uint32_t base = 0; base < n_in; base += 64) {
        const uint32_t j = base + lane, id = nx_id, bits = nx_bits;
        if (j + 64 < n_in) {
            nx_id = m.ids[in0 + j + 64];
            nx_bits = dist_bits[in0 + j + 64];
        }
        const bool present = ok && j < n_in && (m.counts ? j < cnt : id != HX_EMPTY_SLOT);
        const bool kept = present && __builtin_bit_cast(float, bits) <= radius;  // (false for a NaN on either side)
        const u64 km = __ballot(kept);
        n_present += (uint32_t)__popcll(__ballot(present));
        if (kept) {
            const uint32_t slot = w + (uint32_t)__popcll(km & ((1ull << lane) - 1));  // < n_in <= n_out
            a.out_ids[out0 + slot] = id;
            a.out_dists[out0 + slot] = __builtin_bit_cast(float, bits);
        }
        w += (uint32_t)__popcll(km);
    }
    for (uint32_t s = w + lane; s < n_out; s += 64) {
        a.out_ids[out0 + s] = HX_EMPTY_SLOT;
        a.out_dists[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        if (a.out_counts) a.out_counts[q] = w;
        if (m.flags) m.flags[q] = ok && n_present == n_in && w == n_present ? HX_RADIUS_MORE : 0u;
        if (a.out_stats) a.out_stats[q] = st;
    }
}

// The merge kernel's drop form (MergeLists with drop_out != 0, search_filtered.h): the candidate
// list of m.pool entries of query a.qsel[blockIdx.x] (or blockIdx.x), walked as the cut form walks it, without the
// entries whose id one of the query's exclusion ids names.  The exclusion ids sit one per lane; a step compares its 64
// entries with each present one, broadcast by readlane (the walk of the ballot's set bits is the wave's).  A kept
// entry's slot is the number kept before it; the wave stops storing at drop_out but walks on, so that `dropped` covers
// all of pool.  Then the lanes stream the pad: every output word is written once.  No LDS, no list registers.
__device__ __forceinline__ void drop_excluded(const FilterArgs &a, const MergeLists &m, int lane) {
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    const uint32_t n_in = m.pool, n_out = m.drop_out, width = m.ex_width;
    if (q >= m.nq || n_out > n_in || n_in > HX_RADIUS_MAX_N || width > HX_DROP_MAX_WIDTH) return;  // (the launcher's limits)
    const uint32_t *dist_bits = reinterpret_cast<const uint32_t *>(m.dists);
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (m.stats) st = m.stats[q];
    bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0, a padded row, nothing dropped
    if (m.src_status) {
        const int32_t src = m.src_status[q];
        if (src != HNSW_OK) {
            ok = false;
            st.status = src;
        }
    }
    const uint32_t cnt = m.counts ? min(m.counts[q], n_in) : n_in;
    const uint32_t ex = (uint32_t)lane < width ? m.ex[(size_t)q * width + lane] : HX_EMPTY_SLOT;
    const u64 exm = __ballot(ex != HX_EMPTY_SLOT);
    const size_t in0 = (size_t)q * n_in, out0 = (size_t)q * n_out;
    uint32_t w = 0, gone = 0;  // wave-uniform
    uint32_t nx_id = (uint32_t)lane < n_in ? m.ids[in0 + lane] : HX_EMPTY_SLOT;
    uint32_t nx_bits = (uint32_t)lane < n_in ? dist_bits[in0 + lane] : 0u;
    for (uint32_t base = 0; base < n_in; base += 64) {
        const uint32_t j = base + lane, id = nx_id, bits = nx_bits;
        if (j + 64 < n_in) {
            nx_id = m.ids[in0 + j + 64];
            nx_bits = dist_bits[in0 + j + 64];
        }
        const bool present = ok && j < n_in && (m.counts ? j < cnt : id != HX_EMPTY_SLOT);
        bool hit = false;
        for (u64 rest = exm; rest; rest &= rest - 1)
            hit |= id == (uint32_t)__builtin_amdgcn_readlane((int)ex, __builtin_ctzll(rest));
        const bool kept = present && !hit;
        const u64 km = __ballot(kept);
        gone += (uint32_t)__popcll(__ballot(present && hit));
        const uint32_t slot = w + (uint32_t)__popcll(km & ((1ull << lane) - 1));
        if (kept && slot < n_out) {
            a.out_ids[out0 + slot] = id;
            a.out_dists[out0 + slot] = __builtin_bit_cast(float, bits);
        }
        w += (uint32_t)__popcll(km);
    }
    w = min(w, n_out);
    for (uint32_t s = w + lane; s < n_out; s += 64) {
        a.out_ids[out0 + s] = HX_EMPTY_SLOT;
        a.out_dists[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        if (a.out_counts) a.out_counts[q] = w;
        if (m.dropped) m.dropped[q] = gone;
        if (a.out_stats) a.out_stats[q] = st;
    }
}

// Merge: one wave per query folds the nseg partial lists into its top n and writes the results.  With m.ids set the
// lists are those of m.n_shards shards instead (merge_shard_lists; A, nseg, part and part_status are not read), or, with
// m.per_group set as well, the query's one candidate list, collapsed by label (collapse_by_label), or, with m.cut_out
// set instead, that list cut at the query's radius (cut_at_radius), or, with m.drop_out set instead, that list without
// the query's exclusion ids (drop_excluded).  With
// qtab set (the grouped form) A, nseg and the first row of the query's partial lists are its record's.
__global__ void __launch_bounds__(64) hx_filt_merge_kernel(const FilterArgs a, uint32_t A, uint32_t nseg,
                                                           const u64 *part, const int32_t *part_status,
                                                           const MergeLists m, const ExactQuery *qtab) {
    // the merges' 64 keys of scatter room; the collapse form's labels, slot table and group sizes
    __shared__ __attribute__((aligned(16))) unsigned char lds[HX_GROUP_LDS];
    u64 *perm = reinterpret_cast<u64 *>(lds);
    const int lane = threadIdx.x;
    if (m.per_group) {  // (kernel arguments: the branches are the wave's)
        collapse_by_label(a, m, lds, lane);
        return;
    }
    if (m.ids) {
        if (m.cut_out)
            cut_at_radius(a, m, lane);
        else if (m.drop_out)
            drop_excluded(a, m, lane);
        else
            merge_shard_lists(a, m, perm, lane);
        return;
    }
    const uint32_t y = blockIdx.x;
    const uint32_t q = a.qsel ? a.qsel[y] : y;
    size_t row0 = (size_t)y * nseg;
    if (qtab) {
        const ExactQuery rec = qtab[y];
        A = rec.A;
        nseg = rec.seg & ((1u << HX_FILT_SEG_BITS) - 1);
        row0 = rec.seg >> HX_FILT_SEG_BITS;
    }
    FList<1> wl;
    wl.clear();
    bool bad = false;
    for (uint32_t s = 0; s < nseg; s++) {
        const size_t o = row0 + s;
        bad |= part_status[o] != HNSW_OK;
        wl.merge((uint32_t)lane < a.n ? part[o * a.n + lane] : FKEY_INVALID, a.n, perm, lane);
    }
    const uint32_t count = bad ? 0 : wl.n_cur;
    if ((uint32_t)lane < a.n) {
        const bool have = (uint32_t)lane < count;
        a.out_ids[(size_t)q * a.n + lane] = have ? (uint32_t)wl.L[0] : HX_EMPTY_SLOT;
        a.out_dists[(size_t)q * a.n + lane] = have ? __builtin_bit_cast(float, (uint32_t)(wl.L[0] >> 32)) : __builtin_inff();
    }
    if (lane == 0) {
        a.out_counts[q] = count;
        hnsw_query_stats st;
        st.n_dist = A;
        st.n_exp = 0;
        st.sum_deg = 0;
        st.status = bad ? HNSW_ERR_NAN_INPUT : HNSW_OK;
        a.out_stats[q] = st;
    }
}

template <int KIND, int P, int DS, int R>
int launch_graph_r(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    const size_t lds = (4ull << slots_log2) + 64ull * R * 8 + query_lds_bytes(v) + filt_range_lds(a.labels != nullptr, a.n_ranges);
    return launch_checked({"filtered search kernel launch", "filtered search needs %zu bytes of LDS (> 160 KiB)"},
                          hx_filt_graph_kernel<KIND, P, DS, R>, dim3(nblocks), dim3(64), lds, stream, v, a, slots_log2);
}

template <int KIND, int P, int DS>
int launch_graph(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    if (a.ef <= 64) return launch_graph_r<KIND, P, DS, 1>(v, a, nblocks, slots_log2, stream);
    if (a.ef <= 128) return launch_graph_r<KIND, P, DS, 2>(v, a, nblocks, slots_log2, stream);
    return launch_graph_r<KIND, P, DS, 4>(v, a, nblocks, slots_log2, stream);
}

}  // namespace

uint32_t filt_first_slots_log2(const DevView &v, uint32_t ef, uint32_t range_lds) {
    return std::min(default_slots_log2(ef, v.S0), filt_max_slots_log2(v, range_lds));
}

uint32_t filt_max_slots_log2(const DevView &v, uint32_t range_lds) {
    const uint32_t yqb = query_lds_bytes(v);
    uint32_t s = HX_FILT_MAX_SLOTS_LOG2;
    while (s > 12 && (4ull << s) + 64ull * 4 * 8 + yqb + range_lds > 160 * 1024) s--;
    return s;
}

int launch_filtered_graph(const DevView &v, const FilterArgs &args, uint32_t nblocks, uint32_t slots_log2,
                          hipStream_t stream) {
    FilterArgs a = args;
    if (nblocks == 0) return HNSW_OK;
    if (a.ef == 0 || a.ef > HX_FILT_MAX_EF || a.n == 0 || a.n > HX_FILT_MAX_N || a.n > a.ef) {
        set_error("filtered search: needs 1 <= n <= %d and n <= ef' <= %d", HX_FILT_MAX_N, HX_FILT_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if (a.n_ranges > HX_FILT_MAX_RANGES || (a.n_ranges > 1 && (a.allow || !a.labels || ((uintptr_t)a.labels & 3)))) {
        // (the LDS behind the slot holds that many, and no row)
        set_error("filtered search: at most %d label ranges per query, over the label column alone", HX_FILT_MAX_RANGES);
        return HNSW_ERR_ARG;
    }
    // K > 1 reaches the kernel as bit 1 of the column's pointer (its copy is aligned far beyond 4 bytes): the kernel has
    // no scalar register to keep K or a flag in while it walks (filt_allowed)
    if (a.n_ranges > 1) a.labels = reinterpret_cast<const uint32_t *>((uintptr_t)a.labels | 2);
    if (v.kind == HNSW_VEC_QUANT8) {
        if (v.dim == 100 && v.half_bytes == 64) return launch_graph<HNSW_VEC_QUANT8, 4, 100>(v, a, nblocks, slots_log2, stream);
        return launch_graph<HNSW_VEC_QUANT8, 0, 0>(v, a, nblocks, slots_log2, stream);
    }
    if (v.dim == 100 && v.row_stride == 400) return launch_graph<HNSW_VEC_F32, 25, 100>(v, a, nblocks, slots_log2, stream);
    if (v.dim == 128 && v.row_stride == 512) return launch_graph<HNSW_VEC_F32, 32, 128>(v, a, nblocks, slots_log2, stream);
    return launch_graph<HNSW_VEC_F32, 0, 0>(v, a, nblocks, slots_log2, stream);
}

int launch_filter_compact(const FilterArgs &a, uint64_t n_words, const uint32_t *word_base, uint32_t *ids,
                          hipStream_t stream, const RangeList *list) {
    if (n_words == 0) return HNSW_OK;
    if (list && (list->n > HX_FILT_MAX_RANGES || (list->n > 1 && (!a.labels || a.allow)))) {
        set_error("filter compaction: at most %d label ranges, over the label column alone", HX_FILT_MAX_RANGES);
        return HNSW_ERR_ARG;
    }
    const uint64_t nb = (n_words + 63) / 64;
    return launch_checked({"filter compaction kernel launch"}, hx_filt_compact_kernel, dim3((uint32_t)nb), dim3(64), 0, stream, a,
                          n_words, word_base, ids, list ? *list : RangeList{}, static_cast<const ExactGroup *>(nullptr));
}

int launch_filter_compact_grouped(const FilterArgs &a, const ExactGroup *gtab, uint32_t ngroups, uint64_t max_words,
                                  hipStream_t stream) {
    if (ngroups == 0 || max_words == 0) return HNSW_OK;
    if (!gtab || ngroups > 65535) {
        set_error("filter compaction: the grouped form needs its table and at most 65535 groups per launch");
        return HNSW_ERR_ARG;
    }
    const uint64_t nb = (max_words + 63) / 64;
    return launch_checked({"filter compaction kernel launch"}, hx_filt_compact_kernel, dim3((uint32_t)nb, ngroups), dim3(64), 0,
                          stream, a, (uint64_t)0, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr),
                          RangeList{}, gtab);
}

uint32_t filt_exact_segments(uint64_t A, uint32_t nsel) {
    // about 2048 ids per block, fewer segments when the batch alone fills the chip
    uint64_t s = (A + 2047) / 2048;
    const uint64_t cap = std::max<uint64_t>(1, 262144 / std::max<uint32_t>(1, nsel));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({s, 256, cap}));
}

int launch_filtered_exact(const DevView &v, const FilterArgs &a, uint32_t nsel, const uint32_t *ids, uint32_t A,
                          uint32_t nseg, unsigned long long *part, int32_t *part_status, hipStream_t stream) {
    if (nsel == 0) return HNSW_OK;
    if (a.n == 0 || a.n > HX_FILT_MAX_N || nsel > 65535 || nseg == 0) {
        set_error("filtered exact search: needs 1 <= n <= %d and at most 65535 queries per launch", HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    // scan, then merge: two launches back to back under one message, the second only after the first was accepted
    const LaunchSite site{"filtered exact search launch"};
    if (int rc = launch_checked(site, v.kind == HNSW_VEC_QUANT8 ? hx_filt_scan_kernel<HNSW_VEC_QUANT8> : hx_filt_scan_kernel<HNSW_VEC_F32>,
                                dim3(nseg, nsel), dim3(64), 64 * 8 + (size_t)query_lds_bytes(v), stream, v, a, ids, A, nseg, part,
                                part_status, static_cast<const ExactQuery *>(nullptr)))
        return rc;
    return launch_checked(site, hx_filt_merge_kernel, dim3(nsel), dim3(64), 0, stream, a, A, nseg, part, part_status,
                          MergeLists{}, static_cast<const ExactQuery *>(nullptr));
}

int launch_filtered_exact_grouped(const DevView &v, const FilterArgs &a, uint32_t nsel, const ExactQuery *qtab,
                                  uint32_t max_nseg, unsigned long long *part, int32_t *part_status, hipStream_t stream) {
    if (nsel == 0) return HNSW_OK;
    if (a.n == 0 || a.n > HX_FILT_MAX_N || nsel > 65535 || max_nseg == 0 || max_nseg >= (1u << HX_FILT_SEG_BITS) || !qtab || !a.qsel) {
        set_error("filtered exact search: the grouped form needs 1 <= n <= %d, at most 65535 queries per launch and its table",
                  HX_FILT_MAX_N);
        return HNSW_ERR_ARG;
    }
    const LaunchSite site{"filtered exact search launch"};
    if (int rc = launch_checked(site, v.kind == HNSW_VEC_QUANT8 ? hx_filt_scan_kernel<HNSW_VEC_QUANT8> : hx_filt_scan_kernel<HNSW_VEC_F32>,
                                dim3(max_nseg, nsel), dim3(64), 64 * 8 + (size_t)query_lds_bytes(v), stream, v, a,
                                static_cast<const uint32_t *>(nullptr), 0u, 0u, part, part_status, qtab))
        return rc;
    return launch_checked(site, hx_filt_merge_kernel, dim3(nsel), dim3(64), 0, stream, a, 0u, 0u, part, part_status,
                          MergeLists{}, qtab);
}

int launch_merge_lists(const MergeLists &m, uint32_t n, uint32_t *out_ids, float *out_dists, uint32_t *out_counts,
                       hnsw_query_stats *out_stats, hipStream_t stream) {
    if (m.nq == 0) return HNSW_OK;
    if (n == 0 || n > HX_FILT_MAX_N || m.n_shards == 0 || m.n_shards > HX_MERGE_MAX_SHARDS || m.nq > 0x7FFFFFFFu || !m.ids ||
        !m.dists || !out_ids || !out_dists || (m.stats != nullptr) != (out_stats != nullptr)) {
        set_error("shard merge: needs 1 <= n <= %d, 1 to %d shards, at most 2^31 - 1 queries, the lists and the outputs",
                  HX_FILT_MAX_N, HX_MERGE_MAX_SHARDS);
        return HNSW_ERR_ARG;
    }
    FilterArgs a{};  // the form reads n and the outputs
    a.n = n;
    a.out_ids = out_ids;
    a.out_dists = out_dists;
    a.out_counts = out_counts;
    a.out_stats = out_stats;
    return launch_checked({"shard merge kernel launch"}, hx_filt_merge_kernel, dim3(m.nq), dim3(64), 0, stream, a, 0u, 0u,
                          static_cast<const u64 *>(nullptr), static_cast<const int32_t *>(nullptr), m,
                          static_cast<const ExactQuery *>(nullptr));
}

int launch_group_by_label(const MergeLists &lists, uint32_t *out_ids, float *out_dists, uint32_t *out_counts,
                          hnsw_query_stats *out_stats, hipStream_t stream) {
    MergeLists m = lists;
    if (m.nq == 0) return HNSW_OK;
    if (m.pool == 0 || m.pool > HX_GROUP_POOL_MAX || m.n_groups == 0 || m.n_groups > m.pool || m.per_group == 0 ||
        m.per_group > m.pool || (uint64_t)m.n_groups * m.per_group > HX_GROUP_SLOTS_MAX || m.nq > 0x7FFFFFFFu || !m.ids ||
        !m.dists || !m.group_labels || !m.group_sizes || !out_ids || !out_dists ||
        (m.stats != nullptr) != (out_stats != nullptr)) {
        set_error("group by label: needs 1 <= n_groups, per_group <= pool <= %d, n_groups x per_group <= %d, at most 2^31 - 1 "
                  "queries, the lists and the outputs", HX_GROUP_POOL_MAX, HX_GROUP_SLOTS_MAX);
        return HNSW_ERR_ARG;
    }
    if (!m.labels) m.label_len = 0;  // no column: every label is 0 and nothing is read
    FilterArgs a{};  // the form reads the outputs
    a.out_ids = out_ids;
    a.out_dists = out_dists;
    a.out_counts = out_counts;
    a.out_stats = out_stats;
    return launch_checked({"group by label kernel launch"}, hx_filt_merge_kernel, dim3(m.nq), dim3(64), 0, stream, a, 0u, 0u,
                          static_cast<const u64 *>(nullptr), static_cast<const int32_t *>(nullptr), m,
                          static_cast<const ExactQuery *>(nullptr));
}

int launch_radius_cut(const MergeLists &lists, const uint32_t *sel, uint32_t n_sel, uint32_t *out_ids, float *out_dists,
                      uint32_t *out_counts, hnsw_query_stats *out_stats, hipStream_t stream) {
    MergeLists m = lists;
    const uint32_t nblocks = sel ? n_sel : m.nq;
    if (nblocks == 0) return HNSW_OK;
    if (m.pool == 0 || m.pool > m.cut_out || m.cut_out > HX_RADIUS_MAX_N || m.nq > 0x7FFFFFFFu || nblocks > m.nq || !m.ids ||
        !m.dists || !m.radius || !out_ids || !out_dists || (m.stats != nullptr) != (out_stats != nullptr)) {
        set_error("radius cut: needs 1 <= n_in <= n_out <= %d, at most 2^31 - 1 queries, a selection no longer than that, "
                  "the lists, the radii and the outputs", HX_RADIUS_MAX_N);
        return HNSW_ERR_ARG;
    }
    m.per_group = 0;  // (the collapse form's selector)
    FilterArgs a{};   // the form reads the selection and the outputs
    a.qsel = sel;
    a.out_ids = out_ids;
    a.out_dists = out_dists;
    a.out_counts = out_counts;
    a.out_stats = out_stats;
    return launch_checked({"radius cut kernel launch"}, hx_filt_merge_kernel, dim3(nblocks), dim3(64), 0, stream, a, 0u, 0u,
                          static_cast<const u64 *>(nullptr), static_cast<const int32_t *>(nullptr), m,
                          static_cast<const ExactQuery *>(nullptr));
}

int launch_drop_ids(const MergeLists &lists, const uint32_t *sel, uint32_t n_sel, uint32_t *out_ids, float *out_dists,
                    uint32_t *out_counts, hnsw_query_stats *out_stats, hipStream_t stream) {
    MergeLists m = lists;
    const uint32_t nblocks = sel ? n_sel : m.nq;
    if (nblocks == 0) return HNSW_OK;
    if (m.drop_out == 0 || m.drop_out > m.pool || m.pool > HX_RADIUS_MAX_N || m.ex_width == 0 || m.ex_width > HX_DROP_MAX_WIDTH ||
        m.nq > 0x7FFFFFFFu || nblocks > m.nq || !m.ids || !m.dists || !m.ex || !out_ids || !out_dists ||
        (m.stats != nullptr) != (out_stats != nullptr)) {
        set_error("drop ids: needs 1 <= n_out <= n_in <= %d, 1 <= width <= %d, at most 2^31 - 1 queries, a selection no longer "
                  "than that, the lists, the exclusion ids and the outputs", HX_RADIUS_MAX_N, HX_DROP_MAX_WIDTH);
        return HNSW_ERR_ARG;
    }
    m.per_group = 0;  // (the collapse form's selector)
    m.cut_out = 0;    // (the cut form's)
    FilterArgs a{};   // the form reads the selection and the outputs
    a.qsel = sel;
    a.out_ids = out_ids;
    a.out_dists = out_dists;
    a.out_counts = out_counts;
    a.out_stats = out_stats;
    return launch_checked({"drop ids kernel launch"}, hx_filt_merge_kernel, dim3(nblocks), dim3(64), 0, stream, a, 0u, 0u,
                          static_cast<const u64 *>(nullptr), static_cast<const int32_t *>(nullptr), m,
                          static_cast<const ExactQuery *>(nullptr));
}

}  // namespace hx
