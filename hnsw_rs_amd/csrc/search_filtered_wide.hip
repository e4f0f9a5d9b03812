// search_filtered_wide.hip -- wide filtered k-NN: up to 1024 results and ef' up to 1024 among the admissible ids, as
// hand-written HIP for gfx950.
//
// Graph path (hx_filt_wide_kernel): one 64-lane wave per query and the walk of hx_filt_graph_kernel (search_filtered.hip):
// the upper layers unfiltered, layer 0 with the frontier F and the results R, a pass's fresh keys admitted against max(R)
// at the start of the pass and merged at once, the same distance routine.  What differs is where the state lives:
//   F, R      sorted arrays of 8-byte keys in LDS, each a ring of wide_ring_keys(ef') slots.  F is the window
//             [head, head + len) of its ring: popping its smallest key is head++, nothing moves.  The length, the
//             largest key of a full list and F's smallest key are wave-uniform registers: the loop's break test and the
//             admission test read no LDS.
//   a merge   the pass's admitted keys are sorted across the wave in registers (bitonic, 21 exchanges) and parked in LDS;
//             each finds its rank in the list by binary search; the list's tail from the smallest rank on is moved back
//             to front in 64-key pieces, each key by the number of new keys below it (a binary search over the parked
//             keys); then the new keys are written.  A piece reads its 64 keys before it writes, and writes at or above
//             where it read: only slots that later pieces do not read.  R's merge is the same routine over the allowed
//             subset of the same sorted keys.
//   visited   two levels: the bucketed LDS table of the other kernels, closed when it holds three quarters of its
//             slots; from then on an id that is not in it is claimed by one compare-and-swap in the query's own
//             open-addressed table in HBM (the scheme of hx_search_kernel's second level), closed at three quarters too.
//   output    the lanes stream the first min(n, |R|) keys of R out of LDS, 64 entries at a time, and pad behind them.
//
// Exact path: hx_filt_wide_scan_kernel evaluates one segment of at most HX_WIDE_SEG admissible ids per block into LDS,
// sorts the keys there (bitonic) and writes the first n; hx_filt_wide_merge_kernel folds a query's runs pairwise by
// merge-path ranks in LDS.  The compaction is hx_filt_compact_kernel, as it is.
//
// Float fidelity as everywhere: -ffp-contract=off, the reference's accumulation order.

#include <algorithm>

#include "launch.h"
#include "search_filtered_dev.h"
#include "search_filtered_wide.h"

namespace hx {

namespace {

__device__ __forceinline__ u64 shfl_xor64(u64 x, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o);
    return ((u64)hi << 32) | lo;
}

// the wave's 64 keys in ascending order, lane i holding the i-th smallest (FKEY_INVALID, the maximum, sorts behind)
__device__ __forceinline__ u64 wave_sort64(u64 x, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 y = shfl_xor64(x, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            x = keep_min ? (y < x ? y : x) : (y > x ? y : x);
        }
    }
    return x;
}

// entries below `key` among the n sorted keys L[(head + i) & mask], i < n: the same number of probes on every lane
__device__ __forceinline__ uint32_t lds_lower_bound(const u64 *L, uint32_t head, uint32_t mask, uint32_t n, u64 key) {
    uint32_t base = 0;
    while (n > 1) {  // (wave-uniform)
        const uint32_t half = n >> 1;
        if (L[(head + base + half - 1) & mask] < key) base += half;
        n -= half;
    }
    if (n == 1 && L[(head + base) & mask] < key) base++;
    return base;
}

// A sorted list of up to cap keys in a ring of mask + 1 LDS slots (file comment)
struct WideList {
    u64 *L;
    uint32_t mask, head, len;  // wave-uniform
    u64 last;                  // the largest key when the list holds cap keys, else FKEY_INVALID
    u64 front;                 // the smallest key, FKEY_INVALID when the list is empty

    __device__ __forceinline__ void init(u64 *ring, uint32_t ring_keys) {
        L = ring, mask = ring_keys - 1, head = 0, len = 0;
        last = front = FKEY_INVALID;
    }
    __device__ __forceinline__ u64 at(uint32_t i) const { return L[(head + i) & mask]; }
    __device__ __forceinline__ bool full(uint32_t cap) const { return len >= cap; }
    __device__ __forceinline__ void pop_front() {
        head = (head + 1) & mask;
        len--;
        last = FKEY_INVALID;
        front = len ? readlane64(at(0), 0) : FKEY_INVALID;
    }
    // Merge the keys `sk` of the lanes with `take` (ascending over the lanes, distinct and not in the list) and keep the
    // cap smallest; park: 64 keys of LDS
    __device__ __forceinline__ void merge(u64 sk, bool take, uint32_t cap, u64 *park, int lane) {
        const bool surv = take && (len < cap || sk < last);
        const u64 sm = __ballot(surv);
        if (sm == 0) return;
        const uint32_t m = (uint32_t)__popcll(sm);
        if (surv) park[__popcll(sm & ((1ull << lane) - 1))] = sk;
        wave_fence();
        const u64 nk = (uint32_t)lane < m ? park[lane] : FKEY_INVALID;
        const uint32_t pos = lds_lower_bound(L, head, mask, len, nk);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);  // (lane 0 holds the smallest new key)
        for (uint32_t hi = len; hi > first;) {
            const uint32_t lo = hi - first > 64 ? hi - 64 : first, idx = lo + lane;
            const bool act = idx < hi;
            const u64 e = act ? at(idx) : FKEY_INVALID;
            const uint32_t to = idx + lds_lower_bound(park, 0, 63, m, e);
            wave_fence();  // the piece is read before any of it is overwritten
            if (act && to < cap) L[(head + to) & mask] = e;
            hi = lo;
        }
        if ((uint32_t)lane < m && pos + lane < cap) L[(head + pos + lane) & mask] = nk;
        wave_fence();
        len = min(len + m, cap);
        last = len >= cap ? readlane64(at(cap - 1), 0) : FKEY_INVALID;
        const u64 nk0 = readlane64(nk, 0);
        front = nk0 < front ? nk0 : front;
    }
};

// ---------------------------------------------------------------------------------------------
// Graph path.  LDS: visited table (4 << lds_log2 bytes) | F's ring | R's ring (8 wide_ring_keys(ef') bytes each) |
// parked keys (64) | query | under a label range, the wave's range and row (HX_FILT_RANGE_LDS bytes).
// ---------------------------------------------------------------------------------------------
template <int KIND, int P, int DS>
__global__ void __launch_bounds__(64) hx_filt_wide_kernel(const DevView v, const FilterArgs a, const WideVisited w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t q = a.qsel ? a.qsel[w.q_base + blockIdx.x] : w.q_base + blockIdx.x;
    // the wave's filter, picked once as hx_filt_graph_kernel picks it: its row (a row the set does not have is the
    // query's own HNSW_ERR_ARG, under an id bound of 0), its label range (an empty one: bound 0), the deleted set's bound
    const uint32_t g = a.mask_of ? a.mask_of[q] : 0;
    const bool bad_row = a.mask_of && g != HNSW_MASK_NONE && g >= a.n_masks;
    const uint64_t *row = g == HNSW_MASK_NONE ? nullptr : a.allow + (size_t)g * a.mask_words;
    const uint64_t *allow = a.labels ? reinterpret_cast<const uint64_t *>((uintptr_t)a.labels | 1) : row;
    uint32_t lo = 0u, hi = 0u;
    if (a.labels) lo = a.range_lo[q], hi = a.range_hi[q];
    const uint64_t ids = g == HNSW_MASK_NONE ? a.none_bits : a.allow_bits;
    const uint32_t bound = bad_row || lo > hi ? 0u : (uint32_t)min(a.labels ? min(ids, a.label_len) : ids, (uint64_t)HX_EMPTY_SLOT);
    const uint32_t deny_n = a.deny ? (uint32_t)min(a.deny_bits, (uint64_t)HX_EMPTY_SLOT) : 0u;

    const uint32_t lds_log2 = w.lds_log2, hmask = (1u << lds_log2) - 1, ef = a.ef;
    uint32_t ring = 64;  // wide_ring_keys(ef)
    while (ring < ef) ring <<= 1;
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    u64 *ringF = reinterpret_cast<u64 *>(smem + (4ull << lds_log2));
    u64 *ringR = ringF + ring;
    u64 *park = ringR + ring;
    float *yq = reinterpret_cast<float *>(park + 64);
    uint32_t *range = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(yq) + query_lds_bytes(v));
    if (a.labels && lane == 0)  // (read after the wave_fence of the first clear_visited)
        *reinterpret_cast<uint4 *>(range) = make_uint4(lo, hi - lo, (uint32_t)(uintptr_t)row, (uint32_t)((uintptr_t)row >> 32));

    // the visited set's two levels
    const uint32_t lds_limit = filt_visited_limit(lds_log2);
    uint32_t *gtab = w.hbm ? w.hbm + ((size_t)blockIdx.x << w.hbm_log2) : nullptr;
    const uint32_t gmask = (1u << w.hbm_log2) - 1, gshift = gtab ? 32 - w.hbm_log2 : 0u;
    const uint32_t vis_limit = lds_limit + (gtab ? filt_visited_limit(w.hbm_log2) : 0u);
    bool spill = false;  // wave-uniform: the LDS level is closed (reset at every layer)
    bool dirty = false;  // the HBM level holds ids of an earlier layer

    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;  // lanes per candidate
    constexpr int CHUNK = 64 / LPC;                         // ids per pass
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;

    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0, n_vis = 0;
    int32_t status = stage_query<KIND>(v, a.Q + (size_t)q * v.dim, yq, lane) ? HNSW_OK : HNSW_ERR_NAN_INPUT;
    if (bad_row) status = HNSW_ERR_ARG;

    auto clear_visited = [&]() {
        for (uint32_t s = lane; s < (1u << (lds_log2 - 2)); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
        n_vis = 0;
        spill = false;
    };
    // true when id was absent (and is now present): the LDS level while it is open; once it is closed, an id it does
    // not hold is claimed in the HBM level, where the compare-and-swap is the probe
    auto visit = [&](uint32_t id) __attribute__((always_inline)) -> bool {
        if (!spill) return filt_visit(htab, lds_log2, id);
        if (visited_contains(htab, hmask, lds_log2, id)) return false;
        uint32_t s2 = ((id * 0x9E3779B1u) >> gshift) & gmask;
        while (true) {
            const uint32_t old = atomicCAS(gtab + s2, HX_EMPTY_SLOT, id);
            if (old == HX_EMPTY_SLOT) return true;
            if (old == id) return false;
            s2 = (s2 + 1) & gmask;
        }
    };
    // room for cnt more ids?  Closes the LDS level when they would take it past its limit (and empties the HBM level
    // when an earlier layer has used it): checked BEFORE the ids of a pass are inserted
    auto room = [&](uint32_t cnt) __attribute__((always_inline)) -> bool {
        if (gtab != nullptr && !spill && n_vis + cnt > lds_limit) {
            if (dirty) {
                for (uint32_t s2 = lane; s2 < ((gmask + 1) >> 2); s2 += 64)
                    reinterpret_cast<uint4 *>(gtab)[s2] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            spill = dirty = true;
        }
        return n_vis + cnt <= vis_limit;
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
    auto pass = [&](uint32_t nb, bool valid, auto &&body) __attribute__((always_inline)) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
        if (cnt == 0) return;
        sum_deg += cnt;
        if (!room(cnt)) {
            status = HNSW_ERR_OVERFLOW;
            return;
        }
        bool f = false;
        if (valid && h == 0) f = visit(nb);
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
        const uint32_t *adj;
        uint32_t S;
        if (layer == 0) {
            S = v.S0;
            adj = v.adj0 + (size_t)cid * S;
        } else {
            S = v.S1;
            const uint32_t ub = v.upper_base[cid];
            if (ub == HX_EMPTY_SLOT) {  // Graph::neighbors_vec -> NodeNotInGraph
                status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                return;
            }
            adj = v.adj_up + ((size_t)ub + layer - 1) * S;
        }
        n_exp++;
        uint32_t ovf = HX_EMPTY_SLOT;
        for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += CHUNK) {
            const uint32_t slot = c0 + cslot;
            const uint32_t nb = slot < S ? adj[slot] : HX_EMPTY_SLOT;
            const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
            const u64 pm = __ballot(is_ptr);
            if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
            pass(nb, nb != HX_EMPTY_SLOT && !is_ptr, body);
        }
        if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of the row
            const uint32_t o0 = v.ovf_off[ovf], o1 = v.ovf_off[ovf + 1];
            for (uint32_t base = o0; base < o1 && status == HNSW_OK; base += CHUNK) {
                const uint32_t i = base + cslot;
                pass(i < o1 ? v.ovf_nbrs[i] : HX_EMPTY_SLOT, i < o1, body);
            }
        }
    };

    WideList F, R;
    F.init(ringF, ring);
    R.init(ringR, ring);
    if (status == HNSW_OK) {
        // ---- entry point and the upper layers: the greedy ef = 1 walk, unfiltered ----
        const u64 ek = eval_key(v.ep, (uint32_t)lane < (uint32_t)LPC);
        u64 best = readlane64(ek, 0);
        n_dist = 1;
        if (best == FKEY_INVALID) status = HNSW_ERR_NAN_INPUT;
        for (int layer = (int)v.nb_layers - 1; layer >= 1 && status == HNSW_OK; layer--) {
            clear_visited();
            if (lane == 0) filt_visit(htab, lds_log2, (uint32_t)best);
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
            if (lane == 0) filt_visit(htab, lds_log2, (uint32_t)best);
            wave_fence();
            n_vis = 1;
            const u64 k0 = lane == 0 ? best : FKEY_INVALID;
            F.merge(k0, lane == 0, ef, park, lane);
            R.merge(k0, lane == 0 && filt_allowed(a.deny, deny_n, allow, bound, range, (uint32_t)best), ef, park, lane);
        }
        while (status == HNSW_OK && F.len > 0) {
            const u64 c = F.front;
            if (R.full(ef) && c > R.last) break;
            F.pop_front();
            expand((uint32_t)c, 0, [&](u64 key) {
                // admitted against the bound at the start of the pass; sorted once for both lists; R takes the allowed ones
                const bool adm = key != FKEY_INVALID && (!R.full(ef) || key < R.last);
                if (__ballot(adm) == 0) return;
                const u64 sk = wave_sort64(adm ? key : FKEY_INVALID, lane);
                const bool have = sk != FKEY_INVALID;
                const bool alw = have && filt_allowed(a.deny, deny_n, allow, bound, range, (uint32_t)sk);
                F.merge(sk, have, ef, park, lane);
                R.merge(sk, alw, ef, park, lane);
            });
        }
    }

    // ---- the first min(n, |R|) keys of R, streamed out of LDS 64 entries at a time, the pad behind them ----
    const uint32_t count = status == HNSW_OK ? min(a.n, R.len) : 0;
    for (uint32_t i = lane; i < a.n; i += 64) {
        const u64 k = i < count ? ringR[i] : FKEY_INVALID;
        a.out_ids[(size_t)q * a.n + i] = i < count ? (uint32_t)k : HX_EMPTY_SLOT;
        a.out_dists[(size_t)q * a.n + i] = i < count ? __builtin_bit_cast(float, (uint32_t)(k >> 32)) : __builtin_inff();
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
// Exact path, scan: block (seg, y) evaluates ids [HX_WIDE_SEG seg, ...) of the list against query y, sorts the keys in
// LDS and writes the first n of them (FKEY_INVALID behind the segment's own) to part[(y nseg + seg) n + i].
// LDS: keys (8 HX_WIDE_SEG bytes) | query.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(64) hx_filt_wide_scan_kernel(const DevView v, const FilterArgs a, const uint32_t *ids,
                                                               uint32_t A, uint32_t nseg, u64 *part, int32_t *part_status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *keys = reinterpret_cast<u64 *>(smem);
    float *yq = reinterpret_cast<float *>(keys + HX_WIDE_SEG);
    const int lane = threadIdx.x;
    const uint32_t seg = blockIdx.x, y = blockIdx.y;
    const size_t row = (size_t)y * nseg + seg;
    const uint32_t q = a.qsel ? a.qsel[y] : y;
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    bool bad = !stage_query<KIND>(v, a.Q + (size_t)q * v.dim, yq, lane);
    const uint32_t lo = min(A, (uint32_t)HX_WIDE_SEG * seg), hi = min(A, lo + (uint32_t)HX_WIDE_SEG), cnt = hi - lo;
    uint32_t p2 = 64;  // keys sorted: the power of two at or above the segment's
    while (p2 < cnt) p2 <<= 1;
    for (uint32_t i = cnt + lane; i < p2; i += 64) keys[i] = FKEY_INVALID;
    for (uint32_t base = lo; base < hi && !bad; base += CHUNK) {
        const uint32_t i = base + lane / LPC;
        const bool active = i < hi;
        const uint32_t id = active ? ids[i] : 0;
        const float dist = filt_dist<KIND, 0, 0>(v, id, active, h, yq);
        if (active && h == 0) {
            if (dist != dist)
                bad = true;
            else
                keys[i - lo] = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
        }
        bad = __ballot(bad) != 0;
    }
    wave_fence();
    if (!bad) {
        for (uint32_t k = 2; k <= p2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = lane; t < (p2 >> 1); t += 64) {  // compare-exchange (i, i + j), ascending where i & k == 0
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const u64 x = keys[i], z = keys[i + j];
                    if ((x > z) == ((i & k) == 0)) keys[i] = z, keys[i + j] = x;
                }
                wave_fence();
            }
        }
    }
    for (uint32_t i = lane; i < a.n; i += 64) part[row * a.n + i] = !bad && i < cnt ? keys[i] : FKEY_INVALID;
    if (lane == 0) part_status[row] = bad ? HNSW_ERR_NAN_INPUT : HNSW_OK;
}

// Merge: one wave per query folds its nseg runs (run s: the first min(n, segment s) keys of its row of part, ascending)
// pairwise: every key of the kept run finds its rank in the next run by binary search and the reverse (ids are distinct:
// no ties), and lands at the sum of its ranks when that is below n.  Three buffers of n keys rotate: kept, next, merged.
__global__ void __launch_bounds__(64) hx_filt_wide_merge_kernel(const FilterArgs a, uint32_t A, uint32_t nseg, const u64 *part,
                                                                const int32_t *part_status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t y = blockIdx.x, n = a.n;
    const uint32_t q = a.qsel ? a.qsel[y] : y;
    u64 *cur = reinterpret_cast<u64 *>(smem), *nxt = cur + n, *out = nxt + n;
    auto run_len = [&](uint32_t s) { return min(n, min(A, (uint32_t)HX_WIDE_SEG * (s + 1)) - min(A, (uint32_t)HX_WIDE_SEG * s)); };
    bool bad = false;
    uint32_t lc = 0;
    for (uint32_t s = 0; s < nseg; s++) {
        const size_t o = (size_t)y * nseg + s;
        bad |= part_status[o] != HNSW_OK;
        const uint32_t ln = run_len(s);
        u64 *dst = s == 0 ? cur : nxt;
        for (uint32_t i = lane; i < ln; i += 64) dst[i] = part[o * n + i];
        wave_fence();
        if (s == 0) {
            lc = ln;
            continue;
        }
        for (uint32_t i = lane; i < lc; i += 64) {
            const u64 k = cur[i];
            const uint32_t to = i + lds_lower_bound(nxt, 0, ~0u, ln, k);
            if (to < n) out[to] = k;
        }
        for (uint32_t i = lane; i < ln; i += 64) {
            const u64 k = nxt[i];
            const uint32_t to = i + lds_lower_bound(cur, 0, ~0u, lc, k);
            if (to < n) out[to] = k;
        }
        wave_fence();
        lc = min(lc + ln, n);
        u64 *t = cur;
        cur = out, out = t;
    }
    const uint32_t count = bad ? 0 : lc;
    for (uint32_t i = lane; i < n; i += 64) {
        const u64 k = i < count ? cur[i] : FKEY_INVALID;
        a.out_ids[(size_t)q * n + i] = i < count ? (uint32_t)k : HX_EMPTY_SLOT;
        a.out_dists[(size_t)q * n + i] = i < count ? __builtin_bit_cast(float, (uint32_t)(k >> 32)) : __builtin_inff();
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

template <int KIND, int P, int DS>
int launch_wide(const DevView &v, const FilterArgs &a, uint32_t nblocks, const WideVisited &vis, hipStream_t stream) {
    const size_t lds = (4ull << vis.lds_log2) + 2ull * wide_ring_keys(a.ef) * 8 + 64 * 8 + query_lds_bytes(v) +
                       filt_range_lds(a.labels != nullptr);
    return launch_checked({"wide filtered search kernel launch", "wide filtered search needs %zu bytes of LDS (> 160 KiB)"},
                          hx_filt_wide_kernel<KIND, P, DS>, dim3(nblocks), dim3(64), lds, stream, v, a, vis);
}

}  // namespace

int launch_filtered_wide_graph(const DevView &v, const FilterArgs &a, uint32_t nblocks, const WideVisited &vis,
                               hipStream_t stream) {
    if (nblocks == 0) return HNSW_OK;
    if (a.ef == 0 || a.ef > HX_WIDE_MAX_EF || a.n == 0 || a.n > a.ef || a.n_ranges > 1) {
        set_error("wide filtered search: needs 1 <= n <= ef' <= %d and at most one label range per query", HX_WIDE_MAX_EF);
        return HNSW_ERR_ARG;
    }
    if (vis.lds_log2 < HX_WIDE_LDS_LOG2_MIN || vis.lds_log2 > HX_WIDE_LDS_LOG2_MAX ||
        (vis.hbm && (vis.hbm_log2 < HX_WIDE_HBM_LOG2_MIN || vis.hbm_log2 > HX_WIDE_HBM_LOG2_MAX))) {
        set_error("wide filtered search: a visited set of 2^%u slots in LDS and 2^%u words in HBM", vis.lds_log2, vis.hbm_log2);
        return HNSW_ERR_ARG;
    }
    if (v.kind == HNSW_VEC_QUANT8) {
        if (v.dim == 100 && v.half_bytes == 64) return launch_wide<HNSW_VEC_QUANT8, 4, 100>(v, a, nblocks, vis, stream);
        return launch_wide<HNSW_VEC_QUANT8, 0, 0>(v, a, nblocks, vis, stream);
    }
    if (v.dim == 100 && v.row_stride == 400) return launch_wide<HNSW_VEC_F32, 25, 100>(v, a, nblocks, vis, stream);
    if (v.dim == 128 && v.row_stride == 512) return launch_wide<HNSW_VEC_F32, 32, 128>(v, a, nblocks, vis, stream);
    return launch_wide<HNSW_VEC_F32, 0, 0>(v, a, nblocks, vis, stream);
}

int launch_filtered_wide_exact(const DevView &v, const FilterArgs &a, uint32_t nsel, const uint32_t *ids, uint32_t A,
                               unsigned long long *part, int32_t *part_status, hipStream_t stream) {
    if (nsel == 0) return HNSW_OK;
    const uint32_t nseg = wide_exact_segments(A);
    if (a.n == 0 || a.n > HX_WIDE_MAX_N || nsel > 65535) {
        set_error("wide filtered exact search: needs 1 <= n <= %d and at most 65535 queries per launch", HX_WIDE_MAX_N);
        return HNSW_ERR_ARG;
    }
    // scan, then merge: two launches back to back under one message, the second only after the first was accepted
    const LaunchSite site{"wide filtered exact search launch", "wide filtered exact search needs %zu bytes of LDS (> 160 KiB)"};
    if (int rc = launch_checked(site, v.kind == HNSW_VEC_QUANT8 ? hx_filt_wide_scan_kernel<HNSW_VEC_QUANT8> : hx_filt_wide_scan_kernel<HNSW_VEC_F32>,
                                dim3(nseg, nsel), dim3(64), HX_WIDE_SEG * 8 + (size_t)query_lds_bytes(v), stream, v, a, ids, A, nseg,
                                part, part_status))
        return rc;
    return launch_checked(site, hx_filt_wide_merge_kernel, dim3(nsel), dim3(64), 3 * (size_t)a.n * 8, stream, a, A, nseg, part,
                          part_status);
}

}  // namespace hx
