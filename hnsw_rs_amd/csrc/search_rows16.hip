// search_rows16.hip -- the graph walk over an HNSW_VEC_F32 index whose snapshot keeps its rows as IEEE binary16 (option
// "rows_f16"): hx_search16_kernel, its launcher, and nothing else.  launch_search routes every view
// with v.rows16 set here; no other kernel may see such a view (the guard is ensure_uploaded, capi.cpp).
//
// The search is hx_search_kernel's (search_kernels.hip) over FullVec rows: ONE wave per query, one sorted list of <= ef
// keys with an expanded bit in registers (WaveList), the visited set an LDS table of four-slot buckets, two adjacency rows
// per pass on layer 0 (the candidate's and the runner-up's), a batch of neighbours merged by rank.  What is new is how a
// row reaches its sum (rows16.inc): half the bytes per row from HBM, widened exactly on the way into the reference's own
// f32 chain -- so ids, distance bits and traversal counters are those of the plain f32 index over the widened rows.
//
// Not here: the inline-rows loop (QUANT8 only), the lean kernels (the 100-d metric is a latency chain: halving the
// bytes buys little there), the second level of the visited set and the ef > 1024 spill kernel (refused by the launcher).
// The visited table is one level of LDS at every list width: ef 321 .. 1024 run two waves / one wave per CU.
//
// Built without packed-f32 instructions (Makefile): every operation below is the scalar IEEE one.

#include <algorithm>

#include "device_index.h"
#include "launch.h"
#include "search_common.h"

namespace hx {

#include "rows16.inc"

// bytes of the region the merge's permutation buffer shares with the gather's image + rank words (never live together:
// a distance pass ends before its merge starts)
template <int DS, int R>
__host__ __device__ constexpr uint32_t region16_bytes() {
    return coop_rows16<DS>() && 64u * R * 8u < HX_COOP_IMG_BYTES + 256u ? (uint32_t)HX_COOP_IMG_BYTES + 256u : 64u * R * 8u;
}

// DS: the dimension when the rows are gathered cooperatively (128, 256, 768), 0: a lane per row, any dimension
template <int DS, int R>
__global__ void __launch_bounds__(64)
hx_search16_kernel(const DevView v, const SearchArgs a, const uint32_t slots_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    const uint32_t hslots = 1u << slots_log2, hmask = hslots - 1;
    u64 *perm = reinterpret_cast<u64 *>(smem + 4ull * hslots);
    float *yq = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(perm) + region16_bytes<DS, R>());
    unsigned char *coop_img = reinterpret_cast<unsigned char *>(perm);
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(coop_img + HX_COOP_IMG_BYTES);
    const uint32_t vis_limit = hslots - (hslots >> 2);  // 75 % load at most
    const uint32_t np = v.row_stride >> 4;

    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0, n_vis = 0;
    int32_t status = HNSW_OK;
    if (!stage_query<HNSW_VEC_F32>(v, a.Q + (size_t)q * v.dim, yq, lane)) status = HNSW_ERR_NAN_INPUT;

    WaveList<R> wl;
#pragma unroll
    for (int r = 0; r < R; r++) wl.L[r] = KEY_INVALID;
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;

    // distance of one row per lane; every lane calls it (the gather is the whole wave's)
    auto eval_dist = [&](uint32_t id, bool active) __attribute__((always_inline)) -> float {
        float sm = 0.0f;
        if constexpr (coop_rows16<DS>()) {
            sm = f16_rows_coop<(DS > 0 ? DS : 64)>(v.rows, id, active, yq, coop_ids, coop_img, lane);
        } else if (active) {
            sm = f16_row_lane(v.rows + (size_t)id * v.row_stride, v.dim, np, yq);
        }
        return __builtin_sqrtf(sm);
    };
    // one pass over up to 64 ids, one per lane: visited filter, distances, merge
    auto process = [&](uint32_t id, bool valid, bool visit, uint32_t ef_l) __attribute__((always_inline)) {
        bool fresh = valid;
        if (visit) fresh = valid && visited_insert(htab, hmask, slots_log2, id);
        const u64 fm = __ballot(fresh);
        if (visit) n_vis += (uint32_t)__popcll(fm);
        if (fm == 0) return;
        n_dist += (uint32_t)__popcll(fm);
        const float dist = eval_dist(id, fresh);
        if (__ballot(fresh && dist != dist)) {
            status = HNSW_ERR_NAN_INPUT;  // Dist::cmp would panic (dist.rs:32)
            return;
        }
        wl.merge(fresh ? (((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id) : KEY_INVALID, ef_l, perm, lane);
    };
    // the ids of an overflow list (degree > S), 64 at a time
    auto process_overflow = [&](uint32_t ovf, uint32_t ef_l) __attribute__((always_inline)) {
        const uint32_t lo = v.ovf_off[ovf], hi = v.ovf_off[ovf + 1];
        for (uint32_t base = lo; base < hi && status == HNSW_OK; base += 64) {
            const uint32_t i = base + (uint32_t)lane;
            const bool ov = i < hi;
            const uint32_t onb = ov ? v.ovf_nbrs[i] : HX_EMPTY_SLOT;
            const uint32_t ocnt = (uint32_t)__popcll(__ballot(ov));
            sum_deg += ocnt;
            if (n_vis + ocnt > vis_limit) {
                status = HNSW_ERR_OVERFLOW;
                break;
            }
            process(onb, ov, true, ef_l);
        }
    };
    // pop the entry at cpos: mark it expanded, return its id
    auto take = [&](int cpos) __attribute__((always_inline)) -> uint32_t {
        uint32_t cid = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if ((cpos >> 6) == r) {
                cid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], cpos & 63);
                if (lane == (cpos & 63)) wl.L[r] |= KEY_EXPANDED;
            }
        }
        n_exp++;
        return cid;
    };

    if (status == HNSW_OK) {
        // ---- entry set: {ep} (template.rs:316-319) or the caller's ----
        const uint32_t n_entry = a.entries ? a.n_entry : 1;
        const uint32_t ef_first = max(1u, (a.layer_hi > a.layer_lo) ? a.ef_upper : a.ef_bottom);
        for (uint32_t base = 0; base < n_entry; base += 64) {
            const uint32_t i = base + (uint32_t)lane;
            const bool valid = i < n_entry;
            uint32_t id = 0;
            if (valid) id = a.entries ? a.entries[i] : v.ep;
            if (__ballot(valid && id >= v.n_points)) {
                status = HNSW_ERR_ARG;
                break;
            }
            process(id, valid, false, max(ef_first, n_entry));
        }
    }

    for (int layer = a.layer_hi; status == HNSW_OK && layer >= a.layer_lo; layer--) {
        const uint32_t ef_l = max(1u, layer > a.layer_lo ? a.ef_upper : a.ef_bottom);
        // visited.clear() (searcher.rs:101) / fresh Results: empty table
        for (uint32_t s = lane; s < (hslots >> 2); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
        // candidates = selected, visited = ids(selected)  (searcher.rs:32-33)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (64u * r + lane < wl.n_cur) {
                wl.L[r] &= KEY_MASK;
                visited_insert(htab, hmask, slots_log2, (uint32_t)wl.L[r]);
            }
        }
        n_vis = wl.n_cur;
        wl.refresh_last(ef_l);
        const uint32_t S = layer == 0 ? v.S0 : v.S1;

        if (layer == 0 && S <= 32 && !(a.flags & 1u)) {
            // ---- layer 0, rows of at most 32 slots: TWO adjacency rows per pass (hx_search_kernel's loop).  Lanes 0..31
            // take the row of the candidate c, lanes 32..63 the row of the runner-up p; one gather evaluates both -- up to
            // 64 wanted rows.  c is committed; if p is then still the smallest unexpanded entry it is committed from the
            // distances already in registers, otherwise they are dropped.  Nothing of p touches the visited set or the
            // list before its commit, and the commit filters against everything c inserted, so expansions, fresh sets,
            // counters and result are those of the one-at-a-time loop.
            int cpos = wl.first_unexpanded(lane);
            while (status == HNSW_OK && cpos >= 0) {
                const uint32_t cid = take(cpos);
                const int ppos = wl.first_unexpanded(lane);
                uint32_t pid = cid;
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (ppos >= 0 && (ppos >> 6) == r)
                        pid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], ppos & 63);
                const bool upper = lane >= 32;
                const uint32_t slot = (uint32_t)lane & 31u;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S && (!upper || ppos >= 0)) nb = v.adj0[(size_t)(upper ? pid : cid) * S + slot];
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                const u64 pm = __ballot(is_ptr);
                const bool spec_ok = ppos >= 0 && (pm >> 32) == 0;  // a runner-up row with an overflow list is not speculated on
                uint32_t ovf = HX_EMPTY_SLOT;
                if (pm & 0xFFFFFFFFull)
                    ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)(pm & 0xFFFFFFFFull)) - 1) & ~HX_OVF_FLAG;
                const u64 vmask = __ballot(valid);
                const uint32_t cnt_c = (uint32_t)__popcll(vmask & 0xFFFFFFFFull), cnt_p = (uint32_t)__popcll(vmask >> 32);
                sum_deg += cnt_c;
                if (n_vis + cnt_c > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                // c: filter now; p: a read-only look-up behind c's inserts (its own insert happens at its commit)
                bool want = false;
                if (valid && !upper) want = visited_insert(htab, hmask, slots_log2, nb);
                n_vis += (uint32_t)__popcll(__ballot(want && !upper));
                wave_fence();
                if (valid && upper && spec_ok) want = !visited_contains(htab, hmask, slots_log2, nb);
                n_dist += (uint32_t)__popcll(__ballot(want && !upper));
                float dist = 0.0f;
                if (__ballot(want)) dist = eval_dist(nb, want);
                const bool nan = want && dist != dist;
                if (__ballot(nan && !upper)) {
                    status = HNSW_ERR_NAN_INPUT;
                    break;
                }
                const u64 key = (want && !nan) ? (((u64)__builtin_bit_cast(uint32_t, dist) << 32) | nb) : KEY_INVALID;
                wl.merge(upper ? KEY_INVALID : key, ef_l, perm, lane);
                if (ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of c's row
                    process_overflow(ovf, ef_l);
                    if (status != HNSW_OK) break;
                }
                // ---- is p the next candidate?  then commit it from the registers
                const int npos = wl.first_unexpanded(lane);
                cpos = npos;
                if (npos < 0) break;
                if (!spec_ok) continue;
                uint32_t nid = 0;
#pragma unroll
                for (int r = 0; r < R; r++)
                    if ((npos >> 6) == r) nid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], npos & 63);
                if (nid != pid) continue;
                (void)take(npos);
                sum_deg += cnt_p;
                if (n_vis + cnt_p > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                // every valid neighbour of p goes through the filter now: one that c's commit inserted meanwhile is
                // dropped, one that was skipped above was in the set already
                bool fresh = false;
                if (valid && upper) fresh = visited_insert(htab, hmask, slots_log2, nb);
                const uint32_t nf = (uint32_t)__popcll(__ballot(fresh));
                n_vis += nf;
                n_dist += nf;
                if (__ballot(fresh && nan)) {
                    status = HNSW_ERR_NAN_INPUT;
                    break;
                }
                wl.merge((fresh && upper) ? key : KEY_INVALID, ef_l, perm, lane);
                cpos = wl.first_unexpanded(lane);
            }
            continue;
        }

        // ---- the upper layers (and layer-0 rows of more than 32 slots): one adjacency row per expansion
        while (status == HNSW_OK) {
            const int cpos = wl.first_unexpanded(lane);
            if (cpos < 0) break;  // candidates exhausted / only worse ones left
            const uint32_t cid = take(cpos);
            const uint32_t *row;
            if (layer == 0) {
                row = v.adj0 + (size_t)cid * S;
            } else {
                const uint32_t ub = v.upper_base[cid];
                if (ub == HX_EMPTY_SLOT) {  // Graph::neighbors_vec -> NodeNotInGraph
                    status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                    break;
                }
                row = v.adj_up + ((size_t)ub + layer - 1) * S;
            }
            uint32_t ovf = HX_EMPTY_SLOT;
            for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += 64) {
                const uint32_t slot = c0 + (uint32_t)lane;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S) nb = row[slot];
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                const u64 pm = __ballot(is_ptr);
                if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
                if (cnt == 0) continue;
                sum_deg += cnt;
                if (n_vis + cnt > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                process(nb, valid, true, ef_l);
            }
            if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) process_overflow(ovf, ef_l);
        }
    }

    // ---- get_top_selected(n) (results.rs:59-61): the first n of the ascending list ----
    const uint32_t count = status == HNSW_OK ? min(a.n, wl.n_cur) : 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t idx = 64u * r + lane;
        if (idx < a.n) {
            const bool have = idx < count;
            a.out_ids[(size_t)q * a.n + idx] = have ? (uint32_t)wl.L[r] : HX_EMPTY_SLOT;
            if (a.out_dists)
                a.out_dists[(size_t)q * a.n + idx] =
                    have ? __builtin_bit_cast(float, (uint32_t)((wl.L[r] & KEY_MASK) >> 32)) : __builtin_inff();
        }
    }
    for (uint32_t idx = 64u * R + lane; idx < a.n; idx += 64) {  // n > list capacity: padding
        a.out_ids[(size_t)q * a.n + idx] = HX_EMPTY_SLOT;
        if (a.out_dists) a.out_dists[(size_t)q * a.n + idx] = __builtin_inff();
    }
    if (lane == 0) {
        if (a.out_counts) a.out_counts[q] = count;
        hnsw_query_stats st;
        st.n_dist = n_dist;
        st.n_exp = n_exp;
        st.sum_deg = sum_deg;
        st.status = status;
        a.out_stats[q] = st;
    }
}

// ---------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------
template <int DS, int R>
static int launch16_one(const DevView &v, const SearchArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    const size_t lds = (4ull << slots_log2) + region16_bytes<DS, R>() + query_lds_bytes(v);
    return launch_checked({"search kernel launch (f16 rows)", "search over f16 rows needs %zu bytes of LDS (> 160 KiB)"},
                          hx_search16_kernel<DS, R>, dim3(nblocks), dim3(64), lds, stream, v, a, slots_log2);
}

template <int DS>
static int launch16_r(const DevView &v, const SearchArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream,
                      uint32_t ef_max) {
    if (ef_max <= 64) return launch16_one<DS, 1>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 128) return launch16_one<DS, 2>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 256) return launch16_one<DS, 4>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 64 * HX_MAX_R) return launch16_one<DS, HX_MAX_R>(v, a, nblocks, slots_log2, stream);
    // sixteen list registers: the any-dimension form only, as in launch_search
    return launch16_one<0, HX_MAX_R_WIDE>(v, a, nblocks, slots_log2, stream);
}

int launch_search_rows16(const DevView &v, const SearchArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream,
                         uint32_t ef_max) {
    if (v.kind != HNSW_VEC_F32 || !v.rows16 || v.row_stride != f16_row_stride(v.dim)) {
        set_error("search over f16 rows: the snapshot does not hold f16 rows");
        return HNSW_ERR_ARG;
    }
    if (ef_max > 64 * HX_MAX_R_WIDE) {
        set_error("ef = %u is above %d, the widest search available with rows_f16 yet", ef_max, 64 * HX_MAX_R_WIDE);
        return HNSW_ERR_ARG;
    }
    slots_log2 = std::min(std::max(slots_log2, 12u), 15u);  // one level of LDS (the limit of 160 KiB is launch_checked's)
    if (v.dim == 128) return launch16_r<128>(v, a, nblocks, slots_log2, stream, ef_max);
    if (v.dim == 256) return launch16_r<256>(v, a, nblocks, slots_log2, stream, ef_max);
    if (v.dim == 768) return launch16_r<768>(v, a, nblocks, slots_log2, stream, ef_max);
    return launch16_r<0>(v, a, nblocks, slots_log2, stream, ef_max);
}

}  // namespace hx
