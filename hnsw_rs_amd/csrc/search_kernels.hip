// search_kernels.hip -- the HNSW search hot path as hand-written HIP for gfx950 (MI355X, CDNA4).
//
// What runs here replaces, for a whole batch of queries at once,
//   HNSW::ann_by_vector          hnsw/src/template.rs:306-335
//   Searcher::search_layer       hnsw/src/template/searcher.rs:23-103
//   Results (ordered sets)       hnsw/src/template/results.rs:26-33,96-116,148-180
//   QuantVec::new / distance_unrolled   vectors/src/quant.rs:41-66,14-37
//   FullVec::distance            vectors/src/full.rs:23-29
//   Dist ordering                graph/src/dist.rs:30-38
// and returns bit-identical ids (and distances) for the same index and query.
//
// Execution model: ONE 64-lane wavefront per query (one single-wave workgroup), everything a
// query needs while it runs lives on chip:
//   - `selected` and `candidates` (two BTreeSets in the reference) collapse into ONE sorted list
//     of <= ef keys with an "expanded" bit: every element enters both sets together
//     (searcher.rs:79-80,86-87), leaves `candidates` only by being expanded, and an element
//     evicted from `selected` is > selected.last() forever, so popping it could only hit the
//     `break` (searcher.rs:41-44).  key = dist_bits << 32 | id orders exactly like Dist::cmp for
//     the non-negative, non-NaN distances a sqrt produces; bit 63 (never set by such a float) is
//     the expanded flag.  The list is held in registers (lane l, register r = list[64 r + l]) and
//     re-sorted through an LDS permutation buffer when a batch of neighbours is merged.
//   - `visited` (an IntSet, cleared per layer, searcher.rs:101) is an open-addressing hash table
//     in LDS filled with ds_cmpst (atomicCAS).
//   - the (dequantised) query is staged in LDS / registers once.
// Per expansion the wave loads one adjacency row (one coalesced 128-B load at m = 16), filters
// it through the visited table, gathers the vector rows of the fresh neighbours (QUANT8: a lane
// PAIR per neighbour, each lane streaming 4 of distance_unrolled's 8 running sums from its own
// contiguous half row; F32: one lane per neighbour because FullVec's sum is one sequential
// chain), and merges the batch into the list by rank (ballot + popcount), which is the
// reference's streaming top-ef (searcher.rs:74-94) evaluated for the whole batch at once: the
// final `selected` does not depend on the order in which a batch is applied.
//
// Float fidelity: compiled with -ffp-contract=off; no FMA may fuse `code * delta + min` or
// `acc += t * t`; sqrt and the quantiser's division are the correctly rounded forms hipcc emits
// by default.  Accumulation order is the reference's (quant.rs:23-36, full.rs:24-28).
//
// This file: hx_search_kernel, hx_search_spill_kernel (ef > 1024), their launchers and launch_search.  The wave
// primitives they share with the other kernel files are in search_common.h; the on-device build is build_kernels.hip,
// the exact scans are exact_scan.hip, the lean kernels search_lean.hip.

#include <cstdio>
#include <cstdlib>

#include "device_index.h"
#include "launch.h"
#include "search_common.h"
#include "stamps.h"
#include "switches.h"

namespace hx {

// bytes of the region the merge buffer shares with the cooperative gather's image (4 KiB + 64 rank words)
template <int KIND, int DS, int R>
__host__ __device__ constexpr uint32_t scratch_region_bytes() {
    return coop_rows<KIND, DS>() && 64u * R * 8u < HX_COOP_IMG_BYTES + 256u ? (uint32_t)HX_COOP_IMG_BYTES + 256u : 64u * R * 8u;
}

template <int KIND, int P, int DS, int R, bool FAT>
__global__ void __launch_bounds__(64)
hx_search_kernel(const DevView v, const SearchArgs a, const uint32_t slots_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    const uint32_t hslots = 1u << slots_log2, hmask = hslots - 1;
    u64 *perm = reinterpret_cast<u64 *>(smem + 4ull * hslots);
    // the merge's permutation buffer (64 R keys) and the cooperative gather's stage image + rank words are
    // never live together (a distance pass ends before its merge starts), so they share one region: with a
    // 32-KiB visited table the wave stays within a quarter of the CU's LDS for every list width up to 512
    constexpr uint32_t PERM_BYTES = scratch_region_bytes<KIND, DS, R>();
    float *yq = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(perm) + PERM_BYTES);
    // the visited set: an LDS table at 75 % load at most, and -- lists of eight / sixteen registers, round 4 -- a second
    // level in HBM for the ids beyond it, so that the table stays at 32 KiB and four waves per CU stay resident where a
    // 64- / 128-KiB table left two / one (the scheme of search_lean.hip's Visited::look2: the LDS level is CLOSED once it
    // holds its limit, later ids are claimed by one compare-and-swap in the HBM table, an id is in the set iff it is in
    // either level and is only inserted after both were found not to hold it)
    constexpr bool SPILLV = R >= 8;
    uint32_t lds_limit = hslots - (hslots >> 2);
    uint32_t *gtab = nullptr;
    uint32_t gmask = 0, gshift = 0;
    bool spill = false;  // wave-uniform: the LDS level is closed (reset at every layer)
    if (SPILLV && a.spill_tab != nullptr) {
        gtab = a.spill_tab + ((size_t)blockIdx.x << a.spill_log2);
        gmask = (1u << a.spill_log2) - 1;
        gshift = 32 - a.spill_log2;
        if (a.lds_limit != 0) lds_limit = min(lds_limit, max(128u, a.lds_limit));
    }
    const uint32_t vis_limit = lds_limit + (gtab != nullptr ? (gmask + 1) / 2 : 0u);
    // FAT: two 64 x 16 x P byte buffers for the prefetched block (after yq, 16-byte aligned)
    const uint32_t yq_bytes =  // == query_lds_bytes(v) (launch.h), KIND being v.kind: the launcher reserves that
        ((KIND == HNSW_VEC_QUANT8 ? 2u * (v.half_bytes - 8) * 4u : v.dim * 4u) + 15u) & ~15u;
    unsigned char *spec_buf = reinterpret_cast<unsigned char *>(yq) + yq_bytes;
    const uint32_t spec_lds = __builtin_amdgcn_groupstaticsize() + 4u * hslots + PERM_BYTES + yq_bytes;
    unsigned char *coop_img = reinterpret_cast<unsigned char *>(perm);
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(coop_img + HX_COOP_IMG_BYTES);

    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;  // lanes per candidate
    constexpr int CHUNK = 64 / LPC;                         // adjacency slots per pass
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;

    const uint32_t d = v.dim;
    const float *qv = a.Q + (size_t)q * d;
    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0;
    int32_t status = HNSW_OK;
    STAMP_STATE_GENERIC();

    // ---- stage the query (Point::new -> QuantVec::new for QUANT8, template.rs:313) ----
    const uint32_t nq_half = (KIND == HNSW_VEC_QUANT8) ? (v.half_bytes - 8) : 0;
    if (!stage_query<KIND>(v, qv, yq, lane)) status = HNSW_ERR_NAN_INPUT;

    // query values of this lane in registers when the dimension is a compile-time constant
    // (wide compile-time dimensions keep the query in LDS: 4 d / 8 registers would not fit)
    constexpr bool QREG = (KIND == HNSW_VEC_QUANT8 && DS > 0 && DS <= 160);
    constexpr int NQR = QREG ? (4 * (DS / 8) + DS % 8) : 1;
    QRegs<NQR> qreg;
    if (QREG) {
#pragma unroll
        for (int e = 0; e < NQR; e++) qreg.v[e] = yq[h * nq_half + e];
    }
    const QLds qlds{yq + h * nq_half};

    WaveList<R> wl;
#pragma unroll
    for (int r = 0; r < R; r++) wl.L[r] = KEY_INVALID;
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;

    // ---- distance of one candidate per lane group; returns the key on the group's first lane
    auto eval_dist = [&](uint32_t id, bool active, bool hidden_loads) __attribute__((always_inline)) -> float {
        float dist = 0.0f;
        if (KIND == HNSW_VEC_QUANT8 && P > 0) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (active) {
                const uint4 *src = reinterpret_cast<const uint4 *>(
                    v.rows + (size_t)id * v.row_stride + (size_t)h * v.half_bytes);
                uint4 w[P > 0 ? P : 1];
                if (FAT && hidden_loads) {
#pragma unroll
                    for (int p = 0; p < P; p++) w[p] = asm_ld128(src + p);
                } else {
#pragma unroll
                    for (int p = 0; p < P; p++) w[p] = src[p];
                    __builtin_amdgcn_sched_barrier(0);  // every piece requested before the arithmetic
                }
                if (QREG)
                    quant_half_sums<(P > 0 ? P : 1), DS>(w, qreg, h, v.nch4, v.rem, acc);
                else
                    quant_half_sums<(P > 0 ? P : 1), DS>(w, qlds, h, v.nch4, v.rem, acc);
            }
            // acc.iter().sum(): ((((((a0+a1)+a2)+a3)+a4)+a5)+a6)+a7 with a4..a7 on the odd lane
            const float b0 = pair_swap(acc[0]), b1 = pair_swap(acc[1]), b2 = pair_swap(acc[2]),
                        b3 = pair_swap(acc[3]);
            float s = 0.0f;
            s += acc[0];
            s += acc[1];
            s += acc[2];
            s += acc[3];
            s += b0;
            s += b1;
            s += b2;
            s += b3;
            dist = __builtin_sqrtf(s);
        } else if (KIND == HNSW_VEC_F32 && P > 0 && DS > 0) {
            float sm = 0.0f;
            if constexpr (coop_rows<KIND, DS>()) {
                // whole-line rows: eight lanes to a 128-byte line, owners sum out of an LDS image
                sm = f32_rows_coop<(DS > 0 ? DS : 32), HX_COOP_K>(v.rows, id, active, yq, coop_ids, coop_img, lane);
            } else if (active) {
                const uint4 *src = reinterpret_cast<const uint4 *>(v.rows + (size_t)id * v.row_stride);
                if constexpr (coop_rows<KIND, DS>()) {
                    // (never reached: the cooperative gather below runs outside the lane mask)
                } else if constexpr (P > 48) {
                    sm = f32_row_sum_staged<(DS > 0 ? DS : 1), HX_WIDE_CH, true>(src, yq);
                } else {
                    uint4 w[P > 0 ? P : 1];
#pragma unroll
                    for (int p = 0; p < P; p++) w[p] = src[p];
                    __builtin_amdgcn_sched_barrier(0);  // every piece requested before the chain starts
                    STAMP_ROWS_LANDED();
                    sm = f32_row_sum<(P > 0 ? P : 1), (DS > 0 ? DS : 1)>(w, yq);
                }
            }
            dist = __builtin_sqrtf(sm);
        } else {
            dist = dist_any_dim<KIND>(v, id, active, h, yq);
        }
        return dist;
    };
    auto eval_key = [&](uint32_t id, bool active, bool hidden_loads) -> u64 {
        const float dist = eval_dist(id, active, hidden_loads);
        const bool first = (LPC == 1) || (h == 0);
        if (!(active && first)) return KEY_INVALID;
        if (dist != dist) {
            status = HNSW_ERR_NAN_INPUT;  // Dist::cmp would panic (dist.rs:32)
            return KEY_INVALID;
        }
        return ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
    };

    // ---- one pass over up to CHUNK neighbour ids (one per lane group) ----
    // entries the visited table holds (exact: the overflow check adds the row's worst case before a pass)
    uint32_t n_vis = 0;
    // IntSet::insert / contains over both levels (true = id was absent / is present)
    auto vins = [&](uint32_t id) __attribute__((always_inline)) -> bool {
        if constexpr (SPILLV) {
            if (spill) {
                if (visited_contains(htab, hmask, slots_log2, id)) return false;
                uint32_t s2 = ((id * 0x9E3779B1u) >> gshift) & gmask;
                while (true) {  // the compare-and-swap is the probe: it returns what the slot holds
                    const uint32_t old = atomicCAS(gtab + s2, HX_EMPTY_SLOT, id);
                    if (old == HX_EMPTY_SLOT) return true;
                    if (old == id) return false;
                    s2 = (s2 + 1) & gmask;
                }
            }
        }
        return visited_insert(htab, hmask, slots_log2, id);
    };
    auto vhas = [&](uint32_t id) __attribute__((always_inline)) -> bool {
        if (visited_contains(htab, hmask, slots_log2, id)) return true;
        if constexpr (SPILLV) {
            if (spill) {
                uint32_t s2 = ((id * 0x9E3779B1u) >> gshift) & gmask;
                while (true) {
                    const uint32_t cur = __hip_atomic_load(gtab + s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == id) return true;
                    if (cur == HX_EMPTY_SLOT) return false;
                    s2 = (s2 + 1) & gmask;
                }
            }
        }
        return false;
    };
    // room for cnt more ids?  Closes the LDS level (and empties the HBM one) when they would take it past its limit:
    // checked BEFORE every chunk of ids is inserted, so the LDS table never holds more than its limit
    auto room = [&](uint32_t cnt) __attribute__((always_inline)) -> bool {
        if constexpr (SPILLV) {
            if (gtab != nullptr && !spill && n_vis + cnt > lds_limit) {
                for (uint32_t s2 = lane; s2 < ((gmask + 1) >> 2); s2 += 64)
                    reinterpret_cast<uint4 *>(gtab)[s2] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                spill = true;
            }
        }
        return n_vis + cnt <= vis_limit;
    };
    auto process = [&](uint32_t id, bool valid, bool visit, uint32_t ef_l, bool hidden_loads = false) {
        bool fresh = valid;
        if (visit) {
            bool f = false;
            if (valid && h == 0) f = vins(id);
            if (LPC == 2) f = (pair_swap_i(f ? 1 : 0) | (f ? 1 : 0)) != 0;
            fresh = f;
        }
        const u64 fm = __ballot(fresh && h == 0);
        if (visit) n_vis += (uint32_t)__popcll(fm);
        if (fm == 0) return;
        n_dist += (uint32_t)__popcll(fm);
        u64 key = eval_key(id, fresh, hidden_loads);
        if (__ballot(status != HNSW_OK)) status = HNSW_ERR_NAN_INPUT;
        wl.merge(key, ef_l, perm, lane);
    };

    if (status == HNSW_OK) {
        // ---- entry set: {ep} (template.rs:316-319) or the caller's (search_layer seam) ----
        const uint32_t n_entry = a.entries ? a.n_entry : 1;
        const uint32_t ef_first = max(1u, (a.layer_hi > a.layer_lo) ? a.ef_upper : a.ef_bottom);
        for (uint32_t base = 0; base < n_entry; base += CHUNK) {
            const uint32_t i = base + cslot;
            const bool valid = i < n_entry;
            uint32_t id = 0;
            if (valid) id = a.entries ? a.entries[i] : v.ep;
            if (__ballot(valid && id >= v.n_points)) {
                status = HNSW_ERR_ARG;
                break;
            }
            // the reference keeps every entry it is given; an entry set larger than ef is
            // rejected by the host side
            process(id, valid, false, max(ef_first, n_entry));
        }
    }

    for (int layer = a.layer_hi; status == HNSW_OK && layer >= a.layer_lo; layer--) {
        const uint32_t ef_l = max(1u, layer > a.layer_lo ? a.ef_upper : a.ef_bottom);
        // visited.clear() (searcher.rs:101) / fresh Results: empty table
        for (uint32_t s = lane; s < (hslots >> 2); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] =
                make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
        n_vis = 0;
        spill = false;  // an empty LDS table: open again
        // candidates ∪= selected, visited ∪= ids(selected)  (searcher.rs:32-33)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            if (idx < wl.n_cur) {
                wl.L[r] &= KEY_MASK;
                vins((uint32_t)wl.L[r]);
            }
        }
        n_vis = wl.n_cur;
        wl.refresh_last(ef_l);
        const uint32_t S = layer == 0 ? v.S0 : v.S1;

        if (FAT && layer == 0) {
            // ---- layer 0 over the inline-rows blocks: ONE dependent, coalesced read per expansion
            // (the 32 neighbour rows of the candidate, ids embedded), and the block of the PREDICTED
            // next candidate -- the smallest unexpanded entry once the current one is marked -- is
            // already in flight while the current block is filtered, evaluated and merged.  The
            // prediction is a prefetch only: what is evaluated and merged, and in which order, is
            // exactly what the loop below does on the compact layout.
            constexpr int PP = P > 0 ? P : 1;
            constexpr uint32_t BLK = 1024u * PP;  // bytes of one block image in LDS
            uint4 w[PP];
            bool have_spec = false;
            uint32_t spec_id = 0, spec_sel = 0;
            const size_t lane_off = (size_t)cslot * v.row_stride + (size_t)h * v.half_bytes;
            // The hot loop below holds no compiler-visible VMEM load: hipcc drains vmcnt(0) at the
            // header of any loop with such a load somewhere inside, which would also drain the
            // prefetch.  The rare degree > 32 rows leave the hot loop, are served from the compact
            // layout with plain loads, and re-enter it.
            uint32_t ovf_pending = HX_EMPTY_SLOT;
            bool done = false;
            while (!done && status == HNSW_OK) {
            while (true) {
                STAMP_RAW(t0);
                const int cpos = wl.first_unexpanded(lane);
                if (cpos < 0) {
                    done = true;
                    break;
                }
                uint32_t cid = 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if ((cpos >> 6) == r) {
                        cid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], cpos & 63);
                        if (lane == (cpos & 63)) wl.L[r] |= KEY_EXPANDED;
                    }
                }
                n_exp++;
                STAMP_NOTE_HIT(have_spec && spec_id == cid);
                // Every block is staged through LDS by DMA (no compiler-visible VMEM load in this
                // loop, so hipcc inserts no vmcnt wait that would also drain the prefetch): the
                // current block is either the image prefetched one expansion ago or is fetched now;
                // then the predicted next block is started into the other buffer.
                const bool hit = have_spec && spec_id == cid;
                uint32_t cur_sel = spec_sel;
                if (!hit) {
                    cur_sel = spec_sel ^ 1u;  // a stale prefetch may still be landing in spec_sel
                    const unsigned char *src = v.fat + (size_t)cid * v.fat_stride + lane_off;
#pragma unroll
                    for (int p = 0; p < PP; p++)
                        dma_piece_to_lds(src + 16 * p, spec_lds + cur_sel * BLK + 1024u * p);
                }
                have_spec = false;
                {
                    const int ppos = wl.first_unexpanded(lane);
                    if (ppos >= 0) {
                        uint32_t pid = 0;
#pragma unroll
                        for (int r = 0; r < R; r++)
                            if ((ppos >> 6) == r)
                                pid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], ppos & 63);
                        spec_sel = cur_sel ^ 1u;
                        const unsigned char *src = v.fat + (size_t)pid * v.fat_stride + lane_off;
#pragma unroll
                        for (int p = 0; p < PP; p++)
                            dma_piece_to_lds(src + 16 * p, spec_lds + spec_sel * BLK + 1024u * p);
                        spec_id = pid;
                        have_spec = true;
                    }
                }
                // the current block has landed once all but the PP youngest DMA pieces are done
                if (have_spec)
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PP) : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                {
                    const uint4 *img = reinterpret_cast<const uint4 *>(spec_buf + cur_sel * BLK) + lane;
#pragma unroll
                    for (int p = 0; p < PP; p++) w[p] = img[64 * p];
                }
                STAMP_RAW(t1);
                STAMP_ADD(FAT_PICK, t0, t1);
                // the neighbour id travels in the last 4 bytes of half 0
                const uint32_t raw = w[PP - 1].w;
                const uint32_t nb = h ? (uint32_t)pair_swap_i((int)raw) : raw;
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                uint32_t ovf = HX_EMPTY_SLOT;
                const u64 pm = __ballot(is_ptr);
                if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
                if (cnt != 0) {
                    sum_deg += cnt;
                    if (!room(cnt)) {
                        status = HNSW_ERR_OVERFLOW;
                        break;
                    }
                    bool f = false;
                    if (valid && h == 0) f = vins(nb);
                    const bool fresh = (pair_swap_i(f ? 1 : 0) | (f ? 1 : 0)) != 0;
                    const u64 fm = __ballot(fresh && h == 0);
                    n_vis += (uint32_t)__popcll(fm);  // what the table really holds
                    STAMP_RAW(t2);
                    STAMP_ADD_BY_HIT(FAT_FILTER_HIT, FAT_FILTER_MISS, t1, t2);
                    if (fm != 0) {
                        n_dist += (uint32_t)__popcll(fm);
                        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (fresh) {
                            if (DS > 0)
                                quant_half_sums<PP, DS>(w, qreg, h, v.nch4, v.rem, acc);
                            else
                                quant_half_sums<PP, 0>(w, qlds, h, v.nch4, v.rem, acc);
                        }
                        const float b0 = pair_swap(acc[0]), b1 = pair_swap(acc[1]),
                                    b2 = pair_swap(acc[2]), b3 = pair_swap(acc[3]);
                        float s = 0.0f;
                        s += acc[0];
                        s += acc[1];
                        s += acc[2];
                        s += acc[3];
                        s += b0;
                        s += b1;
                        s += b2;
                        s += b3;
                        const float dist = __builtin_sqrtf(s);
                        u64 key = KEY_INVALID;
                        bool nan = false;
                        if (fresh && h == 0) {
                            nan = dist != dist;
                            if (!nan) key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | nb;
                        }
                        if (__ballot(nan)) {
                            status = HNSW_ERR_NAN_INPUT;
                            break;
                        }
                        STAMP_RAW(t3);
                        STAMP_ADD(FAT_CHAIN, t2, t3);
                        wl.merge(key, ef_l, perm, lane);
                        STAMP_RAW(t4);
                        STAMP_ADD(FAT_MERGE, t3, t4);
                    }
                }
                if (ovf != HX_EMPTY_SLOT) {
                    ovf_pending = ovf;
                    break;
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no prefetch in flight outside the hot loop
            have_spec = false;
            if (done || status != HNSW_OK) break;
            {  // degree > S0: the rest of the row, from the compact rows
                const uint32_t ovf = ovf_pending;
                ovf_pending = HX_EMPTY_SLOT;
                {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)asm_ld32(v.ovf_off + ovf));
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)asm_ld32(v.ovf_off + ovf + 1));
                    for (uint32_t base = lo; base < hi; base += CHUNK) {
                        const uint32_t i = base + cslot;
                        const bool ov = i < hi;
                        const uint32_t onb = ov ? asm_ld32(v.ovf_nbrs + i) : HX_EMPTY_SLOT;
                        const uint32_t ocnt = (uint32_t)__popcll(__ballot(ov && h == 0));
                        sum_deg += ocnt;
                        if (!room(ocnt)) {
                            status = HNSW_ERR_OVERFLOW;
                            break;
                        }
                        process(onb, ov, true, ef_l, true);
                        if (status != HNSW_OK) break;
                    }
                }
            }
            }
            continue;
        }

        if (KIND == HNSW_VEC_F32 && !FAT && layer == 0 && S <= 32 && !(a.flags & 1u)) {
            // ---- layer 0, one lane per neighbour, rows of at most 32 slots: TWO rows per pass.
            // Lanes 0..31 take the row of the candidate c being expanded, lanes 32..63 the row of the
            // runner-up p (the smallest unexpanded entry once c is marked).  Both adjacency rows and
            // both sets of vector rows are fetched together, one pass evaluates all of them.  c is
            // committed (visited insert, merge); if p is then still the smallest unexpanded entry --
            // measured: 2 times out of 3 -- it is committed from the distances already in registers,
            // i.e. that expansion costs no memory round trip and no distance pass.  Otherwise p's
            // results are dropped.  Nothing of p touches the visited set or the list before its
            // commit, and the commit filters against everything c inserted, so the expanded nodes,
            // the fresh sets, the counters and the result are those of the one-at-a-time loop.
            int cpos = wl.first_unexpanded(lane);  // carried: the pick after a merge is the next c
            while (status == HNSW_OK) {
                if (cpos < 0) break;
                STAMP_RAW(f0);
                uint32_t cid = 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if ((cpos >> 6) == r) {
                        cid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], cpos & 63);
                        if (lane == (cpos & 63)) wl.L[r] |= KEY_EXPANDED;
                    }
                }
                n_exp++;
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
                STAMP_WAIT_VMEM();
                STAMP_RAW(f1);
                STAMP_ADD(GENERIC_PICK, f0, f1);
                STAMP_COUNT(GENERIC_PASSES);
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                const u64 pm = __ballot(is_ptr);
                // a runner-up row with an overflow pointer is not speculated on
                const bool spec_ok = ppos >= 0 && (pm >> 32) == 0;
                uint32_t ovf = HX_EMPTY_SLOT;
                if (pm & 0xFFFFFFFFull)
                    ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)(pm & 0xFFFFFFFFull)) - 1) &
                          ~HX_OVF_FLAG;
                // ---- c: filter now; p: read-only look-up (its insert happens at its commit)
                const u64 vmask = __ballot(valid);
                const uint32_t cnt_c = (uint32_t)__popcll(vmask & 0xFFFFFFFFull);
                const uint32_t cnt_p = (uint32_t)__popcll(vmask >> 32);
                sum_deg += cnt_c;
                if (!room(cnt_c)) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                bool want = false;
                if (valid && !upper) want = vins(nb);
                n_vis += (uint32_t)__popcll(__ballot(want && !upper));  // what the table really holds
                // (the look-up runs after the inserts of this pass: what c just claimed is skipped)
                wave_fence();
                if (valid && upper && spec_ok) want = !vhas(nb);
                n_dist += (uint32_t)__popcll(__ballot(want && !upper));
                STAMP_RAW(f2);
                STAMP_ADD(GENERIC_FILTER, f1, f2);
                STAMP_ROWS_LANDED_DEFAULT(f2);
                float dist = 0.0f;
                if (__ballot(want)) dist = eval_dist(nb, want, false);
                STAMP_RAW(f3);
                STAMP_ADD_AROUND_ROWS_LANDED(GENERIC_ROW_WAIT, GENERIC_CHAIN, f2, f3);
                const bool nan = want && dist != dist;
                if (__ballot(nan && !upper)) {
                    status = HNSW_ERR_NAN_INPUT;
                    break;
                }
                const u64 key = (want && !nan) ? (((u64)__builtin_bit_cast(uint32_t, dist) << 32) | nb) : KEY_INVALID;
                wl.merge(upper ? KEY_INVALID : key, ef_l, perm, lane);
                if (ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of c's row
                    const uint32_t lo = v.ovf_off[ovf], hi = v.ovf_off[ovf + 1];
                    for (uint32_t base = lo; base < hi; base += CHUNK) {
                        const uint32_t i = base + cslot;
                        const bool ov = i < hi;
                        const uint32_t onb = ov ? v.ovf_nbrs[i] : HX_EMPTY_SLOT;
                        const uint32_t ocnt = (uint32_t)__popcll(__ballot(ov && h == 0));
                        sum_deg += ocnt;
                        if (!room(ocnt)) {
                            status = HNSW_ERR_OVERFLOW;
                            break;
                        }
                        process(onb, ov, true, ef_l);
                        if (status != HNSW_OK) break;
                    }
                    if (status != HNSW_OK) break;
                }
                // ---- is p the next candidate?  then commit it from the registers
                STAMP_RAW(f4);
                STAMP_ADD(GENERIC_MERGE_C, f3, f4);
                const int npos = wl.first_unexpanded(lane);
                cpos = npos;
                if (npos < 0) break;
                if (!spec_ok) continue;
                uint32_t nid = 0;
#pragma unroll
                for (int r = 0; r < R; r++)
                    if ((npos >> 6) == r)
                        nid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], npos & 63);
                if (nid != pid) continue;
#pragma unroll
                for (int r = 0; r < R; r++)
                    if ((npos >> 6) == r && lane == (npos & 63)) wl.L[r] |= KEY_EXPANDED;
                n_exp++;
                sum_deg += cnt_p;
                if (!room(cnt_p)) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                // every valid neighbour of p goes through the filter now: one that c's commit inserted
                // meanwhile is dropped, one that was skipped above was in the set already
                bool fresh = false;
                if (valid && upper) fresh = vins(nb);
                n_vis += (uint32_t)__popcll(__ballot(fresh));
                n_dist += (uint32_t)__popcll(__ballot(fresh));
                if (__ballot(fresh && nan)) {
                    status = HNSW_ERR_NAN_INPUT;
                    break;
                }
                wl.merge((fresh && upper) ? key : KEY_INVALID, ef_l, perm, lane);
                cpos = wl.first_unexpanded(lane);
                STAMP_RAW(f5);
                STAMP_ADD(GENERIC_COMMIT_P, f4, f5);
            }
            continue;
        }

        while (true) {
            const int cpos = wl.first_unexpanded(lane);
            if (cpos < 0) break;  // candidates exhausted / only worse ones left
            // pop it: mark expanded, fetch its id
            uint32_t cid = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((cpos >> 6) == r) {
                    cid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], cpos & 63);
                    if (lane == (cpos & 63)) wl.L[r] |= KEY_EXPANDED;
                }
            }
            n_exp++;
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
            for (uint32_t c0 = 0; c0 < S; c0 += CHUNK) {
                const uint32_t slot = c0 + cslot;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S) nb = row[slot];
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                const u64 pm = __ballot(is_ptr);
                if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
                if (cnt == 0) continue;
                sum_deg += cnt;
                if (!room(cnt)) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                process(nb, valid, true, ef_l);
                if (status != HNSW_OK) break;
            }
            if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of the row
                const uint32_t lo = v.ovf_off[ovf], hi = v.ovf_off[ovf + 1];
                for (uint32_t base = lo; base < hi; base += CHUNK) {
                    const uint32_t i = base + cslot;
                    const bool valid = i < hi;
                    const uint32_t nb = valid ? v.ovf_nbrs[i] : HX_EMPTY_SLOT;
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
                    sum_deg += cnt;
                    if (!room(cnt)) {
                        status = HNSW_ERR_OVERFLOW;
                        break;
                    }
                    process(nb, valid, true, ef_l);
                    if (status != HNSW_OK) break;
                }
            }
            if (status != HNSW_OK) break;
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
                    have ? __builtin_bit_cast(float, (uint32_t)((wl.L[r] & KEY_MASK) >> 32))
                         : __builtin_inff();
        }
    }
    for (uint32_t idx = 64u * R + lane; idx < a.n; idx += 64) {  // n > list capacity: padding
        a.out_ids[(size_t)q * a.n + idx] = HX_EMPTY_SLOT;
        if (a.out_dists) a.out_dists[(size_t)q * a.n + idx] = __builtin_inff();
    }
    STAMP_WRITE_GENERIC();
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
// launchers
// ---------------------------------------------------------------------------------------------

// Visited-table size for a search with list size ef on rows of up to s0 neighbours.  The table holds
// every id whose distance is computed in one layer; measured on 10240 queries of the 1M x 100d index
// (32-slot rows): efSearch 64 mean 1190 / max 1769, 96: 1593 / 2235, 128: 1966 / 2810, 288: 3593 / 5599
// (scripts/nvis_probe.py).  The limit (75 % of the slots) stays >= 1.1 x the observed maximum plus one
// row.  Too small is safe (status OVERFLOW; the host-pointer API retries with the next size), too
// large costs occupancy: 64 KiB tables leave 2 waves per CU, i.e. a 1024-query launch no longer fits
// the chip in one round.
uint32_t default_slots_log2(uint32_t ef, uint32_t s0) {
    const uint64_t e = (uint64_t)ef * std::max(s0, 8u) / 32u;  // ef in units of 32-slot rows
    if (e <= 112) return 12;  // 4096 slots, 16 KiB: limit 3072
    // 8192 slots, 32 KiB: limit 6144.  Up to ef 320: a search visits ~ 11 ef + 500 ids on average and up to 1.4 x that
    // (1M x 100d: 3.7 k at ef 300, no query of 8192 fills the table; at 384 one in twenty does and would run again with
    // the next size), and four waves per CU -- a whole batch of 1024 at once -- need the table to stay at 32 KiB
    // (ef 300, batch 1024: 0.86 ms against 1.50 ms with 64 KiB)
    if (e <= 320) return 13;
    if (e <= 576) return 14;  // 64 KiB: limit 12288
    if (ef <= 64 * HX_MAX_R_WIDE) return 15;  // 128 KiB
    // the HBM-resident table of hx_search_spill_kernel (limit: one half): about 30 visited ids per list entry
    uint32_t l = 16;
    while (l < 30 && (1ull << l) < 64ull * e) l++;
    return l;
}
uint32_t default_slots_log2(uint32_t ef) { return default_slots_log2(ef, 32); }
uint32_t max_slots_log2(uint32_t ef) { return ef <= 64 * HX_MAX_R_WIDE ? 15 : 31; }  // (the spill kernel caps its table at 4 N slots)

template <int KIND, int P, int DS, int R, bool FAT>
static int launch_one(const DevView &v, const SearchArgs &a_in, uint32_t nblocks, uint32_t slots_log2,
                      hipStream_t stream) {
    SearchArgs a = a_in;
    // lists of eight / sixteen registers (ef > 320 asks for a 64- / 128-KiB table): 32 KiB of LDS + a second level in
    // HBM (stream-ordered scratch), see the kernel
    VisitedSpill sp(R >= 8 && slots_log2 >= 14 && a.spill_tab == nullptr, a, slots_log2, nblocks, stream);
    size_t lds = (4ull << slots_log2) + scratch_region_bytes<KIND, DS, R>() + query_lds_bytes(v);
    if (FAT) lds += 2ull * 1024 * (P > 0 ? P : 1);
    return launch_checked({"search kernel launch", "search needs %zu bytes of LDS (> 160 KiB)"},
                          hx_search_kernel<KIND, P, DS, R, FAT>, dim3(nblocks), dim3(64), lds, stream, v, a, slots_log2);
}

template <int KIND, int P, int DS>
static int launch_r(const DevView &v, const SearchArgs &a, uint32_t nblocks, uint32_t slots_log2,
                    hipStream_t stream, uint32_t ef_max) {
    // the inline-rows variant needs one pass to cover a whole layer-0 row
    // (block images of rows wider than 5 pieces per half would not leave 4 waves per CU: not built)
    constexpr bool CAN_FAT = (KIND == HNSW_VEC_QUANT8 && P > 0 && P <= 5);
    // the inline-rows loop stages two block images in LDS; it is used while a wave still needs no more
    // than a quarter of the CU's LDS, so that 1024 waves fit the chip in one round
    const uint32_t r_list = ef_max <= 64 ? 1 : ef_max <= 128 ? 2 : ef_max <= 256 ? 4 : 8;
    const size_t fat_lds = (4ull << slots_log2) + 64ull * r_list * 8 + 2ull * 1024 * (P > 0 ? P : 1) + 1024;
    // ... and only while the launch is small enough to be latency-bound: with more than four waves per CU
    // the compact layout wins (measured, 1M x 100d quant8, efSearch 68: 2048 queries 0.359 ms inline
    // rows vs 0.256 ms compact; 32768 queries 8.4 vs 10.6 M q/s) -- the block images halve the
    // resident waves and every slot of a block is read whether it is needed or not
    // (every caller's table has at least default_slots_log2(ef_max) slots -- 2^13 above ef 112 at S0 = 32 -- so
    // fat_lds fits at four list registers only for P <= 2 and at eight only for P = 1: the others are not built)
    constexpr bool FAT4 = CAN_FAT && P <= 2, FAT8 = CAN_FAT && P <= 1;
    if (CAN_FAT && v.fat != nullptr && v.S0 == 32 && a.layer_lo == 0 && fat_lds <= 40 * 1024 &&
        nblocks <= 4 * cu_count()) {
        if (ef_max <= 64) return launch_one<KIND, P, DS, 1, CAN_FAT>(v, a, nblocks, slots_log2, stream);
        if (ef_max <= 128) return launch_one<KIND, P, DS, 2, CAN_FAT>(v, a, nblocks, slots_log2, stream);
        if (ef_max <= 256) {
            if constexpr (FAT4) return launch_one<KIND, P, DS, 4, true>(v, a, nblocks, slots_log2, stream);
        } else if (ef_max <= 512) {
            if constexpr (FAT8) return launch_one<KIND, P, DS, 8, true>(v, a, nblocks, slots_log2, stream);
        }
    }
    if (ef_max <= 64) return launch_one<KIND, P, DS, 1, false>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 128) return launch_one<KIND, P, DS, 2, false>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 256) return launch_one<KIND, P, DS, 4, false>(v, a, nblocks, slots_log2, stream);
    if (ef_max <= 512) return launch_one<KIND, P, DS, 8, false>(v, a, nblocks, slots_log2, stream);
    set_error("ef = %u is above the supported maximum of %d", ef_max, 64 * HX_MAX_R);
    return HNSW_ERR_ARG;
}


// =============================================================================================
// ef beyond what a wave's registers hold (> 1024).  The reference's ann_by_vector has no limit on ef
// (template.rs:306-311: `selected` is a BTreeSet); the register-resident list of the kernels above stops
// at sixteen registers per lane.  This kernel keeps the SAME single sorted list (key = dist_bits << 32 |
// id, bit 63 = expanded) and the visited set in HBM scratch instead, one wave per query, and applies a
// batch of neighbour distances the way the reference literally does -- one element at a time
// (searcher.rs:74-94): position by a wave-wide count, the tail moved up by one from the top, the element
// stored.  Slow (every insertion is a few dependent HBM round trips) but exact and without a limit other
// than memory: the list holds ef entries of 8 bytes, the table a power of two of slots that the host
// doubles and re-runs when a query fills it to one half (HNSW_ERR_OVERFLOW), which ends at 4 N slots.
// List and table are read and written through L2 (agent-scope relaxed atomics: the lanes of the wave
// hand entries to each other through memory, and the table's compare-and-swap executes there).
// =============================================================================================
struct SpillScratch {
    u64 *lists;        // nblocks x list_cap
    uint32_t *tabs;    // nblocks << tab_log2
    uint32_t list_cap;
    uint32_t tab_log2;
    uint32_t q_first;  // launch block b serves query (selection entry) q_first + b
};

__device__ __forceinline__ uint32_t spill_ld(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 spill_ld(const u64 *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void spill_st(u64 *p, u64 x) {
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void spill_st(uint32_t *p, uint32_t x) {
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a wave's own stores have reached L2 before its next loads are issued
__device__ __forceinline__ void spill_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// IntSet::insert on the HBM table (linear probing, load <= 1/2): true when id was absent
__device__ __forceinline__ bool spill_visited_insert(uint32_t *tab, uint32_t mask, uint32_t shift, uint32_t id) {
    uint32_t s = ((id * 0x9E3779B1u) >> shift) & mask;
    while (true) {
        const uint32_t cur = spill_ld(tab + s);
        if (cur == id) return false;
        if (cur == HX_EMPTY_SLOT) {
            const uint32_t old = atomicCAS(tab + s, HX_EMPTY_SLOT, id);
            if (old == HX_EMPTY_SLOT) return true;
            if (old == id) return false;
        }
        s = (s + 1) & mask;  // taken (by another id, possibly of this very pass): next slot
    }
}

template <int KIND>
__global__ void __launch_bounds__(64)
hx_search_spill_kernel(const DevView v, const SearchArgs a, const SpillScratch sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *yq = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
    const uint32_t qi = sp.q_first + blockIdx.x;
    const uint32_t q = a.qsel ? a.qsel[qi] : qi;
    u64 *L = sp.lists + (size_t)blockIdx.x * sp.list_cap;
    uint32_t *tab_all = sp.tabs + ((size_t)blockIdx.x << sp.tab_log2);
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;
    const uint32_t d = v.dim;
    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0;
    int32_t status = HNSW_OK;
    if (!stage_query<KIND>(v, a.Q + (size_t)q * d, yq, lane)) status = HNSW_ERR_NAN_INPUT;

    uint32_t n_cur = 0, hint = 0, n_vis = 0;  // hint: every entry before it is expanded
    u64 last_key = KEY_INVALID;                // key of the last entry once the list holds ef of them
    uint32_t tmask = 0, tshift = 0, vis_limit = 0;

    // `selected.insert(e)` + `pop_last` when over ef (searcher.rs:77-92), e wave-uniform
    auto insert_one = [&](u64 e, uint32_t ef_l) __attribute__((always_inline)) {
        if (n_cur >= ef_l && !(e < last_key)) return;
        uint32_t pos = 0;
        for (uint32_t i = 0; i < n_cur; i += 64) {  // entries below e: the list is sorted, the first chunk that holds a larger one ends the count
            const uint32_t idx = i + (uint32_t)lane;
            const u64 k = idx < n_cur ? (spill_ld(L + idx) & KEY_MASK) : KEY_INVALID;
            const u64 below = __ballot(k < e);
            pos += (uint32_t)__popcll(below);
            if (below != ~0ull) break;
        }
        const uint32_t n_new = n_cur < ef_l ? n_cur + 1 : n_cur;  // full: the last entry falls off
        for (uint32_t hi = n_new; hi > pos + 1;) {                // entries pos .. n_new - 2 move up by one, top chunk first
            const bool mv = hi >= 1u + (uint32_t)lane && hi - 1u - (uint32_t)lane > pos;
            const uint32_t idx = hi - 1u - (uint32_t)lane;
            u64 t = 0;
            if (mv) t = spill_ld(L + idx - 1);
            if (mv) spill_st(L + idx, t);  // the chunk's loads have returned before its stores issue
            if (hi <= 64) break;
            hi -= 64;
        }
        if (lane == 0) spill_st(L + pos, e);
        spill_fence();
        n_cur = n_new;
        if (pos < hint) hint = pos;
        last_key = n_cur >= ef_l ? (readlane64(spill_ld(L + (n_cur - 1)), 0) & KEY_MASK) : KEY_INVALID;
    };
    // one pass over up to CHUNK ids: visited filter, distance, then the batch applied in lane order
    auto process = [&](uint32_t id, bool valid, bool visit, uint32_t ef_l) __attribute__((always_inline)) {
        bool fresh = valid;
        if (visit) {
            bool f = false;
            if (valid && h == 0) f = spill_visited_insert(tab_all, tmask, tshift, id);
            if (LPC == 2) f = (pair_swap_i(f ? 1 : 0) | (f ? 1 : 0)) != 0;
            fresh = f;
        }
        const u64 fm = __ballot(fresh && h == 0);
        if (visit) n_vis += (uint32_t)__popcll(fm);
        if (fm == 0) return;
        n_dist += (uint32_t)__popcll(fm);
        const float dist = dist_any_dim<KIND>(v, id, fresh, h, yq);
        const bool mine = fresh && h == 0;
        if (__ballot(mine && dist != dist)) {
            status = HNSW_ERR_NAN_INPUT;  // Dist::cmp would panic (dist.rs:32)
            return;
        }
        const u64 key = mine ? (((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id) : KEY_INVALID;
        u64 it = __ballot(mine);
        while (it) {
            const int j = __ffsll((long long)it) - 1;
            it &= it - 1;
            insert_one(readlane64(key, j), ef_l);
        }
    };

    // the table of a layer: all of it for a wide list, 4096 slots of it for the greedy upper layers
    auto use_table = [&](uint32_t ef_l) __attribute__((always_inline)) {
        const uint32_t log2 = ef_l <= 64 ? min(sp.tab_log2, 12u) : sp.tab_log2;
        tmask = (1u << log2) - 1;
        tshift = 32 - log2;
        vis_limit = 1u << (log2 - 1);
        for (uint32_t s2 = lane; s2 <= tmask; s2 += 64) spill_st(tab_all + s2, HX_EMPTY_SLOT);
        spill_fence();
    };

    if (status == HNSW_OK) {
        // ---- entry set: {ep} (template.rs:316-319) or the caller's (search_layer seam) ----
        const uint32_t n_entry = a.entries ? a.n_entry : 1;
        const uint32_t ef_first = max(1u, (a.layer_hi > a.layer_lo) ? a.ef_upper : a.ef_bottom);
        for (uint32_t base = 0; base < n_entry; base += CHUNK) {
            const uint32_t i = base + cslot;
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
        use_table(ef_l);
        // candidates ∪= selected, visited ∪= ids(selected)  (searcher.rs:32-33)
        for (uint32_t i = 0; i < n_cur; i += 64) {
            const uint32_t idx = i + (uint32_t)lane;
            if (idx < n_cur) {
                const u64 k = spill_ld(L + idx) & KEY_MASK;
                spill_st(L + idx, k);
                spill_visited_insert(tab_all, tmask, tshift, (uint32_t)k);
            }
        }
        spill_fence();
        n_vis = n_cur;
        hint = 0;
        last_key = n_cur >= ef_l ? (readlane64(spill_ld(L + (n_cur - 1)), 0) & KEY_MASK) : KEY_INVALID;
        const uint32_t S = layer == 0 ? v.S0 : v.S1;
        while (status == HNSW_OK) {
            // ---- candidates.pop_first(): the smallest entry not expanded yet (searcher.rs:35-44) ----
            int pos = -1;
            u64 ck = 0;
            for (uint32_t i = hint; i < n_cur; i += 64) {
                const uint32_t idx = i + (uint32_t)lane;
                const u64 k = idx < n_cur ? spill_ld(L + idx) : KEY_INVALID;
                const u64 un = __ballot((k >> 63) == 0);
                if (un) {
                    const int j = __ffsll((long long)un) - 1;
                    pos = (int)i + j;
                    ck = readlane64(k, j);
                    break;
                }
            }
            if (pos < 0) break;
            if (lane == 0) spill_st(L + pos, ck | KEY_EXPANDED);
            spill_fence();
            hint = (uint32_t)pos + 1;
            const uint32_t cid = (uint32_t)ck;
            n_exp++;
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
            for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += CHUNK) {
                const uint32_t slot = c0 + cslot;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S) nb = row[slot];
                const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
                const bool valid = nb != HX_EMPTY_SLOT && !is_ptr;
                const u64 pm = __ballot(is_ptr);
                if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
                if (cnt == 0) continue;
                sum_deg += cnt;
                if (n_vis + cnt > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                process(nb, valid, true, ef_l);
            }
            if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of the row
                const uint32_t lo = v.ovf_off[ovf], hi = v.ovf_off[ovf + 1];
                for (uint32_t base = lo; base < hi && status == HNSW_OK; base += CHUNK) {
                    const uint32_t i = base + cslot;
                    const bool valid = i < hi;
                    const uint32_t nb = valid ? v.ovf_nbrs[i] : HX_EMPTY_SLOT;
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && h == 0));
                    sum_deg += cnt;
                    if (n_vis + cnt > vis_limit) {
                        status = HNSW_ERR_OVERFLOW;
                        break;
                    }
                    process(nb, valid, true, ef_l);
                }
            }
        }
    }

    // ---- get_top_selected(n) (results.rs:59-61) ----
    const uint32_t count = status == HNSW_OK ? min(a.n, n_cur) : 0;
    for (uint32_t idx = lane; idx < a.n; idx += 64) {
        const bool have = idx < count;
        const u64 k = have ? spill_ld(L + idx) : KEY_INVALID;
        a.out_ids[(size_t)q * a.n + idx] = have ? (uint32_t)k : HX_EMPTY_SLOT;
        if (a.out_dists)
            a.out_dists[(size_t)q * a.n + idx] =
                have ? __builtin_bit_cast(float, (uint32_t)((k & KEY_MASK) >> 32)) : __builtin_inff();
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

static int launch_spill(const DevView &v, const SearchArgs &a, uint32_t nblocks, uint32_t slots_log2,
                        hipStream_t stream, uint32_t ef_max) {
    // table: what the caller asks for (it doubles on HNSW_ERR_OVERFLOW), never more than 4 N slots -- a
    // layer visits every id at most once, so a table of 4 N cannot fill to its limit of one half
    uint32_t cap_log2 = 12;
    while (cap_log2 < 31 && (1ull << cap_log2) < 4ull * v.n_points) cap_log2++;
    const uint32_t tab_log2 = std::min(std::max(slots_log2, 12u), cap_log2);
    const uint64_t list_cap = ef_max;
    const uint64_t per_q = list_cap * 8 + (4ull << tab_log2);
    const uint64_t budget = 1ull << 30;  // scratch per launch
    const uint32_t group = (uint32_t)std::min<uint64_t>(nblocks, std::max<uint64_t>(1, budget / per_q));
    char site[64];
    snprintf(site, sizeof site, "search kernel launch (ef = %u)", ef_max);
    for (uint32_t first = 0; first < nblocks; first += group) {
        const uint32_t n = std::min(group, nblocks - first);
        void *mem = nullptr;
        bool async = true;
        if (hipMallocAsync(&mem, n * per_q, stream) != hipSuccess) {  // no stream-ordered pool: plain allocation
            (void)hipGetLastError();
            async = false;
            hipError_t e = hipMalloc(&mem, n * per_q);
            if (e != hipSuccess) {
                set_error("search with ef = %u needs %llu bytes of scratch: %s", ef_max, (unsigned long long)(n * per_q),
                          hipGetErrorString(e));
                return HNSW_ERR_OOM;
            }
        }
        SpillScratch sp{};
        sp.lists = static_cast<u64 *>(mem);
        sp.tabs = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(mem) + (size_t)n * list_cap * 8);
        sp.list_cap = (uint32_t)list_cap;
        sp.tab_log2 = tab_log2;
        sp.q_first = first;
        const int rc = launch_checked({site}, v.kind == HNSW_VEC_QUANT8 ? hx_search_spill_kernel<HNSW_VEC_QUANT8>
                                                                          : hx_search_spill_kernel<HNSW_VEC_F32>,
                                      dim3(n), dim3(64), query_lds_bytes(v), stream, v, a, sp);
        if (async) {
            (void)hipFreeAsync(mem, stream);
        } else {
            (void)hipStreamSynchronize(stream);
            (void)hipFree(mem);
        }
        if (rc != HNSW_OK) return rc;
    }
    return HNSW_OK;
}

int launch_search(const DevView &v, const SearchArgs &a_in, uint32_t nblocks, uint32_t slots_log2,
                  hipStream_t stream) {
    if (nblocks == 0) return HNSW_OK;
    SearchArgs a = a_in;
    if (sw::one_row()) a.flags |= 1u;
    uint32_t ef_max = std::max(1u, a.ef_bottom);
    if (a.layer_hi > a.layer_lo) ef_max = std::max(ef_max, a.ef_upper);
    if (a.entries) ef_max = std::max(ef_max, a.n_entry);
    if (slots_log2 == 0) slots_log2 = default_slots_log2(ef_max, v.S0);
    if (lean_applicable(v, a, ef_max)) return launch_lean(v, a, nblocks, slots_log2, stream);
    if (ef_max > 64 * HX_MAX_R) {
        // beyond 512 entries: the any-dimension kernel with sixteen list registers per lane (ef <= 1024;
        // one wave per CU: the visited table takes 128 KiB).  The reference has no limit
        // (template.rs:306-311); this is as far as a wave-resident list goes.
        // beyond 1024: list and visited table in HBM scratch, exact and slow (the reference has no limit)
        if (ef_max > 64 * HX_MAX_R_WIDE) return launch_spill(v, a, nblocks, slots_log2, stream, ef_max);
        if (v.kind == HNSW_VEC_QUANT8)
            return launch_one<HNSW_VEC_QUANT8, 0, 0, HX_MAX_R_WIDE, false>(v, a, nblocks, slots_log2, stream);
        return launch_one<HNSW_VEC_F32, 0, 0, HX_MAX_R_WIDE, false>(v, a, nblocks, slots_log2, stream);
    }
    if (v.kind == HNSW_VEC_QUANT8) {
        const uint32_t P = v.half_bytes / 16;
        if (v.dim == 100) return launch_r<HNSW_VEC_QUANT8, 4, 100>(v, a, nblocks, slots_log2, stream, ef_max);
        if (v.dim == 128 && P == 5) return launch_r<HNSW_VEC_QUANT8, 5, 128>(v, a, nblocks, slots_log2, stream, ef_max);
        if (v.dim == 256 && P == 9) return launch_r<HNSW_VEC_QUANT8, 9, 256>(v, a, nblocks, slots_log2, stream, ef_max);
        if (v.dim == 768 && P == 25) return launch_r<HNSW_VEC_QUANT8, 25, 768>(v, a, nblocks, slots_log2, stream, ef_max);
        switch (P) {
            case 1: return launch_r<HNSW_VEC_QUANT8, 1, 0>(v, a, nblocks, slots_log2, stream, ef_max);
            case 2: return launch_r<HNSW_VEC_QUANT8, 2, 0>(v, a, nblocks, slots_log2, stream, ef_max);
            case 3: return launch_r<HNSW_VEC_QUANT8, 3, 0>(v, a, nblocks, slots_log2, stream, ef_max);
            case 4: return launch_r<HNSW_VEC_QUANT8, 4, 0>(v, a, nblocks, slots_log2, stream, ef_max);
            case 5: return launch_r<HNSW_VEC_QUANT8, 5, 0>(v, a, nblocks, slots_log2, stream, ef_max);
            default: return launch_r<HNSW_VEC_QUANT8, 0, 0>(v, a, nblocks, slots_log2, stream, ef_max);
        }
    }
    if (v.dim == 100 && v.row_stride == 400)
        return launch_r<HNSW_VEC_F32, 25, 100>(v, a, nblocks, slots_log2, stream, ef_max);
    if (v.dim == 128 && v.row_stride == 512)
        return launch_r<HNSW_VEC_F32, 32, 128>(v, a, nblocks, slots_log2, stream, ef_max);
    if (v.dim == 256 && v.row_stride == 1024)
        return launch_r<HNSW_VEC_F32, 64, 256>(v, a, nblocks, slots_log2, stream, ef_max);
    if (v.dim == 768 && v.row_stride == 3072)
        return launch_r<HNSW_VEC_F32, 192, 768>(v, a, nblocks, slots_log2, stream, ef_max);
    return launch_r<HNSW_VEC_F32, 0, 0>(v, a, nblocks, slots_log2, stream, ef_max);
}

}  // namespace hx
