// build_kernels.hip -- the on-device index build as HIP kernels for gfx950: hx_insert_kernel (the
// insertion searches + heuristic of a batch), hx_connect_kernel / hx_remove_kernel (the edges, from sorted edge records),
// hx_scatter_rows_kernel (dirty rows of the host-connect build), and their launchers.  Host side: device_build.cpp.
// The wave primitives (WaveList, the visited table, the row distances) come from search_common.h.
//
// bench.py's kernel_sources_sha16 does NOT read this file: after an edit to a kernel here, profiles/traffic_latest.json
// (the insert kernel's recorded HBM traffic, attached to `bench.py --config 4` while that hash matches) must be retaken
// by hand.
//
// Float fidelity as in search_kernels.hip: -ffp-contract=off, the reference's accumulation order.

#include <algorithm>
#include <cstdlib>

#include "device_index.h"
#include "launch.h"
#include "search_common.h"
#include "switches.h"

namespace hx {

// =============================================================================================
// On-device insertion search (HNSW::insert's first half: Inserter::build_insertion_results,
// hnsw/src/template/inserter.rs:40-126) for a BATCH of already stored points against the current
// HBM graph, one wave per point:
//   setup_insert            selected = {(ep, d(ep, p))}                      inserter.rs:53-68
//   traverse_layers_above   search_layer(ef = 1) for layers > p.level       inserter.rs:70-89
//   traverse_layers_below   per layer l <= p.level: search_layer(ef_cons), select_heuristic(m,
//                           extend_cands = keep_pruned = true), save, and the selection seeds the
//                           next layer                                       inserter.rs:91-126
// The graph is read-only during a launch: points of one batch do not see each other (the reference's
// multi-threaded insert_bulk is racy in the same way, template.rs:403-440), so a graph built this
// way is judged by recall, not by identity with the sequential build.  Deviations, all documented
// in DESIGN.md: the heuristic's candidate set is capped at the 512 nearest (the reference keeps
// all of selected ∪ their neighbours); the un-popped heuristic candidates do not leak into the
// next layer's frontier.  The edges themselves are applied by hx_connect_kernel /
// hx_remove_kernel below from the edge records this kernel files (or, in the hybrid build, on the host
// with the reference's make_connections / prune_connections / make_pruned_connections).
// =============================================================================================
template <int KIND, int DS>
__global__ void __launch_bounds__(64)
hx_insert_kernel(const DevView v, const InsertArgs a, const uint32_t slots_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = HX_MAX_R;  // list capacity 512: the heuristic's candidate set lives in it
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t p = a.point_ids[b];
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    const uint32_t hslots = 1u << slots_log2, hmask = hslots - 1;
    const uint32_t vis_limit = hslots - (hslots >> 2);
    u64 *perm = reinterpret_cast<u64 *>(smem + 4ull * hslots);
    u64 *selk = perm + 64 * R;                                   // [128] selected keys (m <= 128)
    const uint32_t yq_bytes =  // == query_lds_bytes(v) (launch.h), KIND being v.kind: the launcher reserves that
        ((KIND == HNSW_VEC_QUANT8 ? 2u * (v.half_bytes - 8) * 4u : v.dim * 4u) + 15u) & ~15u;
    float *yq = reinterpret_cast<float *>(selk + 128);
    float *yqe = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(yq) + yq_bytes);
    // cooperative row gather (f32 rows of whole lines): the stage image lives in perm (4 KiB, used by the
    // merges only, never during a distance pass), the rank -> id words behind the staged rows
    unsigned char *coop_img = reinterpret_cast<unsigned char *>(perm);
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(yqe) + yq_bytes);
    static_assert(!coop_rows<KIND, DS>() || 64 * R * 8 >= (int)HX_COOP_IMG_BYTES, "perm holds the stage image");

    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;
    const bool first = (LPC == 1) || (h == 0);
    int32_t status = HNSW_OK;
    uint32_t n_vis = 0;
    // what this point's insertion reads (wave-uniform; summed into a.counters at the end): vector rows
    // (distance evaluations + staged rows), adjacency rows and the ids in them -- the build's algorithmic bytes
    uint32_t c_rows = 1, c_adj = 0, c_ids = 0;

    const uint32_t level = min((uint32_t)a.levels[p], v.nb_layers - 1);
    const uint32_t m = a.m, ef_cons = max(1u, a.ef_cons);
    // outputs of this point: [max_layers][m], padded
    uint32_t *o_ids = a.out_ids + (size_t)b * a.max_layers * m;
    float *o_d = a.out_dists + (size_t)b * a.max_layers * m;
    for (uint32_t i = lane; i < a.max_layers * m; i += 64) {
        o_ids[i] = HX_EMPTY_SLOT;
        o_d[i] = __builtin_inff();
    }

    stage_row<KIND>(v, p, yq, lane);

    WaveList<R> wl;
#pragma unroll
    for (int r = 0; r < R; r++) wl.L[r] = KEY_INVALID;
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;

    // one pass over up to CHUNK ids: optional visited filter, distance to the staged row, merge
    auto process = [&](uint32_t id, bool valid, bool visit, uint32_t ef_l, u64 new_flag) __attribute__((always_inline)) {
        bool fresh = valid;
        if (visit) {
            bool f = false;
            if (valid && first) f = visited_insert(htab, hmask, slots_log2, id);
            if (LPC == 2) f = (pair_swap_i(f ? 1 : 0) | (f ? 1 : 0)) != 0;
            fresh = f;
        }
        const u64 fm = __ballot(fresh && first);
        if (visit) n_vis += (uint32_t)__popcll(fm);  // what the table really holds
        if (fm == 0) return;
        c_rows += (uint32_t)__popcll(fm);
        const float dist = dist_build<KIND, DS, true>(v, id, fresh, h, yq, coop_ids, coop_img, lane);
        u64 key = KEY_INVALID;
        bool nan = false;
        if (fresh && first) {
            nan = dist != dist;
            if (!nan) key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
        }
        if (__ballot(nan)) status = HNSW_ERR_NAN_INPUT;
        // The list has eight registers for the heuristic's 512 candidates, and a merge pays its rank / scatter
        // work per register.  Entries beyond min(n_cur + batch, ef) cannot exist before or after this merge, so it
        // runs over the registers that can hold something: one for the searches (ef = 1 above the point's level,
        // ef_cons <= 64 below), two or four while the candidate set is filling.
        const uint32_t reach = min(wl.n_cur + (uint32_t)__popcll(fm), ef_l);
        if (reach <= 64u)
            merge_prefix<1>(wl, key, ef_l, perm, lane, new_flag);
        else if (reach <= 128u)
            merge_prefix<2>(wl, key, ef_l, perm, lane, new_flag);
        else if (reach <= 256u)
            merge_prefix<4>(wl, key, ef_l, perm, lane, new_flag);
        else
            wl.merge(key, ef_l, perm, lane, new_flag);
    };
    // expand every unexpanded entry of the list on `layer` (search_layer's loop, searcher.rs:35-95)
    auto expand_all = [&](int layer, uint32_t ef_l, u64 new_flag) __attribute__((always_inline)) {
        const uint32_t S = layer == 0 ? v.S0 : v.S1;
        // the entry at cpos: marked expanded, its id returned
        auto take = [&](int cpos) __attribute__((always_inline)) -> uint32_t {
            uint32_t cid = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((cpos >> 6) == r) {
                    cid = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wl.L[r], cpos & 63);
                    if (lane == (cpos & 63)) wl.L[r] |= KEY_EXPANDED;
                }
            }
            return cid;
        };
        auto row_of = [&](uint32_t cid) __attribute__((always_inline)) -> const uint32_t * {
            if (layer == 0) return v.adj0 + (size_t)cid * S;
            const uint32_t ub = v.upper_base[cid];
            if (ub == HX_EMPTY_SLOT) {
                status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                return nullptr;
            }
            return v.adj_up + ((size_t)ub + layer - 1) * S;
        };
        // The heuristic's extension (new entries are born expanded) expands a FIXED set -- the entries the search
        // left -- and keeps the union of their neighbours: the order does not matter, so with one lane per row
        // (f32) and rows of up to 32 slots TWO entries go through one pass, one per half wave, instead of
        // leaving the upper half idle (the visited insert settles an id both rows hold).
        const bool two = LPC == 1 && new_flag != 0 && S <= 32;
        while (status == HNSW_OK) {
            const int cpos = wl.first_unexpanded(lane);
            if (cpos < 0) break;
            const uint32_t cid = take(cpos);
            const uint32_t *row = row_of(cid);
            if (row == nullptr) break;
            c_adj++;
            if (two) {
                const int cpos2 = wl.first_unexpanded(lane);
                const uint32_t *row2 = nullptr;
                if (cpos2 >= 0) {
                    row2 = row_of(take(cpos2));
                    if (row2 == nullptr) break;
                    c_adj++;
                }
                const bool upper = lane >= 32;
                const uint32_t slot = (uint32_t)lane & 31u;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S && (!upper || row2 != nullptr)) nb = (upper ? row2 : row)[slot];
                const bool valid = nb != HX_EMPTY_SLOT && !(nb & HX_OVF_FLAG) && nb != p;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
                c_ids += cnt;
                if (cnt == 0) continue;
                if (n_vis + cnt > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                process(nb, valid, true, ef_l, new_flag);
                continue;
            }
            for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += CHUNK) {
                const uint32_t slot = c0 + cslot;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S) nb = row[slot];
                // during a build the device rows never carry overflow pointers (rows are truncated
                // to the stride when they are scattered); a flagged id is skipped
                const bool valid = nb != HX_EMPTY_SLOT && !(nb & HX_OVF_FLAG) && nb != p;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid && first));
                c_ids += cnt;
                if (cnt == 0) continue;
                if (n_vis + cnt > vis_limit) {
                    status = HNSW_ERR_OVERFLOW;
                    break;
                }
                process(nb, valid, true, ef_l, new_flag);
            }
        }
    };
    // start a layer: visited.clear(), candidates ∪= selected, visited ∪= ids(selected)
    auto begin_layer = [&](uint32_t ef_l) __attribute__((always_inline)) {
        for (uint32_t s = lane; s < (hslots >> 2); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] =
                make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (64u * r + lane < wl.n_cur) {
                wl.L[r] &= KEY_MASK;
                visited_insert(htab, hmask, slots_log2, (uint32_t)wl.L[r]);
            }
        }
        n_vis = wl.n_cur;
        wl.refresh_last(ef_l);
    };

    if (p == v.ep || p >= v.n_points) status = HNSW_ERR_ARG;  // the host never sends the entry point
    if (status == HNSW_OK) process(v.ep, lane < LPC, false, 1u, 0);  // setup_insert

    for (int layer = (int)v.nb_layers - 1; status == HNSW_OK && layer >= 0; layer--) {
        if ((uint32_t)layer > level) {  // traverse_layers_above
            begin_layer(1u);
            expand_all(layer, 1u, 0);
            continue;
        }
        // ---- search_layer(ef_cons) ----
        begin_layer(ef_cons);
        expand_all(layer, ef_cons, 0);
        if (status != HNSW_OK) break;
        // ---- select_heuristic: candidates = selected ∪ neighbours(selected), distances to p
        // (results.rs:105-146).  Every current entry is expanded once more, this time keeping ALL
        // distinct neighbours (cap 512 nearest); entries that arrive now are born expanded.
        begin_layer(64u * R);
        expand_all(layer, 64u * R, KEY_EXPANDED);
        if (status != HNSW_OK) break;
        // The reference pops the candidates in ascending order and accepts e iff (d(e,p), e) <
        // (d(e,s), s) for every s selected so far (searcher.rs:128-139).  Equivalent, and parallel:
        // whenever a candidate s is selected, every LATER candidate e with (d(s,e), s) < (d(e,p), e)
        // is marked rejected (d is bit-symmetric); the next selection is the first unmarked one.
        // Each round stages s once and evaluates up to 64 / LPC candidates per pass.
        const uint32_t n_c = wl.n_cur;
        uint32_t ns = 0;
        uint32_t selbits = 0;  // bit r: the candidate at position 64 r + lane was selected
#pragma unroll
        for (int r = 0; r < R; r++) wl.L[r] &= KEY_MASK;  // the flag now means "rejected"
        uint32_t cursor = 0;
        // One sweep: the staged selected point (yqe, id sid) against the open candidates at positions [lo, hi):
        // those it dominates -- (d(s, e), s) < (d(e, p), e) -- are marked rejected.
        // (a rolled loop over the list registers with static selects: one copy of the distance
        // code instead of R x LPC, and the list stays in registers)
        auto sweep = [&](uint32_t sid, uint32_t lo, uint32_t hi) __attribute__((always_inline)) {
#pragma unroll 1
            for (int rr = 0; rr < R; rr++) {
                if (64u * rr + 64u <= lo || 64u * rr >= hi) continue;
                u64 mine = KEY_INVALID;
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (r == rr) mine = wl.L[r];
                const uint32_t idx = 64u * rr + lane;
                const bool open = idx >= lo && idx < hi && (mine & KEY_EXPANDED) == 0;
                if (__ballot(open) == 0) continue;
                const uint32_t my_id = (uint32_t)mine, my_db = (uint32_t)(mine >> 32);
                bool mark = false;
#pragma unroll
                for (int half = 0; half < LPC; half++) {
                    const int src = half * CHUNK + cslot;  // the lane that owns this pass's candidate
                    const uint32_t cid = (uint32_t)__shfl((int)my_id, src);
                    const uint32_t cdb = (uint32_t)__shfl((int)my_db, src);
                    const bool act = __shfl(open ? 1 : 0, src) != 0;
                    if (__ballot(act) == 0) continue;
                    c_rows += (uint32_t)__popcll(__ballot(act && first));
                    const float dist = dist_build<KIND, DS, true>(v, cid, act, h, yqe, coop_ids, coop_img, lane);
                    bool rej = false;
                    if (act && first) {
                        if (dist != dist) status = HNSW_ERR_NAN_INPUT;
                        const u64 sk = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | sid;
                        const u64 ck = ((u64)cdb << 32) | cid;
                        rej = sk < ck;
                    }
                    const u64 rm = __ballot(rej);  // bit LPC * cslot of the pass <-> owner lane src
                    const int own = lane - half * CHUNK;
                    if (own >= 0 && own < CHUNK && ((rm >> (LPC * own)) & 1)) mark = true;
                }
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (r == rr && mark) wl.L[r] |= KEY_EXPANDED;
            }
        };
        // The candidate set holds up to 512 entries but m selections usually come out of the first hundred:
        // a selected point sweeps only the WINDOW [0, win_end) of candidates; when the window holds nothing
        // unpopped and fewer than m are selected, it grows by 64 and the points selected so far sweep the new
        // part first.  Every candidate is still judged against every point selected before it is popped, so the
        // selection is the one the whole-set sweep made (round 2: every selection swept all 512 -- eight distance
        // passes per selection, most of them for candidates that are never reached).
        uint32_t win_end = min(n_c, 128u);
        while (ns < m && status == HNSW_OK) {
            int pos = -1;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t idx = 64u * r + lane;
                const u64 mk = __ballot(idx >= cursor && idx < win_end && (wl.L[r] & KEY_EXPANDED) == 0);
                if (pos < 0 && mk) pos = 64 * r + (__ffsll((long long)mk) - 1);
            }
            if (pos < 0) {
                if (win_end >= n_c) break;  // every candidate was popped
                const uint32_t new_end = min(n_c, win_end + 64u);
                for (uint32_t k2 = 0; k2 < ns && status == HNSW_OK; k2++) {  // catch up: the new part against the selected
                    const uint32_t sid2 = (uint32_t)selk[k2];
                    c_rows++;
                    stage_row<KIND>(v, sid2, yqe, lane);
                    sweep(sid2, win_end, new_end);
                }
                cursor = win_end;
                win_end = new_end;
                if (__ballot(status != HNSW_OK)) status = HNSW_ERR_NAN_INPUT;
                continue;
            }
            u64 sk_sel = 0;
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((pos >> 6) == r) {
                    sk_sel = readlane64(wl.L[r], pos & 63);
                    if (lane == (pos & 63)) selbits |= 1u << r;
                }
            if (lane == 0) selk[ns] = sk_sel;
            ns++;
            cursor = (uint32_t)pos + 1;
            wave_fence();
            if (ns >= m || (cursor >= win_end && win_end >= n_c)) continue;  // nothing left to decide
            const uint32_t sid = (uint32_t)sk_sel;
            c_rows++;
            stage_row<KIND>(v, sid, yqe, lane);
            sweep(sid, cursor, win_end);
            if (__ballot(status != HNSW_OK)) status = HNSW_ERR_NAN_INPUT;
        }
        // keep_pruned: fill up from the rejected candidates in ascending order (searcher.rs:141-146);
        // only reached with ns < m when every candidate was popped
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t idx = 64u * r + lane;
            u64 mk = __ballot(idx < n_c && (wl.L[r] & KEY_EXPANDED) != 0 && ((selbits >> r) & 1u) == 0);
            while (mk && ns < m && status == HNSW_OK) {
                const int j = __ffsll((long long)mk) - 1;
                mk &= mk - 1;
                const u64 ek = readlane64(wl.L[r], j) & KEY_MASK;
                if (lane == 0) selk[ns] = ek;
                ns++;
            }
        }
        wave_fence();
        // save_layer_results + the selection seeds the next layer (up to 128 selected: two rounds of 64)
#pragma unroll
        for (int r = 0; r < R; r++) wl.L[r] = KEY_INVALID;
        wl.n_cur = 0;
        wl.last_key = KEY_INVALID;
        for (uint32_t j0 = 0; j0 < max(ns, 1u); j0 += 64) {
            const uint32_t j = j0 + (uint32_t)lane;
            const u64 mine = j < ns ? selk[j] : KEY_INVALID;
            if (j < ns) {
                o_ids[(size_t)layer * m + j] = (uint32_t)mine;
                o_d[(size_t)layer * m + j] = __builtin_bit_cast(float, (uint32_t)(mine >> 32));
            }
            wl.merge(mine, max(ns, 1u), perm, lane);
        }
    }
    if (__ballot(status != HNSW_OK)) {
        int32_t st = status;
        for (int o = 32; o > 0; o >>= 1) st = min(st, __shfl_xor(st, o));
        status = st;
    }
    if (a.req_keys != nullptr && status == HNSW_OK) {
        // on-device connect: only a point whose every layer succeeded writes its own rows (nobody can
        // reach p yet) and files one reverse-edge request per selected neighbour
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint32_t total = 0;
        for (uint32_t l = 0; l <= level; l++) {
            for (uint32_t j0 = 0; j0 < m; j0 += 64) {
                const uint32_t j = j0 + (uint32_t)lane;
                const uint32_t id = j < m ? o_ids[(size_t)l * m + j] : HX_EMPTY_SLOT;
                total += (uint32_t)__popcll(__ballot(id != HX_EMPTY_SLOT));
            }
        }
        // emit_own (sharded build): the point's own rows travel as records too -- (layer, p <- n) next
        // to (layer, n <- p) -- so that the record list alone carries the whole batch to every replica
        const uint32_t per_edge = a.emit_own ? 2u : 1u;
        total *= per_edge;
        // Reserve `total` record slots with ONE atomic add.  Round 2 reserved by compare-and-swap so that the counter
        // never passed the last written record; 8192 waves retrying on one word made that loop 85 % of the insert
        // kernel (1M points: 2.21 s against 0.34 s; 90 % of a wave's life in SQ_WAIT_ANY).  The add keeps the
        // guarantee another way: once a reservation does not fit, the counter is beyond the capacity for good and
        // every later one fails too, so the records written are exactly the prefix [0, B) where B is the base of the
        // first failing reservation -- the smallest failing base, kept in *req_fail_base (atomic min; the host
        // starts it at 0xFFFFFFFF and takes min(counter, B) as the record count).
        uint32_t base = 0xFFFFFFFFu;
        if (lane == 0) {
            base = atomicAdd(a.req_count, total);
            if ((uint64_t)base + total > a.req_cap) {
                atomicMin(a.req_fail_base, base);
                base = 0xFFFFFFFFu;
            }
        }
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base == 0xFFFFFFFFu) {
            status = HNSW_ERR_OVERFLOW;  // nothing written, nothing reserved: the point takes the CPU path
        } else {
            for (uint32_t l = 0; l <= level; l++) {
                const uint32_t S = l == 0 ? v.S0 : v.S1;
                // the layer's selection is a prefix of its m output slots: cnt of them are filled
                uint32_t cnt = 0;
                for (uint32_t j0 = 0; j0 < m; j0 += 64) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    cnt += (uint32_t)__popcll(__ballot(j < m && o_ids[(size_t)l * m + j] != HX_EMPTY_SLOT));
                }
                for (uint32_t j0 = 0; j0 < max(S, m); j0 += 64) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    const uint32_t id = j < m ? o_ids[(size_t)l * m + j] : HX_EMPTY_SLOT;
                    if (!a.emit_own) {
                        const size_t at = l == 0 ? (size_t)p * S : ((size_t)v.upper_base[p] + l - 1) * S;
                        uint32_t *row = (l == 0 ? a.adj0_mut : a.adj_up_mut) + at;
                        if (j < S) row[j] = id;
                        uint32_t *rowd = l == 0 ? a.adjd0_mut : a.adjd_up_mut;
                        if (rowd != nullptr && j < S)  // the edge's distance travels with it (ConnectArgs)
                            rowd[at + j] = id != HX_EMPTY_SLOT ? __builtin_bit_cast(uint32_t, o_d[(size_t)l * m + j]) : 0xFFFFFFFFu;
                    }
                    if (id != HX_EMPTY_SLOT) {
                        const uint32_t db = __builtin_bit_cast(uint32_t, o_d[(size_t)l * m + j]);
                        a.req_keys[base + j] = hx_edge_key(l, id, p);
                        a.req_vals[base + j] = db;
                        if (a.emit_own) {
                            a.req_keys[base + cnt + j] = hx_edge_key(l, p, id);
                            a.req_vals[base + cnt + j] = db;
                        }
                    }
                }
                base += cnt * per_edge;
            }
        }
    }
    if (lane == 0) a.out_status[b] = status;
    if (a.counters != nullptr && lane == 0) {
        atomicAdd(a.counters + 0, (unsigned long long)c_rows);
        atomicAdd(a.counters + 1, (unsigned long long)c_adj);
        atomicAdd(a.counters + 2, (unsigned long long)c_ids);
    }
}

// rows[row_index[i]] = data[i] for whole adjacency rows of S slots (dirty rows after a build batch)
__global__ void __launch_bounds__(64)
hx_scatter_rows_kernel(uint32_t *dst, uint32_t S, const uint32_t *row_index, const uint32_t *data,
                       uint32_t n) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    uint32_t *out = dst + (size_t)row_index[i] * S;
    for (uint32_t k = threadIdx.x; k < S; k += 64) out[k] = data[(size_t)i * S + k];
}

// First-attempt size of the insert kernel's visited table, relative to the standard one: - 1 (2048 slots, 8 KiB)
// for ef_construction <= 32 on 32-slot rows.  LDS is what limits the insert kernel's waves per CU (6 with the
// standard 16-KiB table at d = 256, 10 with 8 KiB): 16M x 256d, insert kernel 12.3 -> 10.1 s with 29 points of
// 16M filling the small table (they run again with adjust + 1; round 3).
int insert_table_first_adjust(const DevView &v, const InsertArgs &a) {
    return sw::insert_table_adjust((a.ef_cons <= 32 && v.S0 <= 32) ? -1 : 0);  // (the switch: A/B runs)
}

int launch_insert(const DevView &v, const InsertArgs &a, uint32_t nblocks, hipStream_t stream, int table_adjust) {
    if (nblocks == 0) return HNSW_OK;
    if (a.m > 128 || a.m == 0 || a.ef_cons > 64 * HX_MAX_R) {
        set_error("on-device build supports m <= 128 and ef_construction <= 512");
        return HNSW_ERR_ARG;
    }
    // visited table: what ef_cons list entries with rows of S0 slots visit (m <= 32: 4096 / 8192 / 16384 slots as
    // before; the 128- and 256-slot rows of m = 64 / 128 take up to 32768 slots = 128 KiB, one wave per CU -- a
    // point that still fills it takes the CPU path after the build, like every point whose search fails)
    uint32_t slots_log2 = 12 + (a.ef_cons > 64 ? 1 : 0) + (a.ef_cons > 160 ? 1 : 0);
    if (v.S0 > 64) slots_log2 = std::max(slots_log2, std::min(15u, default_slots_log2(a.ef_cons, v.S0)));
    // table_adjust: the device-connect build first runs a batch with HALF the table where that buys waves per
    // CU (insert_table_first_adjust) and runs the few points that fill it again with a larger one
    slots_log2 = (uint32_t)std::min(15, std::max(9, (int)slots_log2 + table_adjust));
    const size_t lds = (4ull << slots_log2) + 64ull * HX_MAX_R * 8 + 128 * 8 + 2 * (size_t)query_lds_bytes(v) + 256 /* rank -> id words */;
    // the configs[1] dimension gets compile-time row loops
    void (*kfn)(const DevView, const InsertArgs, const uint32_t);
    if (v.kind == HNSW_VEC_QUANT8)
        kfn = v.dim == 100   ? hx_insert_kernel<HNSW_VEC_QUANT8, 100>
              : v.dim == 128 ? hx_insert_kernel<HNSW_VEC_QUANT8, 128>
              : v.dim == 256 ? hx_insert_kernel<HNSW_VEC_QUANT8, 256>
              : v.dim == 768 ? hx_insert_kernel<HNSW_VEC_QUANT8, 768>
                             : hx_insert_kernel<HNSW_VEC_QUANT8, 0>;
    else
        kfn = v.dim == 100                           ? hx_insert_kernel<HNSW_VEC_F32, 100>
              : v.dim == 128                         ? hx_insert_kernel<HNSW_VEC_F32, 128>
              : v.dim == 256 && v.row_stride == 1024 ? hx_insert_kernel<HNSW_VEC_F32, 256>  // the configs[4] dimension
              : v.dim == 768 && v.row_stride == 3072 ? hx_insert_kernel<HNSW_VEC_F32, 768>  // the configs[2] dimension
                                                     : hx_insert_kernel<HNSW_VEC_F32, 0>;
    return launch_checked({"insert kernel launch", "insert kernel needs %zu bytes of LDS"}, kfn, dim3(nblocks), dim3(64), lds,
                          stream, v, a, slots_log2);
}

// ---------------------------------------------------------------------------------------------
// On-device connect.  Edge records hx_edge_key(layer, row node, other node) arrive radix-sorted, so
// the records of one adjacency row are adjacent; one wave is launched per record, the wave of a
// row's first record owns the row for the phase and the others exit at once.  Rows are owned by
// exactly one wave per phase: no locks, no atomics on rows, deterministic for a given batch.
//
// Phase 2 (hx_connect_kernel): make_connections adds the sources to the row (template.rs:196-207); a
// row that would exceed the layer's cap is pruned to its `cap` nearest by (dist, id)
// (prune_connections / select_simple, template.rs:209-238,614-621) -- distances of the existing
// neighbours are evaluated here, the sources bring d(p, n) = d(n, p).  Every dropped neighbour x (and
// every source that did not make it) is reported so that phase 3 removes the reverse edge
// (remove_edge is symmetric, graph.rs:72-83).
// ---------------------------------------------------------------------------------------------
static constexpr uint64_t HX_EDGE_ID_MASK = (1ull << HX_EDGE_ID_BITS) - 1;

// number of records of the row that starts at record i (0 if i is not the first of its row)
__device__ __forceinline__ uint32_t edge_group_size(const uint64_t *keys, uint32_t count, uint32_t i, int lane) {
    const uint64_t prefix = keys[i] >> HX_EDGE_ID_BITS;
    if (i > 0 && (keys[i - 1] >> HX_EDGE_ID_BITS) == prefix) return 0;
    uint32_t k = 1;
    for (;;) {
        const uint32_t j = i + k + lane;
        const bool same = j < count && (keys[j] >> HX_EDGE_ID_BITS) == prefix;
        const u64 diff = ~__ballot(same);
        if (diff) return k + (uint32_t)(__ffsll((long long)diff) - 1);
        k += 64;
    }
}

// RS = registers per lane that hold one adjacency row (slot 64 r + lane): 1 for rows of up to 64 slots
// (m <= 32), 2 / 4 for the 128- / 256-slot layer-0 rows of m = 64 / 128 (the reference's own build benches
// use M in {32, 64, 128}, hnsw/benches/hnsw_benchmarks.rs:7)
template <int KIND, int DS, int RS>
__global__ void __launch_bounds__(64)
hx_connect_kernel(const DevView v, const ConnectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *perm = reinterpret_cast<u64 *>(smem);       // [64 RS]
    u64 *ekeys = perm + 64 * RS;                      // [64 RS] keys of the existing neighbours
    float *yq = reinterpret_cast<float *>(ekeys + 64 * RS);
    const int lane = threadIdx.x;
    const uint32_t lo = blockIdx.x;
    if (lo >= a.count) return;
    const uint32_t k = edge_group_size(a.keys, a.count, lo, lane);
    if (k == 0) return;
    const uint64_t head = a.keys[lo];
    const uint32_t n = (uint32_t)((head >> HX_EDGE_ID_BITS) & HX_EDGE_ID_MASK);
    const uint32_t layer = (uint32_t)(head >> (2 * HX_EDGE_ID_BITS));
    const uint32_t S = layer == 0 ? v.S0 : v.S1;
    const uint32_t cap = layer == 0 ? 2 * a.m : a.m;
    if (n >= v.n_points || layer >= v.nb_layers || (layer > 0 && v.upper_base[n] == HX_EMPTY_SLOT) || S > 64u * RS) {
        *a.status = HNSW_ERR_NODE_NOT_IN_GRAPH;  // a malformed record: never touch memory for it
        return;
    }
    if (a.own_world > 1) {  // sharded build: this row has ONE owner among the ranks
        if (n % a.own_world != a.own_rank) return;
        if (lane == 0) {     // its new contents will travel to the other replicas (64 lists: one counter would serialise)
            const uint32_t seg = blockIdx.x & (HX_CHG_LISTS - 1), at = atomicAdd(a.chg_count + seg, 1u);
            if (at < a.chg_cap)
                a.chg_keys[(size_t)seg * a.chg_cap + at] = hx_edge_key(layer, n, 0);
            else
                *a.status = HNSW_ERR_OVERFLOW;
        }
    }
    const size_t row_at = layer == 0 ? (size_t)n * S : ((size_t)v.upper_base[n] + layer - 1) * S;
    uint32_t *row = (layer == 0 ? a.adj0_mut : a.adj_up_mut) + row_at;
    uint32_t *rowd = layer == 0 ? a.adjd0_mut : a.adjd_up_mut;  // the edges' distances, or null
    if (rowd != nullptr) rowd += row_at;
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const int cslot = lane / LPC;
    const bool first = (LPC == 1) || (h == 0);

    uint32_t cur[RS], curd[RS];
    u64 hm[RS];
    uint32_t deg = 0;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const uint32_t slot = 64u * r + (uint32_t)lane;
        cur[r] = slot < S ? row[slot] : HX_EMPTY_SLOT;
        curd[r] = (rowd != nullptr && slot < S) ? rowd[slot] : 0xFFFFFFFFu;
        hm[r] = __ballot(cur[r] != HX_EMPTY_SLOT);
        deg += (uint32_t)__popcll(hm[r]);
    }
    if (deg + k <= cap && deg + k <= S) {  // room for every source: append
        uint32_t before = 0;               // (all reads of the row happened above)
#pragma unroll
        for (int r = 0; r < RS; r++) {
            if (cur[r] != HX_EMPTY_SLOT) {
                const uint32_t at = before + (uint32_t)__popcll(hm[r] & ((1ull << lane) - 1));
                row[at] = cur[r];
                if (rowd != nullptr) rowd[at] = curd[r];
            }
            before += (uint32_t)__popcll(hm[r]);
        }
        for (uint32_t j = lane; j < k; j += 64) {
            row[deg + j] = (uint32_t)(a.keys[lo + j] & HX_EDGE_ID_MASK);
            if (rowd != nullptr) rowd[deg + j] = a.vals[lo + j];  // d(source, n) = d(n, source)
        }
        for (uint32_t j = deg + k + lane; j < S; j += 64) {
            row[j] = HX_EMPTY_SLOT;
            if (rowd != nullptr) rowd[j] = 0xFFFFFFFFu;
        }
        return;
    }
    // ---- prune: keep the `cap` nearest of existing ∪ sources ----
    // the node's own row is staged only when some existing neighbour's distance is not known yet
    bool any_unknown = false;
#pragma unroll
    for (int r = 0; r < RS; r++) any_unknown |= __ballot(cur[r] != HX_EMPTY_SLOT && curd[r] == 0xFFFFFFFFu) != 0;
    if (any_unknown) stage_row<KIND>(v, n, yq, lane);
    WaveList<RS> wl;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        wl.L[r] = KEY_INVALID;
        ekeys[64 * r + lane] = KEY_INVALID;
    }
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;
    wave_fence();
    for (uint32_t c0 = 0; c0 < S; c0 += CHUNK) {  // existing neighbours, CHUNK at a time
        const uint32_t slot = c0 + cslot;
        uint32_t id = HX_EMPTY_SLOT, dbits = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < RS; r++) {
            const uint32_t t = (uint32_t)__shfl((int)cur[r], (int)(slot & 63));
            const uint32_t td = (uint32_t)__shfl((int)curd[r], (int)(slot & 63));
            if ((slot >> 6) == (uint32_t)r) {
                id = t;
                dbits = td;
            }
        }
        const bool act = slot < S && id < v.n_points;
        if (slot < S && id != HX_EMPTY_SLOT && id >= v.n_points) *a.status = HNSW_ERR_NODE_NOT_IN_GRAPH;
        const bool need = act && dbits == 0xFFFFFFFFu;  // (an edge that predates the build: evaluated once, kept from here on)
        if (__ballot(need) != 0) {
            const float dist = dist_build<KIND, DS>(v, id, need, h, yq);
            if (need) dbits = __builtin_bit_cast(uint32_t, dist);
        }
        u64 key = KEY_INVALID;
        if (act && first) {
            key = ((u64)dbits << 32) | id;
            ekeys[slot] = key;
        }
        wl.merge(key, cap, perm, lane);
    }
    auto source_key = [&](uint32_t j) -> u64 {
        return j < k ? ((u64)a.vals[lo + j] << 32) | (uint32_t)(a.keys[lo + j] & HX_EDGE_ID_MASK) : KEY_INVALID;
    };
    for (uint32_t j0 = 0; j0 < k; j0 += 64) wl.merge(source_key(j0 + lane), cap, perm, lane);
    wave_fence();
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const uint32_t slot = 64u * r + (uint32_t)lane;
        if (slot < S) {
            row[slot] = slot < wl.n_cur ? (uint32_t)wl.L[r] : HX_EMPTY_SLOT;
            if (rowd != nullptr) rowd[slot] = slot < wl.n_cur ? (uint32_t)(wl.L[r] >> 32) : 0xFFFFFFFFu;
        }
    }
    // report what fell out: key > the last kept key (keys are distinct)
    const u64 lastk = wl.n_cur >= cap ? wl.last_key : KEY_INVALID;
    auto emit = [&](u64 key) {
        const bool drop = key != KEY_INVALID && key > lastk;
        const u64 dm = __ballot(drop);
        if (dm == 0) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(a.out_count, (uint32_t)__popcll(dm));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const uint32_t at = base + (uint32_t)__popcll(dm & ((1ull << lane) - 1));
        if (drop) {
            if (at < a.out_cap)
                a.out_keys[at] = hx_edge_key(layer, (uint32_t)key, n);
            else
                *a.status = HNSW_ERR_OVERFLOW;
        }
    };
#pragma unroll
    for (int r = 0; r < RS; r++) emit(ekeys[64 * r + lane]);
    for (uint32_t j0 = 0; j0 < k; j0 += 64) emit(source_key(j0 + lane));
}

// ---------------------------------------------------------------------------------------------
// Phase 3 (hx_remove_kernel): the row of x drops the neighbours that dropped x in phase 2.  An edge
// to x's LAST neighbour is kept (isolate_node, graph.rs:85-94): such a refusal is reported and the
// host restores the reverse direction after the build.
// ---------------------------------------------------------------------------------------------
template <int RS>
__global__ void __launch_bounds__(64)
hx_remove_kernel(const DevView v, const ConnectArgs a) {
    const int lane = threadIdx.x;
    const uint32_t lo = blockIdx.x;
    if (lo >= a.count) return;
    const uint32_t k = edge_group_size(a.keys, a.count, lo, lane);
    if (k == 0) return;
    const uint64_t head = a.keys[lo];
    const uint32_t x = (uint32_t)((head >> HX_EDGE_ID_BITS) & HX_EDGE_ID_MASK);
    const uint32_t layer = (uint32_t)(head >> (2 * HX_EDGE_ID_BITS));
    const uint32_t S = layer == 0 ? v.S0 : v.S1;
    if (x >= v.n_points || layer >= v.nb_layers || (layer > 0 && v.upper_base[x] == HX_EMPTY_SLOT) || S > 64u * RS) {
        *a.status = HNSW_ERR_NODE_NOT_IN_GRAPH;
        return;
    }
    if (a.own_world > 1) {  // sharded build: x's row is dropped from by its owner only, and shipped afterwards
        if (x % a.own_world != a.own_rank) return;
        if (lane == 0) {
            const uint32_t seg = blockIdx.x & (HX_CHG_LISTS - 1), at = atomicAdd(a.chg_count + seg, 1u);
            if (at < a.chg_cap)
                a.chg_keys[(size_t)seg * a.chg_cap + at] = hx_edge_key(layer, x, 0);
            else
                *a.status = HNSW_ERR_OVERFLOW;
        }
    }
    const size_t row_at = layer == 0 ? (size_t)x * S : ((size_t)v.upper_base[x] + layer - 1) * S;
    uint32_t *row = (layer == 0 ? a.adj0_mut : a.adj_up_mut) + row_at;
    uint32_t *rowd = layer == 0 ? a.adjd0_mut : a.adjd_up_mut;  // the edges' distances move with their ids
    if (rowd != nullptr) rowd += row_at;
    uint32_t cur[RS], curd[RS];
    uint32_t deg = 0;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const uint32_t slot = 64u * r + (uint32_t)lane;
        cur[r] = slot < S ? row[slot] : HX_EMPTY_SLOT;
        curd[r] = (rowd != nullptr && slot < S) ? rowd[slot] : 0xFFFFFFFFu;
        deg += (uint32_t)__popcll(__ballot(cur[r] != HX_EMPTY_SLOT));
    }
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t nb = (uint32_t)(a.keys[lo + j] & HX_EDGE_ID_MASK);
        u64 hit = 0;
#pragma unroll
        for (int r = 0; r < RS; r++) hit |= __ballot(cur[r] == nb);
        if (hit == 0) continue;
        if (deg == 1) {  // the last edge stays
            if (lane == 0) {
                const uint32_t at = atomicAdd(a.out_count, 1u);
                if (at < a.out_cap)
                    a.out_keys[at] = hx_edge_key(layer, x, nb);
                else
                    *a.status = HNSW_ERR_OVERFLOW;
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < RS; r++)
            if (cur[r] == nb) cur[r] = HX_EMPTY_SLOT;
        deg--;
    }
    // compact: survivors to the front, every slot written by exactly one lane
    uint32_t before = 0;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const u64 hm = __ballot(cur[r] != HX_EMPTY_SLOT);
        if (cur[r] != HX_EMPTY_SLOT) {
            const uint32_t at = before + (uint32_t)__popcll(hm & ((1ull << lane) - 1));
            row[at] = cur[r];
            if (rowd != nullptr) rowd[at] = curd[r];
        }
        before += (uint32_t)__popcll(hm);
    }
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const uint32_t slot = 64u * r + (uint32_t)lane;
        if (slot >= before && slot < S) {
            row[slot] = HX_EMPTY_SLOT;
            if (rowd != nullptr) rowd[slot] = 0xFFFFFFFFu;
        }
    }
}

// RS = 1 has the configs' dimensions with compile-time row loops; the wide-row instantiations (m = 64 / 128) exist for
// the dimension-generic loops only: one compile-time dimension per row width would triple the build time of this file
// for shapes nobody has measured
template <int RS>
static int launch_connect_rs(const DevView &v, const ConnectArgs &a, hipStream_t stream) {
    const size_t lds = 2 * 64 * RS * 8 + query_lds_bytes(v);
    void (*kfn)(const DevView, const ConnectArgs);
    if (v.kind == HNSW_VEC_QUANT8) {
        kfn = hx_connect_kernel<HNSW_VEC_QUANT8, 0, RS>;
        if constexpr (RS == 1)
            kfn = v.dim == 100   ? hx_connect_kernel<HNSW_VEC_QUANT8, 100, RS>
                  : v.dim == 128 ? hx_connect_kernel<HNSW_VEC_QUANT8, 128, RS>
                  : v.dim == 256 ? hx_connect_kernel<HNSW_VEC_QUANT8, 256, RS>
                  : v.dim == 768 ? hx_connect_kernel<HNSW_VEC_QUANT8, 768, RS>
                                 : kfn;
    } else {
        kfn = hx_connect_kernel<HNSW_VEC_F32, 0, RS>;
        if constexpr (RS == 1)
            kfn = v.dim == 100   ? hx_connect_kernel<HNSW_VEC_F32, 100, RS>
                  : v.dim == 128 ? hx_connect_kernel<HNSW_VEC_F32, 128, RS>
                                 : kfn;
    }
    return launch_checked({"connect kernel launch"}, kfn, dim3(a.count), dim3(64), lds, stream, v, a);
}

int launch_connect(const DevView &v, const ConnectArgs &a, hipStream_t stream) {
    if (a.count == 0) return HNSW_OK;
    const uint32_t S = std::max(v.S0, v.S1);
    if (S <= 64) return launch_connect_rs<1>(v, a, stream);
    if (S <= 128) return launch_connect_rs<2>(v, a, stream);
    if (S <= 256) return launch_connect_rs<4>(v, a, stream);
    set_error("on-device build: adjacency rows of %u slots (m > 128)", S);
    return HNSW_ERR_ARG;
}

int launch_remove(const DevView &v, const ConnectArgs &a, hipStream_t stream) {
    if (a.count == 0) return HNSW_OK;
    const uint32_t S = std::max(v.S0, v.S1);
    if (S > 256) {
        set_error("on-device build: adjacency rows of %u slots (m > 128)", S);
        return HNSW_ERR_ARG;
    }
    return launch_checked({"remove kernel launch"}, S <= 64 ? hx_remove_kernel<1> : S <= 128 ? hx_remove_kernel<2> : hx_remove_kernel<4>,
                          dim3(a.count), dim3(64), 0, stream, v, a);
}

int launch_scatter_rows(uint32_t *dst, uint32_t S, const uint32_t *d_row_index, const uint32_t *d_data,
                        uint32_t n, hipStream_t stream) {
    if (n == 0) return HNSW_OK;
    return launch_checked({"scatter kernel launch"}, hx_scatter_rows_kernel, dim3(n), dim3(64), 0, stream, dst, S, d_row_index,
                          d_data, n);
}

}  // namespace hx
