// build_kernels16.hip -- the on-device index build over an HNSW_VEC_F32 index whose snapshot keeps its rows as IEEE
// binary16 (option "rows_f16"; DESIGN.md sections 36 and 39): hx_insert16_kernel, hx_connect16_kernel, their launchers,
// and nothing else (libhnsw_mi355x_build16.so).  launch_insert and launch_connect (build_kernels.hip) check the
// arguments, size the visited table and the LDS, and route every view with v.rows16 set here; hx_remove_kernel and
// hx_scatter_rows_kernel read no vector rows and serve such a view from the main library as they are.
//
// The algorithm is hx_insert_kernel's / hx_connect_kernel's (build_kernels.hip) for FullVec rows, statement for statement:
// one wave per point, the 512-entry WaveList, the LDS visited table, the greedy descent, search_layer(ef_cons), the
// heuristic's extension (two entries per pass on rows of up to 32 slots), the windowed sweep, keep_pruned, one atomic add
// for the record slots, the same InsertArgs, outputs, counters and statuses.  The bodies are written out here rather than
// shared through an .inc: the f32 file's device code stays byte for byte what it was.  What is new is how a row reaches
// its sum (rows16.inc): two bytes per element from HBM, widened exactly into the reference's own f32 chain -- so every
// distance has the bits the f32 kernels give over the widened rows, and every decision of the searches, the heuristic
// and the prunes is theirs.
//
//   staged rows   yq (the point) and yqe (a sweep's selected point) stay f32 in LDS -- every chain reads f32 y -- and
//                 are widened from the stored row by stage_row16.  The LDS budget is the f32 kernel's.
//   process       d = 128 / 256 / 768: f16_rows_coop<DS>, the stage image in perm, the rank words behind the staged
//                 rows.  Up to 32 fresh ids: eight lanes to a line; the extension's two-entry pass can want 64 rows and
//                 takes the four-lane round (f16_rows_coop chooses by the count).  Any other d: f16_row_lane.
//   the sweep     the same gather against yqe; a list register's open candidates are ranked by the ballot.
//   connect       reads vector rows only for edges that predate the build (distance not stored): at most S per row and
//                 rare, so stage_row16 and the lane-per-row form only -- no gathered instantiation.
//
// Built without packed-f32 instructions (Makefile): every operation below is the scalar IEEE one.

#include <algorithm>

#include "device_index.h"
#include "launch.h"
#include "search_common.h"

namespace hx {

#include "rows16.inc"

// Stage a stored binary16 row as the f32 query: one 16-byte piece per lane per step, eight v_cvt_f32_f16, two 16-byte LDS
// writes; the piece that holds the row's end writes only the elements below d (the rest of it is padding).
__device__ __forceinline__ void stage_row16(const DevView &v, uint32_t id, float *yq, int lane) {
    const u32x4 *src = reinterpret_cast<const u32x4 *>(v.rows + (size_t)id * v.row_stride);
    const uint32_t np = v.row_stride >> 4, d = v.dim;
    for (uint32_t pc = (uint32_t)lane; pc < np; pc += 64) {
        const u32x4 w = src[pc];
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
        float x[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f16x2_t hh = __builtin_bit_cast(f16x2_t, ww[i]);
            x[2 * i] = (float)hh.x;
            x[2 * i + 1] = (float)hh.y;
        }
        const uint32_t e0 = 8 * pc;
        if (e0 + 8 <= d) {
            *reinterpret_cast<float4 *>(yq + e0) = make_float4(x[0], x[1], x[2], x[3]);
            *reinterpret_cast<float4 *>(yq + e0 + 4) = make_float4(x[4], x[5], x[6], x[7]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++)
                if (e0 + j < d) yq[e0 + j] = x[j];
        }
    }
    wave_fence();
}

// DS: the dimension when the rows are gathered cooperatively (128, 256, 768), 0: a lane per row, any dimension
template <int DS>
__global__ void __launch_bounds__(64)
hx_insert16_kernel(const DevView v, const InsertArgs a, const uint32_t slots_log2) {
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
    const uint32_t yq_bytes = (v.dim * 4u + 15u) & ~15u;         // == query_lds_bytes(v): the launcher reserves that
    float *yq = reinterpret_cast<float *>(selk + 128);
    float *yqe = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(yq) + yq_bytes);
    // the gather's stage image lives in perm (4 KiB, used by the merges only, never during a distance pass), the
    // rank -> id words behind the staged rows
    unsigned char *coop_img = reinterpret_cast<unsigned char *>(perm);
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(yqe) + yq_bytes);
    static_assert(64 * R * 8 >= (int)HX_COOP_IMG_BYTES, "perm holds the stage image");
    const uint32_t np = v.row_stride >> 4;

    int32_t status = HNSW_OK;
    uint32_t n_vis = 0;
    // what this point's insertion reads, counted as hx_insert_kernel counts it: vector rows (distance evaluations +
    // staged rows), adjacency rows and the ids in them
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

    stage_row16(v, p, yq, lane);

    WaveList<R> wl;
#pragma unroll
    for (int r = 0; r < R; r++) wl.L[r] = KEY_INVALID;
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;

    // distance of one row per lane to the staged row y; every lane calls it (the gather is the whole wave's)
    auto eval_dist = [&](uint32_t id, bool active, const float *y) __attribute__((always_inline)) -> float {
        float sm = 0.0f;
        if constexpr (coop_rows16<DS>()) {
            sm = f16_rows_coop<(DS > 0 ? DS : 64)>(v.rows, id, active, y, coop_ids, coop_img, lane);
        } else if (active) {
            sm = f16_row_lane(v.rows + (size_t)id * v.row_stride, v.dim, np, y);
        }
        return __builtin_sqrtf(sm);
    };
    // one pass over up to 64 ids: optional visited filter, distance to the staged point, merge
    auto process = [&](uint32_t id, bool valid, bool visit, uint32_t ef_l, u64 new_flag) __attribute__((always_inline)) {
        bool fresh = valid;
        if (visit) fresh = valid && visited_insert(htab, hmask, slots_log2, id);
        const u64 fm = __ballot(fresh);
        if (visit) n_vis += (uint32_t)__popcll(fm);  // what the table really holds
        if (fm == 0) return;
        c_rows += (uint32_t)__popcll(fm);
        const float dist = eval_dist(id, fresh, yq);
        u64 key = KEY_INVALID;
        bool nan = false;
        if (fresh) {
            nan = dist != dist;
            if (!nan) key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
        }
        if (__ballot(nan)) status = HNSW_ERR_NAN_INPUT;
        // the merge runs over the list registers that can hold something (hx_insert_kernel's reasoning)
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
        // The heuristic's extension expands a FIXED set and keeps the union of the neighbours, so on rows of up to 32
        // slots TWO entries go through one pass, one per half wave (the visited insert settles an id both rows hold).
        // Such a pass can want 64 rows: the gather then takes its four-lane round, and one round still serves the pass.
        const bool two = new_flag != 0 && S <= 32;
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
            for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += 64) {
                const uint32_t slot = c0 + (uint32_t)lane;
                uint32_t nb = HX_EMPTY_SLOT;
                if (slot < S) nb = row[slot];
                // during a build the device rows never carry overflow pointers; a flagged id is skipped
                const bool valid = nb != HX_EMPTY_SLOT && !(nb & HX_OVF_FLAG) && nb != p;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
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
    if (status == HNSW_OK) process(v.ep, lane < 1, false, 1u, 0);  // setup_insert

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
        // ---- select_heuristic: candidates = selected ∪ neighbours(selected), distances to p (results.rs:105-146):
        // every current entry is expanded once more, keeping ALL distinct neighbours (cap 512 nearest); entries that
        // arrive now are born expanded.
        begin_layer(64u * R);
        expand_all(layer, 64u * R, KEY_EXPANDED);
        if (status != HNSW_OK) break;
        // Whenever a candidate s is selected, every LATER candidate e with (d(s,e), s) < (d(e,p), e) is marked rejected
        // (d is bit-symmetric); the next selection is the first unmarked one (hx_insert_kernel, searcher.rs:128-139).
        const uint32_t n_c = wl.n_cur;
        uint32_t ns = 0;
        uint32_t selbits = 0;  // bit r: the candidate at position 64 r + lane was selected
#pragma unroll
        for (int r = 0; r < R; r++) wl.L[r] &= KEY_MASK;  // the flag now means "rejected"
        uint32_t cursor = 0;
        // One sweep: the staged selected point (yqe, id sid) against the open candidates at positions [lo, hi).  The open
        // candidates of a list register are not a prefix of the wave: the gather ranks them by their ballot.
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
                const u64 om = __ballot(open);
                if (om == 0) continue;
                c_rows += (uint32_t)__popcll(om);
                const float dist = eval_dist((uint32_t)mine, open, yqe);
                bool rej = false;
                if (open) {
                    if (dist != dist) status = HNSW_ERR_NAN_INPUT;
                    const u64 sk = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | sid;
                    rej = sk < mine;
                }
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (r == rr && rej) wl.L[r] |= KEY_EXPANDED;
            }
        };
        // a selected point sweeps only the WINDOW [0, win_end) of candidates; when the window holds nothing unpopped and
        // fewer than m are selected, it grows by 64 and the points selected so far sweep the new part first
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
                    stage_row16(v, sid2, yqe, lane);
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
            stage_row16(v, sid, yqe, lane);
            sweep(sid, cursor, win_end);
            if (__ballot(status != HNSW_OK)) status = HNSW_ERR_NAN_INPUT;
        }
        // keep_pruned: fill up from the rejected candidates in ascending order (searcher.rs:141-146)
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
        // on-device connect: only a point whose every layer succeeded writes its own rows (nobody can reach p yet) and
        // files one reverse-edge request per selected neighbour
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
        const uint32_t per_edge = a.emit_own ? 2u : 1u;  // (the sharded build's form; kept, as the arguments are)
        total *= per_edge;
        // `total` record slots with ONE atomic add; a reservation that does not fit leaves the counter beyond the
        // capacity for good, and the smallest failing base in *req_fail_base (hx_insert_kernel)
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

// ---------------------------------------------------------------------------------------------
// Phase 2 of the on-device connect over f16 rows: hx_connect_kernel's append / prune of one adjacency row per wave
// (build_kernels.hip), the rare unknown distance evaluated with a lane per row against the node's staged row.
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

// RS = registers per lane that hold one adjacency row (slot 64 r + lane): 1 / 2 / 4 for rows of up to 64 / 128 / 256 slots
template <int RS>
__global__ void __launch_bounds__(64)
hx_connect16_kernel(const DevView v, const ConnectArgs a) {
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
    if (a.own_world > 1) {  // (the sharded build's form; kept, as the arguments are)
        if (n % a.own_world != a.own_rank) return;
        if (lane == 0) {
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
    if (any_unknown) stage_row16(v, n, yq, lane);
    const uint32_t np = v.row_stride >> 4;
    WaveList<RS> wl;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        wl.L[r] = KEY_INVALID;
        ekeys[64 * r + lane] = KEY_INVALID;
    }
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;
    wave_fence();
#pragma unroll
    for (int r = 0; r < RS; r++) {  // existing neighbours, one list register at a time
        const uint32_t slot = 64u * r + (uint32_t)lane;
        if (slot - lane >= S) break;
        const uint32_t id = cur[r];
        uint32_t dbits = curd[r];
        const bool act = slot < S && id < v.n_points;
        if (slot < S && id != HX_EMPTY_SLOT && id >= v.n_points) *a.status = HNSW_ERR_NODE_NOT_IN_GRAPH;
        const bool need = act && dbits == 0xFFFFFFFFu;  // (an edge that predates the build: evaluated once, kept from here on)
        if (need) dbits = __builtin_bit_cast(uint32_t, __builtin_sqrtf(f16_row_lane(v.rows + (size_t)id * v.row_stride, v.dim, np, yq)));
        u64 key = KEY_INVALID;
        if (act) {
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
// launchers: the arguments were checked, the visited table and the LDS sized, by launch_insert / launch_connect
// ---------------------------------------------------------------------------------------------
static bool view_is_rows16(const DevView &v) {
    if (v.kind == HNSW_VEC_F32 && v.rows16 && v.row_stride == f16_row_stride(v.dim)) return true;
    set_error("on-device build over f16 rows: the snapshot does not hold f16 rows");
    return false;
}

int launch_insert_rows16(const DevView &v, const InsertArgs &a, uint32_t nblocks, uint32_t slots_log2, size_t lds,
                         hipStream_t stream) {
    if (!view_is_rows16(v)) return HNSW_ERR_ARG;
    void (*kfn)(const DevView, const InsertArgs, const uint32_t) = v.dim == 128   ? hx_insert16_kernel<128>
                                                                   : v.dim == 256 ? hx_insert16_kernel<256>
                                                                   : v.dim == 768 ? hx_insert16_kernel<768>
                                                                                  : hx_insert16_kernel<0>;
    return launch_checked({"insert kernel launch (f16 rows)", "insert kernel needs %zu bytes of LDS"}, kfn, dim3(nblocks),
                          dim3(64), lds, stream, v, a, slots_log2);
}

int launch_connect_rows16(const DevView &v, const ConnectArgs &a, int rs, hipStream_t stream) {
    if (!view_is_rows16(v)) return HNSW_ERR_ARG;
    const size_t lds = 2 * 64 * (size_t)rs * 8 + query_lds_bytes(v);
    return launch_checked({"connect kernel launch (f16 rows)"},
                          rs == 1 ? hx_connect16_kernel<1> : rs == 2 ? hx_connect16_kernel<2> : hx_connect16_kernel<4>,
                          dim3(a.count), dim3(64), lds, stream, v, a);
}

}  // namespace hx
