// search_filtered16.hip -- filtered k-NN over an HNSW_VEC_F32 index whose snapshot keeps its rows as IEEE binary16 (option
// "rows_f16"; DESIGN.md sections 36 and 37): hx_filt16_graph_kernel, hx_filt16_scan_kernel, their launchers, and nothing
// else.  launch_filtered_graph and launch_filtered_exact* (search_filtered.hip) route every view with v.rows16 set here;
// the planner, the compaction and the merge read no vector rows and stay where they are.
//
// The walk is hx_filt_graph_kernel's: one wave per query, the unfiltered greedy upper walk, the two sorted register lists
// F and R (FList, search_filtered_dev.h), admission against the bound at the start of a pass, filt_allowed's test in all
// its forms, the overflow status of a full visited table.  What is new is how a pass's rows reach their sums (rows16.inc):
// half the bytes per row, a cooperative whole-line gather where the row is whole lines, widened exactly into the
// reference's own f32 chain -- so ids, distance bits, counts, counters and paths are those of the plain f32 index over the
// widened rows under the same filter.
//
// And the order of the filter's reads.  In the f32 kernel the allow test of an admitted key is a dependent round trip
// AFTER the distances (a label or a mask word, then a word of the deleted set).  Here the words of a pass's fresh ids are
// requested BEFORE the first stage of their rows (filt16_request) and tested when the sums are there (filt16_decide): the
// gather is several stages deep, the words ride in front of it in the same queue, and admission never waits for memory.
// A fresh id that is then not admitted has had its word read for nothing -- four to twenty bytes beside a row of 256 to
// 1536; results and counters cannot depend on it, the counters count distances, expansions and degrees.
//
// Built without packed-f32 instructions (Makefile): every operation below is the scalar IEEE one.

#include <algorithm>

#include "launch.h"
#include "search_filtered_dev.h"

namespace hx {

#include "rows16.inc"

static_assert(HX_FILT16_GATHER_LDS == HX_COOP_IMG_BYTES + 256, "the stage image and the 64 rank words");

// bytes of the region the merges' permutation buffer shares with the gather's image + rank words (never live together:
// a distance pass ends before its merges start); filt_region_bytes (search_filtered.h) is the host's statement of it
template <int DS, int R>
__host__ __device__ constexpr uint32_t filt16_region() {
    return coop_rows16<DS>() && 64u * R * 8u < HX_FILT16_GATHER_LDS ? (uint32_t)HX_FILT16_GATHER_LDS : 64u * R * 8u;
}

// ---------------------------------------------------------------------------------------------
// filt_allowed (search_filtered_dev.h) in two halves: the words an id's test reads from HBM, requested early, and the
// test itself over them.  An id at or beyond the bound reads nothing, as there; under a range AND a row the row's word
// is requested with the label instead of after it (any id below the bound lies inside the row).  A word that is not
// needed keeps a value that passes: every bit set for the mask, none for the deleted set.
// ---------------------------------------------------------------------------------------------
struct FiltWords {
    uint32_t label;
    uint64_t mword, dword;
};

__device__ __forceinline__ FiltWords filt16_request(const uint64_t *deny, uint32_t deny_n, const uint64_t *filt, uint32_t bound,
                                                    const uint32_t *range, uint32_t id, bool want) {
    FiltWords w{0u, ~0ull, 0ull};
    if (!want || id >= bound) return w;
    if ((uintptr_t)filt & 1) {
        w.label = reinterpret_cast<const uint32_t *>((uintptr_t)filt & ~(uintptr_t)3)[id];
        if (!((uintptr_t)filt & 2)) {
            const uint2 rw = *reinterpret_cast<const uint2 *>(range + 2);
            const uint64_t *row = reinterpret_cast<const uint64_t *>(((uint64_t)rw.y << 32) | rw.x);
            if (row) w.mword = row[id >> 6];
        }
    } else if (filt) {
        w.mword = filt[id >> 6];
    }
    if (id < deny_n) w.dword = deny[id >> 6];
    return w;
}

__device__ __forceinline__ bool filt16_decide(const FiltWords &w, const uint64_t *filt, uint32_t bound, const uint32_t *range,
                                              uint32_t id) {
    if (id >= bound) return false;
    if ((uintptr_t)filt & 1) {
        const uint4 r = *reinterpret_cast<const uint4 *>(range);
        bool in = w.label - r.x <= r.y;  // lo <= label <= hi in one unsigned compare
        if ((uintptr_t)filt & 2) {
            for (uint32_t j = 1; j < r.z && !in; j++) {
                const uint2 m = *reinterpret_cast<const uint2 *>(range + 4 + 2 * j);
                in = w.label - m.x <= m.y;
            }
        }
        if (!in) return false;
    }
    return ((w.mword >> (id & 63)) & 1ull) != 0 && ((w.dword >> (id & 63)) & 1ull) == 0;
}

// ---------------------------------------------------------------------------------------------
// Graph path.  LDS: visited table (4 << slots_log2 bytes) | the region: merge buffer (64 R keys), and under rows of whole
// lines the gather's 4-KiB stage image + 64 rank words in the same bytes | query | under a label range, the wave's range
// (HX_FILT_RANGE_LDS bytes) | under K > 1 ranges, its K members (8 K bytes): filt_range_lds.
// DS: the dimension when the rows are gathered cooperatively (128, 256, 768), 0: a lane per row, any dimension.
// ---------------------------------------------------------------------------------------------
template <int DS, int R>
__global__ void __launch_bounds__(64) hx_filt16_graph_kernel(const DevView v, const FilterArgs a, const uint32_t slots_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const uint32_t q = a.qsel ? a.qsel[blockIdx.x] : blockIdx.x;
    // ---- the wave's filter, picked once as hx_filt_graph_kernel picks it (the comments are there) ----
    const uint32_t g = a.mask_of ? a.mask_of[q] : 0;
    const bool bad_row = a.mask_of && g != HNSW_MASK_NONE && g >= a.n_masks;
    const uint64_t *row = g == HNSW_MASK_NONE ? nullptr : a.allow + (size_t)g * a.mask_words;
    const uint64_t *allow = a.labels ? reinterpret_cast<const uint64_t *>((uintptr_t)a.labels | 1) : row;
    uint32_t lo = 0u, hi = 0u;
    constexpr uint32_t YQ_BYTES = DS == 0 ? 0u : DS * 4u;
    unsigned char *region = smem + (4ull << slots_log2);
    float *yq = reinterpret_cast<float *>(region + filt16_region<DS, R>());
    uint32_t *range = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(yq) + (YQ_BYTES ? YQ_BYTES : query_lds_bytes(v)));
    if ((uintptr_t)a.labels & 2) {
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
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(f < 64u ? fl : 1u));
        hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(f < 64u ? fh : 0u));
    } else if (a.labels) {
        lo = a.range_lo[q], hi = a.range_hi[q];
    }
    const uint64_t ids = g == HNSW_MASK_NONE ? a.none_bits : a.allow_bits;
    const uint32_t bound = bad_row || lo > hi ? 0u : (uint32_t)min(a.labels ? min(ids, a.label_len) : ids, (uint64_t)HX_EMPTY_SLOT);
    const uint32_t deny_n = a.deny ? (uint32_t)min(a.deny_bits, (uint64_t)HX_EMPTY_SLOT) : 0u;
    uint32_t *htab = reinterpret_cast<uint32_t *>(smem);
    u64 *perm = reinterpret_cast<u64 *>(region);
    unsigned char *coop_img = region;
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(region + HX_COOP_IMG_BYTES);
    if (a.labels && lane == 0) {  // (read after the wave_fence of the first clear_visited)
        const uintptr_t rw = (uintptr_t)a.labels & 2 ? (uintptr_t)a.n_ranges : (uintptr_t)row;
        *reinterpret_cast<uint4 *>(range) = make_uint4(lo, hi - lo, (uint32_t)rw, (uint32_t)(rw >> 32));
    }
    const uint32_t vis_limit = filt_visited_limit(slots_log2);
    const uint32_t np = v.row_stride >> 4;
    const uint32_t ef = a.ef;

    uint32_t n_dist = 0, n_exp = 0, sum_deg = 0, n_vis = 0;
    int32_t status = stage_query<HNSW_VEC_F32>(v, a.Q + (size_t)q * v.dim, yq, lane) ? HNSW_OK : HNSW_ERR_NAN_INPUT;
    if (bad_row) status = HNSW_ERR_ARG;

    auto clear_visited = [&]() {
        for (uint32_t s = lane; s < (1u << (slots_log2 - 2)); s += 64)
            reinterpret_cast<uint4 *>(htab)[s] = make_uint4(HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT, HX_EMPTY_SLOT);
        wave_fence();
        n_vis = 0;
    };
    // key of this lane's id, FKEY_INVALID when not fresh; every lane calls it (the gather is the whole wave's); a NaN
    // distance sets the status
    auto eval_key = [&](uint32_t id, bool fresh) __attribute__((always_inline)) -> u64 {
        float sm = 0.0f;
        if constexpr (coop_rows16<DS>()) {
            sm = f16_rows_coop<(DS > 0 ? DS : 64)>(v.rows, id, fresh, yq, coop_ids, coop_img, lane);
        } else if (fresh) {
            sm = f16_row_lane(v.rows + (size_t)id * v.row_stride, v.dim, np, yq);
        }
        const float dist = __builtin_sqrtf(sm);
        if (!fresh) return FKEY_INVALID;
        if (dist != dist) {
            status = HNSW_ERR_NAN_INPUT;
            return FKEY_INVALID;
        }
        return ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id;
    };
    // One pass over up to 64 ids of a row: visited filter, with `filtered` the request for the fresh ids' filter words,
    // the distances, then body(key, words) with the fresh keys.  The table's room is checked before the ids are inserted.
    auto pass = [&](uint32_t nb, bool valid, bool filtered, auto &&body) __attribute__((always_inline)) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
        if (cnt == 0) return;
        sum_deg += cnt;
        if (n_vis + cnt > vis_limit) {
            status = HNSW_ERR_OVERFLOW;
            return;
        }
        bool f = false;
        if (valid) f = filt_visit(htab, slots_log2, nb);
        const uint32_t nf = (uint32_t)__popcll(__ballot(f));
        n_vis += nf;
        if (nf == 0) return;
        n_dist += nf;
        const FiltWords fw = filt16_request(a.deny, deny_n, allow, bound, range, nb, f && filtered);
        const u64 key = eval_key(nb, f);
        if (__ballot(status != HNSW_OK)) {
            status = HNSW_ERR_NAN_INPUT;
            return;
        }
        body(key, fw);
    };
    // every neighbour of node cid on a layer, 64 ids per pass: the row, then its overflow list
    auto expand = [&](uint32_t cid, int layer, auto &&body) __attribute__((always_inline)) {
        const uint32_t *arow;
        uint32_t S;
        if (layer == 0) {
            S = v.S0;
            arow = v.adj0 + (size_t)cid * S;
        } else {
            S = v.S1;
            const uint32_t ub = v.upper_base[cid];
            if (ub == HX_EMPTY_SLOT) {  // Graph::neighbors_vec -> NodeNotInGraph
                status = HNSW_ERR_NODE_NOT_IN_GRAPH;
                return;
            }
            arow = v.adj_up + ((size_t)ub + layer - 1) * S;
        }
        n_exp++;
        uint32_t ovf = HX_EMPTY_SLOT;
        for (uint32_t c0 = 0; c0 < S && status == HNSW_OK; c0 += 64) {
            const uint32_t slot = c0 + (uint32_t)lane;
            const uint32_t nb = slot < S ? arow[slot] : HX_EMPTY_SLOT;
            const bool is_ptr = nb != HX_EMPTY_SLOT && (nb & HX_OVF_FLAG);
            const u64 pm = __ballot(is_ptr);
            if (pm) ovf = (uint32_t)__builtin_amdgcn_readlane((int)nb, __ffsll((long long)pm) - 1) & ~HX_OVF_FLAG;
            pass(nb, nb != HX_EMPTY_SLOT && !is_ptr, layer == 0, body);
        }
        if (status == HNSW_OK && ovf != HX_EMPTY_SLOT) {  // degree > S: the rest of the row
            const uint32_t olo = v.ovf_off[ovf], ohi = v.ovf_off[ovf + 1];
            for (uint32_t base = olo; base < ohi && status == HNSW_OK; base += 64) {
                const uint32_t i = base + (uint32_t)lane;
                pass(i < ohi ? v.ovf_nbrs[i] : HX_EMPTY_SLOT, i < ohi, layer == 0, body);
            }
        }
    };

    FList<R> F, Rl;
    F.clear();
    Rl.clear();
    if (status == HNSW_OK) {
        // ---- entry point and the upper layers: the greedy ef = 1 walk, unfiltered ----
        const u64 ek = eval_key(v.ep, lane == 0);
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
                expand((uint32_t)before, layer, [&](u64 key, const FiltWords &) { best = min(best, wave_min64(key)); });
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
            expand((uint32_t)c, 0, [&](u64 key, const FiltWords &fw) {
                // admitted against the bound at the start of the pass; R takes the allowed ones, decided over the words
                // that came in ahead of the rows
                const bool adm = key != FKEY_INVALID && (!Rl.full(ef) || key < Rl.last);
                const bool alw = adm && filt16_decide(fw, allow, bound, range, (uint32_t)key);
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
        a.out_dists[(size_t)q * a.n + lane] = have ? __builtin_bit_cast(float, (uint32_t)(Rl.L[0] >> 32)) : __builtin_inff();
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
// Exact path: hx_filt_scan_kernel's block (seg, y) over f16 rows -- the n best of query y's segment of the list into
// part[(y nseg + seg) n + i], the grouped form (qtab) as there; hx_filt_merge_kernel runs behind it unchanged.  Every
// pass wants all 64 lanes' rows: the lanes of a chunk are a prefix of the wave, a lane's rank is its number, and the
// gather is the four-lanes-per-row round every time (the last chunk of a segment has 1 .. 64 rows; a rank past the end
// repeats the last row).  The ids of the next chunk are requested a pass ahead, so that the gather's addresses never
// wait for the list.  LDS: the region (64 keys, or the image + rank words) | query.
// ---------------------------------------------------------------------------------------------
template <int DS>
__global__ void __launch_bounds__(64) hx_filt16_scan_kernel(const DevView v, const FilterArgs a, const uint32_t *ids, uint32_t A,
                                                            uint32_t nseg, u64 *part, int32_t *part_status,
                                                            const ExactQuery *qtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *perm = reinterpret_cast<u64 *>(smem);
    unsigned char *coop_img = smem;
    uint32_t *coop_ids = reinterpret_cast<uint32_t *>(smem + HX_COOP_IMG_BYTES);
    float *yq = reinterpret_cast<float *>(smem + filt16_region<DS, 1>());
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
    const uint32_t np = v.row_stride >> 4;
    bool bad = !stage_query<HNSW_VEC_F32>(v, a.Q + (size_t)q * v.dim, yq, lane);
    FList<1> wl;
    wl.clear();
    const uint32_t per = (A + nseg - 1) / nseg;
    const uint32_t lo = min(A, per * seg), hi = min(A, lo + per);
    uint32_t nx = lo + (uint32_t)lane < hi ? ids[lo + lane] : 0u;
    for (uint32_t base = lo; base < hi && !bad; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        const bool active = i < hi;
        const uint32_t id = nx;
        if (base + 64 < hi) nx = i + 64 < hi ? ids[i + 64] : 0u;
        float sm = 0.0f;
        if constexpr (coop_rows16<DS>()) {
            if (active) coop_ids[lane] = id;
            wave_fence();
            sm = f16_rows_coop_round<(DS > 0 ? DS : 64), 4>(v.rows, active, (uint32_t)lane, min(64u, hi - base), yq, coop_ids,
                                                           coop_img, lane);
        } else if (active) {
            sm = f16_row_lane(v.rows + (size_t)id * v.row_stride, v.dim, np, yq);
        }
        const float dist = __builtin_sqrtf(sm);
        u64 key = FKEY_INVALID;
        if (active) {
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

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
namespace {

bool f16_view(const DevView &v) {
    if (v.kind == HNSW_VEC_F32 && v.rows16 && v.row_stride == f16_row_stride(v.dim)) return true;
    set_error("filtered search over f16 rows: the snapshot does not hold f16 rows");
    return false;
}

template <int DS, int R>
int launch_graph16_one(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    const size_t lds = (4ull << slots_log2) + filt16_region<DS, R>() + query_lds_bytes(v) + filt_range_lds(a.labels != nullptr, a.n_ranges);
    return launch_checked({"filtered search kernel launch (f16 rows)", "filtered search over f16 rows needs %zu bytes of LDS (> 160 KiB)"},
                          hx_filt16_graph_kernel<DS, R>, dim3(nblocks), dim3(64), lds, stream, v, a, slots_log2);
}

template <int DS>
int launch_graph16(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    if (a.ef <= 64) return launch_graph16_one<DS, 1>(v, a, nblocks, slots_log2, stream);
    if (a.ef <= 128) return launch_graph16_one<DS, 2>(v, a, nblocks, slots_log2, stream);
    return launch_graph16_one<DS, 4>(v, a, nblocks, slots_log2, stream);
}

template <int DS>
int launch_scan16(const DevView &v, const FilterArgs &a, uint32_t grid_seg, uint32_t nsel, const uint32_t *ids, uint32_t A,
                  uint32_t nseg, u64 *part, int32_t *part_status, const ExactQuery *qtab, hipStream_t stream) {
    return launch_checked({"filtered exact search launch (f16 rows)"}, hx_filt16_scan_kernel<DS>, dim3(grid_seg, nsel), dim3(64),
                          filt16_region<DS, 1>() + (size_t)query_lds_bytes(v), stream, v, a, ids, A, nseg, part, part_status, qtab);
}

}  // namespace

// (the arguments were checked by launch_filtered_graph, which also tagged the column's pointer under K > 1 ranges)
int launch_filtered_graph_rows16(const DevView &v, const FilterArgs &a, uint32_t nblocks, uint32_t slots_log2, hipStream_t stream) {
    if (!f16_view(v) || a.ef == 0 || a.ef > HX_FILT_MAX_EF || slots_log2 < 12 || slots_log2 > HX_FILT_MAX_SLOTS_LOG2) return HNSW_ERR_ARG;
    if (v.dim == 128) return launch_graph16<128>(v, a, nblocks, slots_log2, stream);
    if (v.dim == 256) return launch_graph16<256>(v, a, nblocks, slots_log2, stream);
    if (v.dim == 768) return launch_graph16<768>(v, a, nblocks, slots_log2, stream);
    return launch_graph16<0>(v, a, nblocks, slots_log2, stream);
}

int launch_filtered_scan_rows16(const DevView &v, const FilterArgs &a, uint32_t grid_seg, uint32_t nsel, const uint32_t *ids,
                                uint32_t A, uint32_t nseg, unsigned long long *part, int32_t *part_status, const ExactQuery *qtab,
                                hipStream_t stream) {
    if (!f16_view(v)) return HNSW_ERR_ARG;
    if (v.dim == 128) return launch_scan16<128>(v, a, grid_seg, nsel, ids, A, nseg, part, part_status, qtab, stream);
    if (v.dim == 256) return launch_scan16<256>(v, a, grid_seg, nsel, ids, A, nseg, part, part_status, qtab, stream);
    if (v.dim == 768) return launch_scan16<768>(v, a, grid_seg, nsel, ids, A, nseg, part, part_status, qtab, stream);
    return launch_scan16<0>(v, a, grid_seg, nsel, ids, A, nseg, part, part_status, qtab, stream);
}

}  // namespace hx
