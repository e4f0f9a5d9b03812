// exact_scan.hip -- the exact scans under the index's own metric, gfx950, with their launchers: hx_brute_kernel (the
// reference's ground truth, every query against all points) and hx_distance_kernel (dist2many for one query, a test seam,
// and the carrier of the list forms: the post-process stages that work on candidate lists, one wave per query).  A form's
// record and limits are list_forms.h (DiverseLists); its body, LDS layout and LDS size are a file of its own:
//   second   form_diversify.inc    the MMR selection of diversified search: stored rows against a stored row
//   third    form_compose.inc      the query rows composed out of stored rows
//   fourth   form_fuse_lists.inc   the fusion of a query's per-vector candidate lists
//   fifth    form_late.inc         the late interaction that scores those candidates as documents
//   sixth    form_refine.inc       the refinement of a candidate list against a table of full rows
//   seventh  form_late.inc         the scoring of named documents over every stored row they have
//   eighth   form_fuse_ranked.inc  the rank fusion of a query's dense list with external ranked lists under the filters
//   ninth    form_boost.inc        the boost of a candidate list by per-id attributes out of a row table
// Same staged query, same row distance (dist_any_dim) and same sorted list (WaveList) as the search kernels:
// search_common.h.  The MFMA screen of hnsw_brute_force_fast is brute_mfma.hip.

#include <algorithm>

#include "device_index.h"
#include "launch.h"
#include "list_forms.h"
#include "search_common.h"

namespace hx {

// (in definition order: the order the kernel's code is generated in)
#include "form_diversify.inc"
#include "form_compose.inc"
#include "form_fuse_lists.inc"
#include "form_late.inc"
#include "form_refine.inc"
#include "form_boost.inc"
#include "form_fuse_ranked.inc"

// ---------------------------------------------------------------------------------------------
// distance_batch: VecBase::dist2many (vectors/src/lib.rs:17-22) for one query -- the search
// kernel restricted to "evaluate these ids": every id is an entry, results come back in list
// order, so this launcher runs the kernel with ef = n = k and then un-sorts on the host side.
// (Kept simple on purpose: it is a test seam, not a hot path.)
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(64)
hx_distance_kernel(const DevView v, const float *q, const uint32_t *ids, uint64_t k, float *out,
                   int32_t *status_out, const DiverseLists dv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *yq = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
    if (dv.boost) {  // (looked at before all others: the boost sets n_out, table and weights too; launch_boost alone sets it)
        boost_lists(dv, smem, lane);
        return;
    }
    if (dv.hybrid) {  // (looked at before all the rest: the rank fusion sets n_out, and may set ids, labels and queries too)
        fuse_ranked<KIND>(v, dv, yq, smem + query_lds_bytes(v), lane);
        return;
    }
    const bool docs = dv.docs != 0;  // (looked at first of the others: the document scoring, late_interaction's other half)
    if (!docs && dv.table) {  // (looked at first of the others: this form sets n_out too, and reads nothing of v)
        refine_lists(dv, smem, lane);
        return;
    }
    if (docs || dv.late) {  // (looked at first: these forms set n_vecs and n_out too)
        late_interaction<KIND>(v, dv, yq, smem + query_lds_bytes(v), lane);
        return;
    }
    if (dv.n_vecs) {  // (a kernel argument: the branch is the wave's; looked at before n_out, which this form sets too)
        fuse_lists<KIND>(v, dv, yq, smem + query_lds_bytes(v), lane);
        return;
    }
    if (dv.n_out) {
        diversify<KIND>(v, dv, yq, smem + query_lds_bytes(v), lane);
        return;
    }
    if (dv.width) {
        compose_rows<KIND>(v, dv, lane);
        return;
    }
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    int32_t status = stage_query<KIND>(v, q, yq, lane) ? HNSW_OK : HNSW_ERR_NAN_INPUT;
    for (uint64_t base = (uint64_t)blockIdx.x * CHUNK; base < k;
         base += (uint64_t)gridDim.x * CHUNK) {
        const uint64_t i = base + lane / LPC;
        const bool active = i < k;
        const uint32_t id = active ? ids[i] : 0;
        const bool ok = active && id < v.n_points;
        const float dist = dist_any_dim<KIND>(v, id, ok, h, yq);
        if (active && h == 0) {
            if (!ok) status = HNSW_ERR_ARG;
            out[i] = ok ? dist : __builtin_nanf("");
        }
    }
    if (status != HNSW_OK) atomicMin(status_out, status);
}

// ---------------------------------------------------------------------------------------------
// brute force: exact top-k of every query over ALL points under the index's own metric (the
// reference's ground truth: helpers/glove.rs:94-109, template.rs:531-541).  Block (seg, q) scans
// one contiguous segment of the ids and keeps its k best in the same sorted list the search
// uses; the host merges the nseg partial lists of a query.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(64)
hx_brute_kernel(const DevView v, const float *Q, uint32_t k, uint32_t nseg, uint32_t *part_ids,
                float *part_dists, int32_t *status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *perm = reinterpret_cast<u64 *>(smem);
    float *yq = reinterpret_cast<float *>(perm + 64);
    const int lane = threadIdx.x;
    const uint32_t seg = blockIdx.x, q = blockIdx.y;
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    int32_t status = stage_query<KIND>(v, Q + (size_t)q * v.dim, yq, lane) ? HNSW_OK : HNSW_ERR_NAN_INPUT;
    WaveList<1> wl;
    wl.L[0] = KEY_INVALID;
    wl.n_cur = 0;
    wl.last_key = KEY_INVALID;
    const uint64_t per = ((uint64_t)v.n_points + nseg - 1) / nseg;
    const uint64_t lo = per * seg, hi = min((uint64_t)v.n_points, lo + per);
    for (uint64_t base = lo; base < hi; base += CHUNK) {
        const uint64_t i = base + lane / LPC;
        const bool active = i < hi;
        const float dist = dist_any_dim<KIND>(v, (uint32_t)i, active, h, yq);
        u64 key = KEY_INVALID;
        if (active && h == 0) {
            if (dist != dist)
                status = HNSW_ERR_NAN_INPUT;
            else
                key = ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | (uint32_t)i;
        }
        wl.merge(key, k, perm, lane);
    }
    if ((uint32_t)lane < k) {
        const size_t o = ((size_t)q * nseg + seg) * k + lane;
        const bool have = (uint32_t)lane < wl.n_cur;
        part_ids[o] = have ? (uint32_t)wl.L[0] : HX_EMPTY_SLOT;
        part_dists[o] = have ? __builtin_bit_cast(float, (uint32_t)(wl.L[0] >> 32)) : __builtin_inff();
    }
    if (__ballot(status != HNSW_OK) && lane == 0) atomicMin(status_out, HNSW_ERR_NAN_INPUT);
}

int launch_brute_force(const DevView &v, const float *d_Q, uint64_t nq, uint32_t k, uint32_t nseg,
                       uint32_t *part_ids, float *part_dists, int32_t *d_status,
                       hipStream_t stream) {
    if (nq == 0) return HNSW_OK;
    if (k == 0 || k > 64 || nq > 65535) {
        set_error("brute force supports 1 <= k <= 64 and at most 65535 queries per call");
        return HNSW_ERR_ARG;
    }
    return launch_checked({"brute force kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_brute_kernel<HNSW_VEC_QUANT8> : hx_brute_kernel<HNSW_VEC_F32>,
                          dim3(nseg, (uint32_t)nq), dim3(64), 64 * 8 + (size_t)query_lds_bytes(v), stream, v, d_Q, k, nseg,
                          part_ids, part_dists, d_status);
}

int launch_distance_batch(const DevView &v, const float *d_q, const uint32_t *d_ids, uint64_t k,
                          float *d_out, int32_t *d_status, hipStream_t stream) {
    if (k == 0) return HNSW_OK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, (k + 31) / 32);
    return launch_checked({"distance kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(grid), dim3(64), query_lds_bytes(v), stream, v, d_q, d_ids, k, d_out, d_status,
                          DiverseLists{});  // (n_out 0: the first form)
}

// The one launch of a list form: d.nq blocks of one wave under the record d, the instantiation by the view's kind.  The
// seam's own parameters (q, ids, k, out, status_out) are read by no list form.
static int launch_lists(const LaunchSite &site, const DevView &v, size_t lds, const DiverseLists &d, hipStream_t stream) {
    return launch_checked(site,
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), lds, stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
}

// the view of the forms that take no handle and read nothing of it: zeroed, and F32 for the instantiation
static DevView no_view() {
    DevView v{};
    v.kind = HNSW_VEC_F32;
    return v;
}

int launch_diversify(const DevView &v, const DiverseLists &d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_out == 0 || d.n_out > d.pool || d.pool > HX_DIVERSE_POOL_MAX || !(d.lambda >= 0.0f && d.lambda <= 1.0f) ||
        d.nq > 0x7FFFFFFFu || !d.ids || !d.dists || !d.out_ids || !d.out_dists || (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("diversify: needs 1 <= n_out <= pool <= %d, lambda in [0, 1], at most 2^31 - 1 queries, the lists and the "
                  "outputs", HX_DIVERSE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    return launch_lists({"diversify kernel launch"}, v, query_lds_bytes(v) + HX_DIVERSE_LDS, d, stream);
}

int launch_compose_rows(const DevView &v, uint32_t nq, uint32_t width, const uint32_t *d_src_ids, const float *d_weights,
                        float *d_rows, int32_t *d_status, hipStream_t stream) {
    if (nq == 0) return HNSW_OK;
    if (width == 0 || width > HX_FROM_ROWS_MAX_TERMS || nq > 0x7FFFFFFFu || !d_src_ids || !d_rows) {
        set_error("compose rows: needs 1 <= width <= %d, at most 2^31 - 1 queries, the source ids and the query rows",
                  HX_FROM_ROWS_MAX_TERMS);
        return HNSW_ERR_ARG;
    }
    DiverseLists d{};  // (n_out 0: not the second form)
    d.ids = d_src_ids;
    d.nq = nq;
    d.width = width;
    d.weights = d_weights;
    d.rows_out = d_rows;
    d.row_status = d_status;
    return launch_lists({"compose rows kernel launch"}, v, 0, d, stream);
}

int launch_fuse_lists(const DevView &v, const DiverseLists &d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_vecs == 0 || d.n_vecs > HX_MULTI_MAX_VECS || d.pool == 0 || d.pool > HX_DIVERSE_POOL_MAX ||
        d.n_vecs * d.pool > HX_DIVERSE_POOL_MAX || d.n_out == 0 || d.n_out > d.pool || d.mode > HNSW_FUSE_MIN ||
        d.nq > 0x7FFFFFFFu || !d.queries || !d.ids || !d.out_ids || !d.out_dists ||
        (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("fuse lists: needs 1 <= n_vecs <= %d, 1 <= n_out <= pool, n_vecs * pool <= %d, a mode, at most 2^31 - 1 "
                  "queries, the vectors, the lists and the outputs", HX_MULTI_MAX_VECS, HX_DIVERSE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    return launch_lists({"fuse lists kernel launch"}, v, query_lds_bytes(v) + HX_DIVERSE_LDS, d, stream);
}

int launch_late_interaction(const DevView &v, DiverseLists d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    const uint64_t total = (uint64_t)d.n_vecs * d.pool;
    if (d.n_vecs == 0 || d.n_vecs > HX_LATE_MAX_VECS || d.pool == 0 || total > HX_LATE_MAX_CANDS || d.n_out == 0 ||
        d.n_out > total || d.n_out > HX_LATE_MAX_DOCS || d.mode > HNSW_LATE_SUM_SQ || d.nq > 0x7FFFFFFFu || !d.queries ||
        !d.ids || !d.out_ids || !d.out_dists || (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("late interaction: needs 1 <= n_vecs <= %d, n_vecs * pool <= %d, 1 <= n_out <= min(n_vecs * pool, %d), a "
                  "mode, at most 2^31 - 1 queries, the vectors, the lists and the outputs", HX_LATE_MAX_VECS, HX_LATE_MAX_CANDS,
                  HX_LATE_MAX_DOCS);
        return HNSW_ERR_ARG;
    }
    d.late = 1;
    if (!d.labels) d.label_len = 0;  // no column: every label is 0 and nothing is read
    const size_t cap = ((size_t)total + 63) & ~(size_t)63;
    return launch_lists({"late interaction kernel launch", "late interaction: the staged vector and the table need %zu bytes of LDS"},
                        v, query_lds_bytes(v) + HX_LATE_LDS(cap), d, stream);
}

int launch_score_documents(const DevView &v, DiverseLists d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_vecs == 0 || d.n_vecs > HX_LATE_MAX_VECS || d.n_out == 0 || d.n_out > d.pool || d.pool > HX_DOCS_MAX_IN ||
        d.rows_cap == 0 || d.rows_cap > HX_DOCS_MAX_ROWS || d.mode > HNSW_LATE_SUM_SQ || d.nq > 0x7FFFFFFFu || !d.queries ||
        !d.ids || !d.doc_keys || !d.out_ids || !d.out_dists || (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("score documents: needs 1 <= n_vecs <= %d, 1 <= n_out <= n_in <= %d, 1 <= rows_cap <= %u, a mode, at most "
                  "2^31 - 1 queries, the vectors, the labels, the document index and the outputs", HX_LATE_MAX_VECS,
                  HX_DOCS_MAX_IN, HX_DOCS_MAX_ROWS);
        return HNSW_ERR_ARG;
    }
    d.docs = 1;
    d.late = 0, d.table = nullptr;
    return launch_lists({"score documents kernel launch", "score documents: the staged vector and the tables need %zu bytes of LDS"},
                        v, query_lds_bytes(v) + HX_DOCS_LDS(d.pool, d.n_vecs), d, stream);
}

int launch_fuse_ranked(const DevView &v, DiverseLists d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    const uint64_t total = (d.ids ? (uint64_t)d.pool : 0) + (uint64_t)d.n_ext * d.ext_width;
    if (d.n_ext > HX_HYBRID_MAX_EXT || total == 0 || total > HX_DIVERSE_POOL_MAX || d.n_out == 0 || d.n_out > total ||
        d.mode > 1 || (d.mode == 0 && (d.rank_constant == 0 || d.rank_constant > (1u << 20))) ||
        (d.mode == 1 && ((d.n_ext != 0 && !d.ext_scores) || (d.n_ext == 0 && !d.queries))) || (d.n_ext != 0 && !d.ext_ids) ||
        (d.out_gaps && !d.queries) || (d.rowed && d.n_masks != 0 && d.mask_words != 0 && !d.allow) ||
        (d.range_lo != nullptr) != (d.range_hi != nullptr) || d.nq > 0x7FFFFFFFu || !d.out_ids || !d.out_dists ||
        (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("fuse ranked: needs n_ext <= %d, 1 <= n_out <= total <= %d, a mode (with 1 <= rank_constant <= 2^20, or with "
                  "the external scores), the vector with the distances, at most 2^31 - 1 queries, the lists and the outputs",
                  HX_HYBRID_MAX_EXT, HX_DIVERSE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    d.hybrid = 1 + d.mode;
    if (!d.labels) d.label_len = 0;  // no column: every label is 0 and nothing is read
    if (!d.deny) d.deny_bits = 0;
    return launch_lists({"fuse ranked kernel launch"}, v, query_lds_bytes(v) + HX_HYBRID_LDS, d, stream);
}

int launch_refine(DiverseLists d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_out == 0 || d.n_out > d.pool || d.pool > HX_REFINE_POOL_MAX || d.full_dim == 0 || d.full_dim > HX_REFINE_MAX_DIM ||
        d.table_dtype > HX_ROWS_F16 || d.nq > 0x7FFFFFFFu || !d.table || !d.queries || !d.ids || !d.out_ids || !d.out_dists ||
        (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("refine: needs 1 <= n_out <= pool <= %d, 1 <= full_dim <= %d, a dtype of the two, at most 2^31 - 1 queries, "
                  "the table, the full queries, the lists and the outputs", HX_REFINE_POOL_MAX, HX_REFINE_MAX_DIM);
        return HNSW_ERR_ARG;
    }
    d.lane_rows = sw::refine_lane_rows() ? 1u : 0u;
    return launch_lists({"refine kernel launch"}, no_view(), refine_lds_bytes(d.full_dim, d.pool), d, stream);
}

int launch_boost(DiverseLists d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_out == 0 || d.n_out > d.pool || d.pool > HX_BOOST_POOL_MAX || d.full_dim == 0 || d.full_dim > HX_BOOST_MAX_ATTRS ||
        d.table_dtype > HX_ROWS_F16 || d.mode > 1 || d.nq > 0x7FFFFFFFu || !d.table || !d.weights || !d.ids || !d.dists ||
        !d.out_ids || !d.out_dists || (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("boost: needs 1 <= n_out <= pool <= %d, 1 <= n_attrs <= %d, a dtype of the two, one weight row or one per "
                  "query, at most 2^31 - 1 queries, the table, the weights, the lists and the outputs", HX_BOOST_POOL_MAX,
                  HX_BOOST_MAX_ATTRS);
        return HNSW_ERR_ARG;
    }
    d.boost = 1 + d.mode;
    return launch_lists({"boost kernel launch"}, no_view(), boost_lds_bytes(d.full_dim, d.pool), d, stream);
}

}  // namespace hx
