// exact_scan.hip -- the exact scans under the index's own metric, gfx950: hx_brute_kernel (the reference's ground truth,
// every query against all points) and hx_distance_kernel (dist2many for one query, a test seam), with their launchers.
// Same staged query, same row distance (dist_any_dim) and same sorted list (WaveList) as the search kernels:
// search_common.h.  The MFMA screen of hnsw_brute_force_fast is brute_mfma.hip.

#include <algorithm>

#include "device_index.h"
#include "launch.h"
#include "search_common.h"

namespace hx {

// ---------------------------------------------------------------------------------------------
// distance_batch: VecBase::dist2many (vectors/src/lib.rs:17-22) for one query -- the search
// kernel restricted to "evaluate these ids": every id is an entry, results come back in list
// order, so this launcher runs the kernel with ef = n = k and then un-sorts on the host side.
// (Kept simple on purpose: it is a test seam, not a hot path.)
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(64)
hx_distance_kernel(const DevView v, const float *q, const uint32_t *ids, uint64_t k, float *out,
                   int32_t *status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *yq = reinterpret_cast<float *>(smem);
    const int lane = threadIdx.x;
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
                          dim3(grid), dim3(64), query_lds_bytes(v), stream, v, d_q, d_ids, k, d_out, d_status);
}

}  // namespace hx
