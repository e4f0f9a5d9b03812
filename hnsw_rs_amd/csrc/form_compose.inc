// form_compose.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's third form: query rows composed out of stored rows.
// ---------------------------------------------------------------------------------------------
// The kernel's third form (DiverseLists with width != 0, list_forms.h; DESIGN.md section 27): query blockIdx.x's row
// composed out of stored rows, one wave per query.  Lane s holds slot s's id and weight; presence and range are ballots,
// decided before any row is read, and the present slots are walked by readlane so that a term's row base is the wave's.
// The element loop is the outer one (e = lane, lane + 64, ...: one accumulator register for any dimension), the terms
// the inner one, in batches of HX_COMPOSE_BATCH whose loads are all issued before the first is folded: the fold order
// is the contract's (slot order, acc = w * x first, then acc = acc + (w * x); never contracted), the loads are
// independent.  A QUANT8 element e sits at byte 8 + i of half hh (stage_query's mapping) and is dequantised with that
// half's own header, as stage_row does.  No LDS, no atomics, no dist_any_dim; every output word is written once.
// ---------------------------------------------------------------------------------------------
#define HX_COMPOSE_BATCH 4
template <int KIND>
__device__ __forceinline__ void compose_rows(const DevView &v, const DiverseLists &d, int lane) {
    const uint32_t q = blockIdx.x, width = d.width, dim = v.dim;
    if (q >= d.nq || width > HX_FROM_ROWS_MAX_TERMS) return;  // (the launcher's limits)
    const bool slot = (uint32_t)lane < width;
    const uint32_t id = slot ? d.ids[(size_t)q * width + lane] : HX_EMPTY_SLOT;
    const float w = slot && d.weights ? d.weights[(size_t)q * width + lane] : 1.0f;
    const u64 present = __ballot(id != HX_EMPTY_SLOT);
    const u64 beyond = __ballot(id != HX_EMPTY_SLOT && id >= v.n_points);
    const bool fail = present == 0 || beyond != 0;  // wave-uniform
    float *out = d.rows_out + (size_t)q * dim;
    if (lane == 0 && d.row_status) d.row_status[q] = fail ? HNSW_ERR_ARG : HNSW_OK;
    if (fail) {  // no row of the index is read for this query
        for (uint32_t e = lane; e < dim; e += 64) out[e] = 0.0f;
        return;
    }
    const uint32_t full = dim & ~7u;
    for (uint32_t e0 = 0; e0 < dim; e0 += 64) {
        const uint32_t e = e0 + lane;
        const bool active = e < dim;
        size_t off;  // this lane's element inside a row, the same for every term
        uint32_t hdr = 0;
        if (KIND == HNSW_VEC_QUANT8) {
            const uint32_t hh = e < full ? (e & 7) >> 2 : 0u;
            const uint32_t i = e < full ? 4 * (e >> 3) + (e & 3) : v.nch4 + (e - full);
            hdr = hh * v.half_bytes;
            off = (size_t)hdr + 8 + i;
        } else {
            off = (size_t)e * 4;
        }
        float acc = 0.0f;
        bool first = true;  // wave-uniform
        u64 rest = present;
        while (rest) {
            float x[HX_COMPOSE_BATCH], ww[HX_COMPOSE_BATCH];
            int nb = 0;  // wave-uniform
#pragma unroll
            for (int t = 0; t < HX_COMPOSE_BATCH; t++) {
                x[t] = 0.0f, ww[t] = 0.0f;
                if (rest) {
                    const int s = __builtin_ctzll(rest);
                    rest &= rest - 1;
                    const uint32_t sid = (uint32_t)__builtin_amdgcn_readlane((int)id, s);  // < v.n_points
                    ww[t] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), s));
                    const uint8_t *row = v.rows + (size_t)sid * v.row_stride;
                    if (active) {
                        if (KIND == HNSW_VEC_QUANT8) {
                            const float mn = *reinterpret_cast<const float *>(row + hdr);
                            const float delta = *reinterpret_cast<const float *>(row + hdr + 4);
                            x[t] = ((float)row[off] * delta) + mn;
                        } else {
                            x[t] = *reinterpret_cast<const float *>(row + off);
                        }
                    }
                    nb = t + 1;
                }
            }
#pragma unroll
            for (int t = 0; t < HX_COMPOSE_BATCH; t++) {
                if (t < nb) {
                    const float p = ww[t] * x[t];
                    acc = first ? p : acc + p;
                    first = false;
                }
            }
        }
        if (active) out[e] = acc;
    }
}
