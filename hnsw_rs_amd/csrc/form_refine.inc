// form_refine.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's sixth form: the refinement of a candidate list against a table of full rows.
// ---------------------------------------------------------------------------------------------
// The kernel's sixth form (DiverseLists with table != nullptr, list_forms.h; DESIGN.md section 31): query blockIdx.x's
// candidate list of d.pool ids re-scored against full rows of a table in HBM -- f32, or IEEE binary16 widened exactly --
// and cut to the n_out nearest, one wave per query.  It reads nothing of the DevView.  LDS, with cap = pool rounded up to 64:
//   yq    the full query row, full_dim floats (rounded up to 16 bytes)
//   keys  cap double words: first the present ids (KEY_INVALID: absent), then (distance bits << 32 | id), KEY_INVALID for NaN
//   ids_s 64 words, rank -> row id of the cooperative gather          img  its 4-KiB stage image
// Presence, the incoming status, the range and the query's NaN check are decided (ballots) before any table row is read.
// The distance of an entry is ONE lane's left-to-right f32 chain over all full_dim elements, t = x - y, s += t * t, then
// the square root: host_index.cpp's dist_full.  How the bytes arrive does not touch it:
//   - an f32 row of whole 128-byte lines is gathered as coop_rows.inc gathers them, eight lanes to a line, 32 rows a round
//     and two rounds for a pass's 64 entries; full_dim is a run-time value here, so the stages are a run-time loop with
//     HX_REFINE_K of them in flight (16 registers each), not the compile-time DS templates;
//   - other rows, and every f16 row (where the same gather measured slower than this loop: its owners are half the wave
//     and convert twice the elements a stage), take a lane per row: 16-byte loads where the table and its row stride
//     allow them, element loads otherwise.
// The rank of an entry is the number of keys before it in (key, position) order, counted by an all-pairs compare over
// the table -- two keys a read, the same address in every lane -- so duplicate ids are separate entries and an entry of
// rank r < n_out stores itself at r.  Plain vector stores, no atomics; every output word is written once.
// ---------------------------------------------------------------------------------------------
#ifndef HX_REFINE_K
#define HX_REFINE_K 4
#endif
__host__ __device__ inline size_t refine_lds_bytes(uint32_t full_dim, uint32_t pool) {
    return (((size_t)full_dim * 4 + 15) & ~(size_t)15) + (((size_t)pool + 63) & ~(size_t)63) * 8 + 64 * 4 + HX_COOP_IMG_BYTES;
}
// sixteen bytes of a row against the query values at y, continuing the chain s: four f32 elements, or eight f16
template <bool F16>
__device__ __forceinline__ void refine_fold(const uint4 pp, const float *y, float &s) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    if constexpr (F16) {
        const uint32_t w[4] = {pp.x, pp.y, pp.z, pp.w};
        const float4 y0 = *reinterpret_cast<const float4 *>(y), y1 = *reinterpret_cast<const float4 *>(y + 4);
        const f32x2 yy[4] = {{y0.x, y0.y}, {y0.z, y0.w}, {y1.x, y1.y}, {y1.z, y1.w}};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f32x2 x = __builtin_convertvector(__builtin_bit_cast(f16x2, w[i]), f32x2);  // (exact)
            const f32x2 dd = x - yy[i];
            const f32x2 qq = dd * dd;
            s += qq.x;
            s += qq.y;
        }
    } else {
        const float4 y0 = *reinterpret_cast<const float4 *>(y);
        const f32x2 xa = {__builtin_bit_cast(float, pp.x), __builtin_bit_cast(float, pp.y)};
        const f32x2 xb = {__builtin_bit_cast(float, pp.z), __builtin_bit_cast(float, pp.w)};
        const f32x2 ya = {y0.x, y0.y}, yb = {y0.z, y0.w};
        const f32x2 da = xa - ya, db = xb - yb;
        const f32x2 qa = da * da, qb = db * db;
        s += qa.x;
        s += qa.y;
        s += qb.x;
        s += qb.y;
    }
}
// a lane per row: `wide` (the wave's) says that the row starts on a 16-byte boundary and is whole 16-byte pieces
template <bool F16>
__device__ __forceinline__ float refine_lane_row(const uint8_t *row, uint32_t dim, bool wide, const float *yq) {
    constexpr uint32_t EPP = F16 ? 8 : 4;  // elements per 16-byte piece
    float s = 0.0f;
    if (wide) {
        const uint4 *src = reinterpret_cast<const uint4 *>(row);
        const uint32_t np = dim / EPP;
        uint32_t p = 0;
#pragma unroll 1
        for (; p + 4 <= np; p += 4) {  // four pieces in flight
            const uint4 a = src[p], b = src[p + 1], c = src[p + 2], e = src[p + 3];
            refine_fold<F16>(a, yq + (size_t)p * EPP, s);
            refine_fold<F16>(b, yq + (size_t)(p + 1) * EPP, s);
            refine_fold<F16>(c, yq + (size_t)(p + 2) * EPP, s);
            refine_fold<F16>(e, yq + (size_t)(p + 3) * EPP, s);
        }
#pragma unroll 1
        for (; p < np; p++) refine_fold<F16>(src[p], yq + (size_t)p * EPP, s);
    } else {
#pragma unroll 1
        for (uint32_t e = 0; e < dim; e++) {
            float x;
            if constexpr (F16)
                x = (float)__builtin_bit_cast(_Float16, reinterpret_cast<const uint16_t *>(row)[e]);  // (exact)
            else
                x = reinterpret_cast<const float *>(row)[e];
            const float t = x - yq[e];
            s += t * t;
        }
    }
    return s;
}
// One round of the cooperative gather (f32_rows_coop_round of coop_rows.inc with eight lanes to a line, the stage count
// `ns` a run-time value): the nw <= 32 f32 rows of ids_s, the owner of rank `rank` (`mine`) summing its own row.
__device__ __forceinline__ float refine_coop_round(const uint8_t *table, size_t row_bytes, uint32_t ns, bool mine, uint32_t rank,
                                                   uint32_t nw, const float *yq, const uint32_t *ids_s, unsigned char *img,
                                                   int lane) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // (native: a HIP uint4 would keep the ring in scratch)
    constexpr int K = HX_REFINE_K;
    constexpr uint32_t EPS = 32;  // elements of a row per 128-byte stage
    const uint32_t g = (uint32_t)lane >> 3, t = (uint32_t)lane & 7u;
    const uint8_t *src[4];
    uint32_t wofs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {  // rows of instruction i: rank 8 i + g; a rank past the end repeats the last row
        const uint32_t slot = 8u * i + g;
        const uint32_t rr = min(slot, nw - 1);
        src[i] = table + (size_t)ids_s[rr] * row_bytes + 16u * t;
        wofs[i] = slot * 128u + ((t ^ ((slot >> 1) & 7u)) << 4);
    }
    const unsigned char *rd = img + rank * 128u;
    const uint32_t sw = (rank >> 1) & 7u;
    float s = 0.0f;
    u32x4 w[K][4];
    auto request = [&](int j, uint32_t st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) w[j][i] = *reinterpret_cast<const u32x4 *>(src[i] + (size_t)st * 128u);
    };
    auto to_image = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(img + wofs[i]) = w[j][i];
    };
    auto owners_sum = [&](uint32_t st) __attribute__((always_inline)) {
        if (mine) {
            const float *y = yq + (size_t)st * EPS;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                // (read as a HIP uint4 from the swizzled address: coop_rows.inc, DESIGN.md section 4c)
                const uint4 pp = *reinterpret_cast<const uint4 *>(rd + (((uint32_t)k ^ sw) << 4));
                refine_fold<false>(pp, y + k * (EPS / 8), s);
            }
        }
        // the next stage's image may only be written once every owner has read this one: one wave's LDS operations
        // execute in issue order, the clobber keeps the compiler from moving them across
        asm volatile("" ::: "memory");
    };
#pragma unroll
    for (int j = 0; j < K; j++)
        if ((uint32_t)j < ns) request(j, j);
#pragma unroll 1
    for (uint32_t st0 = 0; st0 < ns; st0 += K) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (st0 + j < ns) {  // (the wave's branch)
                to_image(j);
                if (st0 + K + j < ns) request(j, st0 + K + j);
                owners_sum(st0 + j);
            }
        }
    }
    return s;
}
// every lane's f32 row (active: it wants one) by rounds of 32; all 64 lanes call it together
__device__ __forceinline__ float refine_rows_coop(const uint8_t *table, size_t row_bytes, uint32_t id, bool active,
                                                  const float *yq, uint32_t *ids_s, unsigned char *img, int lane) {
    const u64 W = __ballot(active);
    const uint32_t nw = (uint32_t)__popcll(W);
    if (nw == 0) return 0.0f;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(W >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)W, 0u));
    if (active) ids_s[rank] = id;
    const uint32_t ns = (uint32_t)(row_bytes / 128);
    float s = 0.0f;
#pragma unroll 1
    for (uint32_t r0 = 0; r0 < nw; r0 += 32) {  // (one copy of the round's code)
        const bool mine = active && rank >= r0 && rank < r0 + 32;
        const float sr = refine_coop_round(table, row_bytes, ns, mine, (rank - r0) & 31u, min(nw - r0, 32u), yq, ids_s + r0,
                                                img, lane);
        s = mine ? sr : s;
    }
    return s;
}
template <bool F16>
__device__ __forceinline__ void refine_evaluate(const DiverseLists &d, const float *yq, u64 *keys, uint32_t *ids_s,
                                                unsigned char *img, int lane) {
    const uint8_t *table = static_cast<const uint8_t *>(d.table);
    const size_t row_bytes = (size_t)d.full_dim * (F16 ? 2 : 4);
    const bool wide = (reinterpret_cast<uintptr_t>(table) & 15) == 0 && row_bytes % 16 == 0;  // the wave's
    // (f16 rows take a lane per row at every width: measured faster, DESIGN.md section 31)
    const bool coop = !F16 && wide && row_bytes % 128 == 0 && d.lane_rows == 0;
    for (uint32_t base = 0; base < d.pool; base += 64) {
        const uint32_t j = base + lane;  // (< cap)
        const u64 k = keys[j];
        const bool active = k != KEY_INVALID;
        const uint32_t id = (uint32_t)k;  // (< table_rows)
        float s = 0.0f;
        if (coop)
            s = refine_rows_coop(table, row_bytes, id, active, yq, ids_s, img, lane);
        else if (active)
            s = refine_lane_row<F16>(table + (size_t)id * row_bytes, d.full_dim, wide, yq);
        const float dist = __builtin_sqrtf(s);
        // a NaN distance is never returned
        keys[j] = active && dist == dist ? ((u64)__builtin_bit_cast(uint32_t, dist) << 32) | id : KEY_INVALID;
    }
    wave_fence();
}
__device__ __forceinline__ void refine_lists(const DiverseLists &d, unsigned char *smem, int lane) {
    const uint32_t q = blockIdx.x, pool = d.pool, n_out = d.n_out, dim = d.full_dim;
    if (q >= d.nq || pool == 0 || pool > HX_REFINE_POOL_MAX || n_out > pool || dim == 0 || dim > HX_REFINE_MAX_DIM)
        return;  // (the launcher's limits)
    const uint32_t cap = (pool + 63u) & ~63u;
    float *yq = reinterpret_cast<float *>(smem);
    u64 *keys = reinterpret_cast<u64 *>(smem + (((size_t)dim * 4 + 15) & ~(size_t)15));
    uint32_t *ids_s = reinterpret_cast<uint32_t *>(keys + cap);
    unsigned char *img = reinterpret_cast<unsigned char *>(ids_s + 64);  // (16-byte aligned: every part before it is)
    const size_t in0 = (size_t)q * pool, out0 = (size_t)q * n_out;
    const float *qf = d.queries + (size_t)q * dim;
    bool bad = false;
    for (uint32_t e = lane; e < dim; e += 64) {
        const float x = qf[e];
        bad |= (x != x);
        yq[e] = x;
    }
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (d.stats) st = d.stats[q];
    const uint32_t cnt = d.counts ? min(d.counts[q], pool) : pool;
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0 and padded rows
    bool beyond = false;
    for (uint32_t j = lane; j < cap; j += 64) {
        u64 k = KEY_INVALID;
        if (j < pool) {
            const uint32_t id = d.ids[in0 + j];
            const bool present = ok && (d.counts ? j < cnt : id != HX_EMPTY_SLOT);
            beyond |= present && (uint64_t)id >= d.table_rows;
            if (present) k = id;
        }
        keys[j] = k;
    }
    wave_fence();
    const bool nan = __ballot(bad) != 0, far = __ballot(beyond) != 0;  // the wave's
    uint32_t count = 0;
    if (ok && far) {
        st.status = HNSW_ERR_ARG;  // no row of the table is read for this query
    } else if (ok && nan) {
        st.status = HNSW_ERR_NAN_INPUT;
    } else if (ok) {
        if (d.table_dtype == HX_ROWS_F16)
            refine_evaluate<true>(d, yq, keys, ids_s, img, lane);
        else
            refine_evaluate<false>(d, yq, keys, ids_s, img, lane);
        const uint32_t even = (pool + 1u) & ~1u;  // (<= cap; the table is KEY_INVALID behind pool)
        uint32_t n_valid = 0;
        for (uint32_t base = 0; base < pool; base += 64) {
            const uint32_t j = base + lane;
            const u64 mine = keys[j];
            const bool valid = mine != KEY_INVALID;
            uint32_t r = 0;  // the keys before mine in (key, position) order
            for (uint32_t i = 0; i < even; i += 2) {
                const uint4 w = *reinterpret_cast<const uint4 *>(keys + i);
                const u64 k0 = ((u64)w.y << 32) | w.x, k1 = ((u64)w.w << 32) | w.z;
                r += (k0 < mine) | ((k0 == mine) & (i < j));
                r += (k1 < mine) | ((k1 == mine) & (i + 1 < j));
            }
            if (valid && r < n_out) {
                d.out_ids[out0 + r] = (uint32_t)mine;
                d.out_dists[out0 + r] = __builtin_bit_cast(float, (uint32_t)(mine >> 32));
            }
            n_valid += (uint32_t)__popcll(__ballot(valid));
        }
        count = min(n_valid, n_out);
    }
    for (uint32_t s = count + lane; s < n_out; s += 64) {
        d.out_ids[out0 + s] = HX_EMPTY_SLOT;
        d.out_dists[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        if (d.out_counts) d.out_counts[q] = count;
        if (d.out_stats) d.out_stats[q] = st;
    }
}
