// form_boost.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's ninth form: the boost of a candidate list by per-id attributes.
// ---------------------------------------------------------------------------------------------
// The kernel's ninth form (DiverseLists with boost != 0, list_forms.h; DESIGN.md section 34): query blockIdx.x's
// candidate list of d.pool (id, distance) pairs re-ranked by s = w[0] * distance + sum_k w[1 + k] * attribute k of the id,
// the attributes a row of d.full_dim <= 32 elements of a table in HBM -- f32, or IEEE binary16 widened exactly -- and cut
// to the n_out smallest, one wave per query.  It reads nothing of the DevView.  LDS, with cap = pool rounded up to 64:
//   keys  cap double words: first the present ids (KEY_INVALID: absent), then (score key << 32 | id), KEY_INVALID for NaN
//   wq    the query's weight row, 1 + full_dim floats
// Presence, the incoming status and the range are decided (a ballot) before any table row is read.  A lane owns entries
// lane, lane + 64, ...: it reads its row -- at most 128 bytes, one line -- by 16-byte loads where the table and its row
// stride allow them, element loads otherwise, and runs the chain s = w0 * d, then p = w * a; s = s + p attribute by
// attribute, every operation rounded on its own.  -0 becomes +0.  The score key is the order-preserving map of the f32
// bits (all bits of a negative flipped, the sign bit of a non-negative set), so that a 64-bit unsigned compare of
// (key, id) is the ranking; the rank of an entry is counted as the sixth form counts it, so duplicate ids are separate
// entries ordered by position.  A winner reads its own incoming distance again (the same word it scored) for out_gaps.
// Plain vector stores, no atomics; every output word is written once.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline size_t boost_lds_bytes(uint32_t n_attrs, uint32_t pool) {
    return (((size_t)pool + 63) & ~(size_t)63) * 8 + (((size_t)(1 + n_attrs) * 4 + 15) & ~(size_t)15);
}
// the chain over a row of `na` attributes, continuing s; `wide` (the wave's): whole 16-byte pieces on a 16-byte grid
template <bool F16>
__device__ __forceinline__ float boost_row(const uint8_t *row, uint32_t na, bool wide, const float *w, float s) {
    constexpr uint32_t EPP = F16 ? 8 : 4;  // elements per 16-byte piece
    if (wide) {
        const uint4 *src = reinterpret_cast<const uint4 *>(row);
        const uint32_t np = na / EPP;
#pragma unroll 1
        for (uint32_t p = 0; p < np; p++) {
            const uint4 pp = src[p];
            const uint32_t x[4] = {pp.x, pp.y, pp.z, pp.w};
            const float *wp = w + (size_t)p * EPP;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if constexpr (F16) {
                    const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(x[i] & 0xFFFFu));  // (exact)
                    const float hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(x[i] >> 16));
                    s = __fadd_rn(s, __fmul_rn(wp[2 * i], lo));
                    s = __fadd_rn(s, __fmul_rn(wp[2 * i + 1], hi));
                } else {
                    s = __fadd_rn(s, __fmul_rn(wp[i], __builtin_bit_cast(float, x[i])));
                }
            }
        }
    } else {
#pragma unroll 1
        for (uint32_t e = 0; e < na; e++) {
            float a;
            if constexpr (F16)
                a = (float)__builtin_bit_cast(_Float16, reinterpret_cast<const uint16_t *>(row)[e]);  // (exact)
            else
                a = reinterpret_cast<const float *>(row)[e];
            s = __fadd_rn(s, __fmul_rn(w[e], a));
        }
    }
    return s;
}
__device__ __forceinline__ void boost_lists(const DiverseLists &d, unsigned char *smem, int lane) {
    const uint32_t q = blockIdx.x, pool = d.pool, n_out = d.n_out, na = d.full_dim;
    if (q >= d.nq || pool == 0 || pool > HX_BOOST_POOL_MAX || n_out > pool || na == 0 || na > HX_BOOST_MAX_ATTRS)
        return;  // (the launcher's limits)
    const uint32_t cap = (pool + 63u) & ~63u;
    u64 *keys = reinterpret_cast<u64 *>(smem);
    float *wq = reinterpret_cast<float *>(keys + cap);
    const size_t in0 = (size_t)q * pool, out0 = (size_t)q * n_out;
    const float *w = d.weights + (d.boost == 2 ? (size_t)q * (1 + na) : (size_t)0);
    if ((uint32_t)lane <= na) wq[lane] = w[lane];  // (1 + na <= 33 lanes)
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
    const bool far = __ballot(beyond) != 0;  // the wave's
    uint32_t count = 0;
    if (ok && far) {
        st.status = HNSW_ERR_ARG;  // no row of the table is read for this query
    } else if (ok) {
        const bool f16 = d.table_dtype == HX_ROWS_F16;
        const uint8_t *table = static_cast<const uint8_t *>(d.table);
        const size_t row_bytes = (size_t)na * (f16 ? 2 : 4);
        const bool wide = (reinterpret_cast<uintptr_t>(table) & 15) == 0 && row_bytes % 16 == 0;  // the wave's
        const float w0 = wq[0];
        for (uint32_t base = 0; base < pool; base += 64) {
            const uint32_t j = base + lane;  // (< cap)
            const u64 k = keys[j];
            u64 key = KEY_INVALID;
            if (k != KEY_INVALID) {
                const uint32_t id = (uint32_t)k;  // (< table_rows)
                const uint8_t *row = table + (size_t)id * row_bytes;
                float s = __fmul_rn(w0, d.dists[in0 + j]);
                s = f16 ? boost_row<true>(row, na, wide, wq + 1, s) : boost_row<false>(row, na, wide, wq + 1, s);
                uint32_t b = __builtin_bit_cast(uint32_t, s);
                if (b == 0x80000000u) b = 0u;  // -0 is +0
                // a NaN score is never returned
                if (s == s) key = ((u64)((b & 0x80000000u) ? ~b : (b | 0x80000000u)) << 32) | id;
            }
            keys[j] = key;
        }
        wave_fence();
        const uint32_t even = (pool + 1u) & ~1u;  // (<= cap; the table is KEY_INVALID behind pool)
        uint32_t n_valid = 0;
        for (uint32_t base = 0; base < pool; base += 64) {
            const uint32_t j = base + lane;
            const u64 mine = keys[j];
            const bool valid = mine != KEY_INVALID;
            uint32_t r = 0;  // the keys before mine in (key, position) order
            for (uint32_t i = 0; i < even; i += 2) {
                const uint4 kk = *reinterpret_cast<const uint4 *>(keys + i);
                const u64 k0 = ((u64)kk.y << 32) | kk.x, k1 = ((u64)kk.w << 32) | kk.z;
                r += (k0 < mine) | ((k0 == mine) & (i < j));
                r += (k1 < mine) | ((k1 == mine) & (i + 1 < j));
            }
            if (valid && r < n_out) {
                const uint32_t kb = (uint32_t)(mine >> 32);
                d.out_ids[out0 + r] = (uint32_t)mine;
                d.out_dists[out0 + r] = __builtin_bit_cast(float, (kb & 0x80000000u) ? (kb ^ 0x80000000u) : ~kb);
                if (d.out_gaps) d.out_gaps[out0 + r] = d.dists[in0 + j];
            }
            n_valid += (uint32_t)__popcll(__ballot(valid));
        }
        count = min(n_valid, n_out);
    }
    for (uint32_t s = count + lane; s < n_out; s += 64) {
        d.out_ids[out0 + s] = HX_EMPTY_SLOT;
        d.out_dists[out0 + s] = __builtin_inff();
        if (d.out_gaps) d.out_gaps[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        if (d.out_counts) d.out_counts[q] = count;
        if (d.out_stats) d.out_stats[q] = st;
    }
}
