// form_fuse_lists.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's fourth form: the fusion of a query's per-vector candidate lists.
// ---------------------------------------------------------------------------------------------
// The kernel's fourth form (DiverseLists with n_vecs != 0, list_forms.h; DESIGN.md section 28): query blockIdx.x's
// n_vecs candidate lists of d.pool ids each fused into the n_out best by summed (or smallest) weighted distance to the
// query's n_vecs vectors, one wave per query.  Behind the staged vector the LDS table holds
//   sid[256]   the n_vecs * pool entries as loaded, absent ones (and everything behind them) as HX_EMPTY_SLOT
//   sacc[256]  the running fold of compacted entry j        cid[256]  the distinct present ids, compacted
// Lane `lane` holds entries 64 k + lane in registers.  Presence, range and the incoming statuses are decided (a ballot)
// before any row is read.  The duplicates go by an all-pairs compare: every lane reads the table once, four words a read and
// the same address in every lane (a broadcast, no bank conflict), and an entry with an equal id before it is dropped;
// the survivors are compacted by ballot prefix, so that the passes below cover `unique` entries, not n_vecs * pool.
// Per vector: stage_query as any query is staged, then diversify's pass loop (QUANT8 a lane pair per entry and 32
// entries a pass, F32 a lane per entry and 64; a pass's row reads all in flight together) with w * dist folded into
// sacc[j].  The emission takes n_out times the wave's minimum of (orderable score, id) over keys held in registers;
// ids are distinct by now, so exactly one lane owns the minimum and stores it.  Plain vector stores, no atomics.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ void fuse_lists(const DevView &v, const DiverseLists &d, float *yq, unsigned char *tab, int lane) {
    uint32_t *sid = reinterpret_cast<uint32_t *>(tab);
    float *sacc = reinterpret_cast<float *>(sid + HX_DIVERSE_POOL_MAX);
    uint32_t *cid = sid + 2 * HX_DIVERSE_POOL_MAX;
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    constexpr int PER = HX_DIVERSE_POOL_MAX / 64;  // entries a lane holds
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const uint32_t q = blockIdx.x, T = d.n_vecs, pool = d.pool, n_out = d.n_out;
    if (q >= d.nq || T > HX_MULTI_MAX_VECS || pool > HX_DIVERSE_POOL_MAX || T * pool > HX_DIVERSE_POOL_MAX || n_out > pool)
        return;  // (the launcher's limits)
    const uint32_t total = T * pool;
    const size_t l0 = (size_t)q * T, in0 = (size_t)q * total, out0 = (size_t)q * n_out;
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (d.stats)
        for (uint32_t t = 0; t < T; t++) {  // (wave-uniform: the wrapping sums, the first status that is not OK)
            const hnsw_query_stats s = d.stats[l0 + t];
            st.n_dist += s.n_dist, st.n_exp += s.n_exp, st.sum_deg += s.sum_deg;
            if (st.status == HNSW_OK) st.status = s.status;
        }
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0 and padded rows
    uint32_t mine[PER];
    bool beyond = false;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const uint32_t j = 64u * k + lane;
        uint32_t id = HX_EMPTY_SLOT;
        if (j < total) {
            const uint32_t t = j / pool, jj = j - t * pool;
            const uint32_t raw = d.ids[in0 + j];
            const bool present = ok && (d.counts ? jj < min(d.counts[l0 + t], pool) : raw != HX_EMPTY_SLOT);
            beyond |= present && raw >= v.n_points;
            id = present ? raw : HX_EMPTY_SLOT;
        }
        mine[k] = id;
        sid[j] = id;  // (j < 256: the whole table is written)
    }
    wave_fence();
    uint32_t count = 0, unique = 0;  // wave-uniform
    if (__ballot(beyond)) {
        st.status = HNSW_ERR_ARG;  // no row of the index is read for this query
    } else if (ok) {
        bool dup[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) dup[k] = false;
        for (uint32_t i = 0; i < total; i += 4) {  // (total <= 256, and the table is EMPTY behind `total`)
            const uint4 w = *reinterpret_cast<const uint4 *>(sid + i);
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const uint32_t j = 64u * k + lane, id = mine[k];
                dup[k] |= (w.x == id && i < j) | (w.y == id && i + 1 < j) | (w.z == id && i + 2 < j) | (w.w == id && i + 3 < j);
            }
        }
#pragma unroll
        for (int k = 0; k < PER; k++) {  // the distinct present ids, in table order, to cid[0 .. unique)
            const bool live = mine[k] != HX_EMPTY_SLOT && !dup[k];
            const u64 b = __ballot(live);
            if (live) cid[unique + __builtin_popcountll(b & ((1ull << lane) - 1))] = mine[k];
            unique += (uint32_t)__builtin_popcountll(b);
        }
        wave_fence();
        bool nan = false;  // wave-uniform
        for (uint32_t t = 0; t < T; t++) {
            if (!stage_query<KIND>(v, d.queries + (l0 + t) * v.dim, yq, lane)) {
                nan = true;
                break;
            }
            const float w = d.weights ? d.weights[l0 + t] : 1.0f;
            for (uint32_t base = 0; base < unique; base += CHUNK) {
                const uint32_t j = base + lane / LPC;
                const bool active = j < unique;
                const uint32_t id = active ? cid[j] : 0u;
                const float dist = dist_any_dim<KIND>(v, id, active, h, yq);
                if (active && h == 0) {
                    const float p = d.weights ? w * dist : dist;
                    float s;
                    if (d.mode == HNSW_FUSE_MIN) {
                        const float cur = t == 0 ? __builtin_inff() : sacc[j];
                        s = p < cur ? p : cur;  // (a NaN term leaves the minimum as it is)
                    } else {
                        s = t == 0 ? p : sacc[j] + p;
                    }
                    sacc[j] = s;
                }
            }
            wave_fence();
        }
        if (nan) {
            st.status = HNSW_ERR_NAN_INPUT;
            unique = 0;
        } else {
            u64 key[PER];
            float sc[PER];
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const uint32_t j = 64u * k + lane;
                key[k] = KEY_INVALID;
                sc[k] = 0.0f;
                if (j < unique) {
                    const float score = sacc[j];
                    sc[k] = score;
                    if (score == score) {  // a NaN score is never returned
                        const uint32_t u = __builtin_bit_cast(uint32_t, score == 0.0f ? 0.0f : score);  // -0 == +0: one key
                        key[k] = ((u64)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | cid[j];
                    }
                }
            }
            for (uint32_t t = 0; t < n_out; t++) {
                u64 best = KEY_INVALID;
#pragma unroll
                for (int k = 0; k < PER; k++) best = key[k] < best ? key[k] : best;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const u64 other = ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o) << 32) |
                                      (uint32_t)__shfl_xor((int)(uint32_t)best, o);
                    best = other < best ? other : best;
                }
                if (best == KEY_INVALID) break;  // nothing left
#pragma unroll
                for (int k = 0; k < PER; k++)
                    if (key[k] == best) {  // (ids are distinct: one entry of one lane)
                        key[k] = KEY_INVALID;
                        d.out_ids[out0 + t] = (uint32_t)best;
                        d.out_dists[out0 + t] = sc[k];
                    }
                count = t + 1;
            }
        }
    }
    for (uint32_t s = count + lane; s < n_out; s += 64) {
        d.out_ids[out0 + s] = HX_EMPTY_SLOT;
        d.out_dists[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        if (d.out_counts) d.out_counts[q] = count;
        if (d.unique_out) d.unique_out[q] = unique;
        if (d.out_stats) d.out_stats[q] = st;
    }
}
