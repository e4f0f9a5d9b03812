// form_diversify.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's second form: the MMR selection of diversified search.
// ---------------------------------------------------------------------------------------------
// The kernel's second form (DiverseLists with n_out != 0, list_forms.h; DESIGN.md section 26): query blockIdx.x's
// candidate list of d.pool entries re-ranked by maximal marginal relevance, one wave per query.  The entries live in
// LDS behind the staged row, entry j at index j of
//   sid[256]   its id, HX_EMPTY_SLOT once it is absent or selected   sbits[256]  its distance bits
//   smin[256]  the minimum so far of its distances to the selected rows (+inf before the first)
// so the two vector kinds differ in one place only, the pass that evaluates distances: QUANT8 takes a lane pair per
// entry and covers 32 entries a pass, F32 a lane per entry and 64.  A step stages the row selected last
// (stage_row: Point::dist2other's first argument), folds dist_any_dim of every entry still selectable into smin --
// a pass's row reads are all in flight together -- and takes the wave's minimum of (orderable score, position); the
// scoring holds entry 64 k + lane in lane `lane`.  Step 0 evaluates nothing.  Plain vector stores, no atomics.
// ---------------------------------------------------------------------------------------------
#define HX_DIVERSE_LDS (HX_DIVERSE_POOL_MAX * 12)
template <int KIND>
__device__ __forceinline__ void diversify(const DevView &v, const DiverseLists &d, float *yq, unsigned char *tab, int lane) {
    uint32_t *sid = reinterpret_cast<uint32_t *>(tab);
    uint32_t *sbits = sid + HX_DIVERSE_POOL_MAX;
    float *smin = reinterpret_cast<float *>(sbits + HX_DIVERSE_POOL_MAX);
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const uint32_t q = blockIdx.x, pool = d.pool, n_out = d.n_out;
    if (q >= d.nq || pool > HX_DIVERSE_POOL_MAX || n_out > pool) return;  // (the launcher's limits)
    const uint32_t *dist_bits = reinterpret_cast<const uint32_t *>(d.dists);
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (d.stats) st = d.stats[q];
    const uint32_t cnt = d.counts ? min(d.counts[q], pool) : pool;
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0 and padded rows
    const size_t in0 = (size_t)q * pool, out0 = (size_t)q * n_out;
    bool beyond = false;
    for (uint32_t j = lane; j < pool; j += 64) {
        const uint32_t id = d.ids[in0 + j];
        const bool present = ok && (d.counts ? j < cnt : id != HX_EMPTY_SLOT);
        beyond |= present && id >= v.n_points;
        sid[j] = present ? id : HX_EMPTY_SLOT;
        sbits[j] = dist_bits[in0 + j];
        smin[j] = __builtin_inff();
    }
    wave_fence();
    uint32_t count = 0;  // wave-uniform
    if (__ballot(beyond)) {
        st.status = HNSW_ERR_ARG;  // no row of the index is read for this query
    } else {
        const float lam = d.lambda, rest = 1.0f - lam;
        uint32_t last = 0;  // the id selected by the step before
        for (uint32_t t = 0; t < n_out; t++) {
            if (t > 0) {
                stage_row<KIND>(v, last, yq, lane);
                for (uint32_t base = 0; base < pool; base += CHUNK) {
                    const uint32_t j = base + lane / LPC;
                    const uint32_t id = j < pool ? sid[j] : HX_EMPTY_SLOT;
                    const bool active = id != HX_EMPTY_SLOT;
                    const float dist = dist_any_dim<KIND>(v, active ? id : 0u, active, h, yq);
                    if (active && h == 0 && dist < smin[j]) smin[j] = dist;  // (a NaN leaves the minimum as it is)
                }
                wave_fence();
            }
            u64 best = KEY_INVALID;
#pragma unroll
            for (int k = 0; k < HX_DIVERSE_POOL_MAX / 64; k++) {
                const uint32_t j = 64u * k + lane;
                if (j >= pool || sid[j] == HX_EMPTY_SLOT) continue;
                const float near = lam * __builtin_bit_cast(float, sbits[j]);
                const float far = rest * (t == 0 ? 0.0f : smin[j]);
                float score = near - far;
                if (score != score) continue;       // a NaN score is never selected
                if (score == 0.0f) score = 0.0f;    // -0 == +0: one key for both
                const uint32_t u = __builtin_bit_cast(uint32_t, score);
                const u64 key = ((u64)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | j;
                best = key < best ? key : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 other = ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o) << 32) |
                                  (uint32_t)__shfl_xor((int)(uint32_t)best, o);
                best = other < best ? other : best;
            }
            if (best == KEY_INVALID) break;  // nothing selectable: the selection ends
            const uint32_t js = (uint32_t)best & (HX_DIVERSE_POOL_MAX - 1);
            last = (uint32_t)__builtin_amdgcn_readfirstlane((int)sid[js]);  // one address for the wave: a broadcast
            const uint32_t bits = sbits[js];
            const float gap = smin[js];  // (+inf at step 0, by definition)
            wave_fence();
            if (lane == 0) {
                sid[js] = HX_EMPTY_SLOT;
                d.out_ids[out0 + t] = last;
                d.out_dists[out0 + t] = __builtin_bit_cast(float, bits);
                if (d.out_gaps) d.out_gaps[out0 + t] = gap;
            }
            wave_fence();
            count = t + 1;
        }
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
