// form_fuse_ranked.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's eighth form: the rank fusion of a dense list with external ranked lists.
// ---------------------------------------------------------------------------------------------
// The kernel's eighth form (DiverseLists with hybrid != 0, list_forms.h; DESIGN.md section 33): query blockIdx.x's
// ranked lists -- the optional dense one, then n_ext external ones -- fused by reciprocal rank or by a weighted sum of
// scores into the n_out best under the handle's filters, one wave per query.  A SLOT is a list-major position, so slot
// order is list order.  Behind the staged row the LDS table holds, 256 entries each,
//   sid   a slot's id: as loaded and admissible, then (pass A) only where the slot is KEPT; HX_EMPTY_SLOT otherwise
//   sx    its external score, as bits          srk   a kept slot's 1-based rank in its list
//   cid   the distinct kept ids (the LEADERS: first kept slot of an id in any list), compacted in slot order
//   sD    D of an evaluated entry              wid   the winners' ids by output position
//   skey  (double words) the candidates' keys: an order-preserving map of the score bits, then the id
// Lane `lane` holds slots, and later candidates, 64 k + lane in registers.  The incoming status, the query's mask row,
// presence, the range of the ids and the query's NaN check are decided before anything else is read; then the deny word,
// the mask word and the label of every present slot are read, all of them issued before the first is looked at.  Passes A
// and B are all-pairs compares over the table, four words a read and the same address in every lane (a broadcast):
// A drops a slot that an earlier admissible slot of its own list repeats, B counts the kept slots before a slot in its
// list (its rank) and finds whether an earlier kept slot of any list has its id (then it is no leader).  Pass C: every
// candidate walks the kept slots in slot order -- one address for the wave -- and folds the term of each that carries its
// id, so the fold's order is the contract's.  D is dist_any_dim after stage_query (QUANT8 a lane pair per entry and 32
// entries a pass, F32 a lane per entry and 64), under LINEAR of every candidate before the fold, under RRF of the winners
// alone and only when the distances are asked for: the two-turn loop keeps it at one call site.  A candidate's output
// position is the number of keys below its own, counted over skey two keys a read.  Plain vector stores, no atomics.
// ---------------------------------------------------------------------------------------------
#define HX_HYBRID_LDS (HX_DIVERSE_POOL_MAX * 32)
template <int KIND>
__device__ __forceinline__ void fuse_ranked(const DevView &v, const DiverseLists &d, float *yq, unsigned char *tab, int lane) {
    uint32_t *sid = reinterpret_cast<uint32_t *>(tab);
    uint32_t *sx = sid + HX_DIVERSE_POOL_MAX, *srk = sx + HX_DIVERSE_POOL_MAX, *cid = srk + HX_DIVERSE_POOL_MAX;
    float *sD = reinterpret_cast<float *>(cid + HX_DIVERSE_POOL_MAX);
    uint32_t *wid = cid + 2 * HX_DIVERSE_POOL_MAX;
    u64 *skey = reinterpret_cast<u64 *>(wid + HX_DIVERSE_POOL_MAX);  // (6 KiB in: 16-byte aligned, as the table is)
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    constexpr int PER = HX_DIVERSE_POOL_MAX / 64;  // slots, and candidates, a lane holds
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const bool linear = d.hybrid == 2;
    const uint32_t q = blockIdx.x, E = d.n_ext, W = d.ext_width, n_out = d.n_out;
    const uint32_t p0 = d.ids ? d.pool : 0u;  // the dense list's slots
    if (q >= d.nq || E > HX_HYBRID_MAX_EXT || p0 > HX_DIVERSE_POOL_MAX || (E != 0 && W > HX_DIVERSE_POOL_MAX)) return;
    const uint32_t total = p0 + E * W;
    if (total == 0 || total > HX_DIVERSE_POOL_MAX || n_out > total) return;  // (the launcher's limits, here and above)
    const size_t out0 = (size_t)q * n_out, w0 = (size_t)q * (1 + E);
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (d.stats) st = d.stats[q];
    int32_t status = st.status;  // wave-uniform: the causes of a failed query, in the contract's order
    const uint64_t *row = nullptr;  // the query's mask row (nullptr: no bit test)
    bool rowed = false;
    if (status == HNSW_OK && d.rowed) {
        const uint32_t m = d.mask_of ? d.mask_of[q] : 0u;
        if (m != HNSW_MASK_NONE) {
            if (m >= d.n_masks) {
                status = HNSW_ERR_ARG;  // no mask word is read
            } else {
                rowed = true;
                row = d.allow + (size_t)m * d.mask_words;
            }
        }
    }
    bool nan = false;  // (reads the query alone)
    if (status == HNSW_OK && d.queries) nan = !stage_query<KIND>(v, d.queries + (size_t)q * v.dim, yq, lane);
    uint32_t mine[PER], ls[PER], xs[PER];  // a slot's id, the first slot of its list, its score bits
    bool beyond = false;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const uint32_t j = 64u * k + lane;
        uint32_t id = HX_EMPTY_SLOT, xb = 0u, start = 0u;
        if (j < total && status == HNSW_OK) {
            uint32_t raw;
            bool present;
            if (j < p0) {
                raw = d.ids[(size_t)q * p0 + j];
                present = d.counts ? j < min(d.counts[q], p0) : raw != HX_EMPTY_SLOT;
            } else {
                const uint32_t e = (j - p0) / W, jj = j - p0 - e * W;
                const size_t at = ((size_t)q * E + e) * W + jj;
                start = p0 + e * W;
                raw = d.ext_ids[at];
                present = d.ext_counts ? jj < min(d.ext_counts[(size_t)q * E + e], W) : raw != HX_EMPTY_SLOT;
                if (d.ext_scores) xb = __builtin_bit_cast(uint32_t, d.ext_scores[at]);
            }
            beyond |= present && raw >= v.n_points;
            id = present ? raw : HX_EMPTY_SLOT;
        }
        mine[k] = id, ls[k] = start, xs[k] = xb;
    }
    if (status == HNSW_OK && __ballot(beyond) != 0) status = HNSW_ERR_ARG;  // no row, mask word or label is read
    if (status == HNSW_OK && nan) status = HNSW_ERR_NAN_INPUT;
    uint32_t count = 0, unique = 0, dropped = 0;  // wave-uniform
    if (status == HNSW_OK) {
        // ---- the filter: every gather issued before the first is looked at ----
        const bool ranged = d.range_lo != nullptr;
        const uint32_t lo = ranged ? d.range_lo[q] : 0u, hi = ranged ? d.range_hi[q] : 0u;
        const bool label_test = ranged && lo <= hi;  // (lo > hi admits nothing and reads no label)
        u64 wd[PER], wa[PER];
        uint32_t lab[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t id = mine[k];
            const bool p = id != HX_EMPTY_SLOT;
            wd[k] = (p && d.deny && id < d.deny_bits) ? d.deny[id >> 6] : 0ull;
            wa[k] = (p && rowed && id < d.allow_bits) ? row[id >> 6] : 0ull;
            lab[k] = (p && label_test && id < d.label_len) ? d.labels[id] : 0u;
        }
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t j = 64u * k + lane, id = mine[k];
            const bool p = id != HX_EMPTY_SLOT;
            bool adm = p && ((wd[k] >> (id & 63u)) & 1ull) == 0;
            if (rowed) adm = adm && ((wa[k] >> (id & 63u)) & 1ull) != 0;  // (a word of 0 beyond allow_bits)
            if (ranged) adm = adm && label_test && lab[k] >= lo && lab[k] <= hi;
            dropped += (uint32_t)__popcll(__ballot(p && !adm));
            if (!adm) mine[k] = HX_EMPTY_SLOT;
            sid[j] = mine[k];  // (j < 256: the whole table is written)
            sx[j] = xs[k];
        }
        wave_fence();
        // ---- pass A: a slot an earlier admissible slot of its own list repeats is not kept ----
        bool rep[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) rep[k] = false;
        for (uint32_t i = 0; i < total; i += 4) {  // (total <= 256, and the table is EMPTY behind `total`)
            const uint4 w = *reinterpret_cast<const uint4 *>(sid + i);
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const uint32_t j = 64u * k + lane, id = mine[k], s0 = ls[k];
                rep[k] |= (w.x == id && i >= s0 && i < j) | (w.y == id && i + 1 >= s0 && i + 1 < j) |
                          (w.z == id && i + 2 >= s0 && i + 2 < j) | (w.w == id && i + 3 >= s0 && i + 3 < j);
            }
        }
        wave_fence();
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (rep[k]) {
                mine[k] = HX_EMPTY_SLOT;
                sid[64u * k + lane] = HX_EMPTY_SLOT;
            }
        wave_fence();
        // ---- pass B: a kept slot's rank in its list, and whether an earlier kept slot of any list has its id ----
        uint32_t before[PER];
        bool later[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) before[k] = 0u, later[k] = false;
        for (uint32_t i = 0; i < total; i += 4) {
            const uint4 w = *reinterpret_cast<const uint4 *>(sid + i);
#pragma unroll
            for (int k = 0; k < PER; k++) {
                const uint32_t j = 64u * k + lane, id = mine[k], s0 = ls[k];
                before[k] += (uint32_t)(w.x != HX_EMPTY_SLOT && i >= s0 && i < j) +
                             (uint32_t)(w.y != HX_EMPTY_SLOT && i + 1 >= s0 && i + 1 < j) +
                             (uint32_t)(w.z != HX_EMPTY_SLOT && i + 2 >= s0 && i + 2 < j) +
                             (uint32_t)(w.w != HX_EMPTY_SLOT && i + 3 >= s0 && i + 3 < j);
                later[k] |= (w.x == id && i < j) | (w.y == id && i + 1 < j) | (w.z == id && i + 2 < j) | (w.w == id && i + 3 < j);
            }
        }
#pragma unroll
        for (int k = 0; k < PER; k++) {  // the leaders, in slot order, to cid[0 .. unique)
            srk[64u * k + lane] = before[k] + 1u;
            const bool lead = mine[k] != HX_EMPTY_SLOT && !later[k];
            const u64 b = __ballot(lead);
            if (lead) cid[unique + __builtin_popcountll(b & ((1ull << lane) - 1))] = mine[k];
            unique += (uint32_t)__builtin_popcountll(b);
        }
        wave_fence();
        uint32_t cm[PER];  // candidate 64 k + lane's id
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const uint32_t j = 64u * k + lane;
            cm[k] = j < unique ? cid[j] : HX_EMPTY_SLOT;
        }
        const bool eval_first = linear && d.queries != nullptr;  // D enters the score: every candidate, before the fold
#pragma unroll 1
        for (int turn = 0; turn < 2; turn++) {
            if ((turn == 0) != eval_first) {
                // ---- pass C: the fold, in list order ----
                float s[PER];
                bool have[PER];
#pragma unroll
                for (int k = 0; k < PER; k++) s[k] = 0.0f, have[k] = false;
                if (eval_first) {
                    const float wdense = d.weights ? d.weights[w0] : 1.0f;
#pragma unroll
                    for (int k = 0; k < PER; k++) {
                        const float x = sD[64u * k + lane];
                        s[k] = d.weights ? wdense * x : x;
                        have[k] = true;
                    }
                }
                for (uint32_t l = d.ids ? 0u : 1u; l <= E; l++) {  // list l: the dense one, or external list l - 1
                    const uint32_t start = l == 0 ? 0u : p0 + (l - 1) * W, width = l == 0 ? p0 : W;
                    const float wl = d.weights ? d.weights[w0 + l] : 1.0f;
                    if (!linear) {
                        for (uint32_t i = start; i < start + width; i++) {
                            const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)sid[i]);  // one address: a broadcast
                            if (id == HX_EMPTY_SLOT) continue;
                            const float t = wl / (float)(d.rank_constant + srk[i]);  // ONE correctly rounded division
#pragma unroll
                            for (int k = 0; k < PER; k++)
                                if (cm[k] == id) {
                                    s[k] = have[k] ? s[k] + t : t;
                                    have[k] = true;
                                }
                        }
                    } else if (l != 0) {
                        float ab = 0.0f;
#pragma unroll
                        for (uint32_t e = 0; e < HX_HYBRID_MAX_EXT; e++)
                            if (e == l - 1) ab = d.absent[e];  // (by compile-time index: the record stays in the argument block)
                        float x[PER];
#pragma unroll
                        for (int k = 0; k < PER; k++) x[k] = ab;
                        for (uint32_t i = start; i < start + width; i++) {
                            const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)sid[i]);
                            if (id == HX_EMPTY_SLOT) continue;
                            const float xv = __builtin_bit_cast(float, sx[i]);
#pragma unroll
                            for (int k = 0; k < PER; k++)
                                if (cm[k] == id) x[k] = xv;
                        }
#pragma unroll
                        for (int k = 0; k < PER; k++) {
                            const float p = d.weights ? wl * x[k] : x[k];
                            s[k] = have[k] ? s[k] + p : p;
                            have[k] = true;
                        }
                    }
                }
                // ---- the selection: a candidate's position is the number of keys below its own ----
                u64 key[PER];
                uint32_t n_valid = 0;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const uint32_t j = 64u * k + lane;
                    key[k] = KEY_INVALID;
                    const float score = s[k];
                    if (j < unique && have[k] && score == score) {  // a NaN score is never returned
                        const uint32_t u = __builtin_bit_cast(uint32_t, score == 0.0f ? 0.0f : score);  // -0 == +0: one key
                        const uint32_t up = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending with the score
                        key[k] = ((u64)(linear ? up : ~up) << 32) | cm[k];                  // RRF: larger is better
                    }
                    skey[j] = key[k];  // (j < 256: the whole table is written)
                    n_valid += (uint32_t)__popcll(__ballot(key[k] != KEY_INVALID));
                }
                wave_fence();
                uint32_t r[PER];
#pragma unroll
                for (int k = 0; k < PER; k++) r[k] = 0u;
                const uint32_t even = (unique + 1u) & ~1u;
                for (uint32_t i = 0; i < even; i += 2) {
                    const uint4 w = *reinterpret_cast<const uint4 *>(skey + i);
                    const u64 k0 = ((u64)w.y << 32) | w.x, k1 = ((u64)w.w << 32) | w.z;
#pragma unroll
                    for (int k = 0; k < PER; k++) r[k] += (uint32_t)(k0 < key[k]) + (uint32_t)(k1 < key[k]);
                }
#pragma unroll
                for (int k = 0; k < PER; k++)
                    if (key[k] != KEY_INVALID && r[k] < n_out) {  // (ids are distinct: so are the keys and the positions)
                        d.out_ids[out0 + r[k]] = cm[k];
                        d.out_dists[out0 + r[k]] = s[k];
                        wid[r[k]] = cm[k];
                        if (eval_first && d.out_gaps) d.out_gaps[out0 + r[k]] = sD[64u * k + lane];
                    }
                count = min(n_valid, n_out);
                wave_fence();
            }
            const bool winners = !eval_first && d.out_gaps != nullptr;  // RRF: D of the winners alone, when asked for
            if (turn == 0 && (eval_first || winners)) {
                const uint32_t *el = eval_first ? cid : wid;
                const uint32_t n_e = eval_first ? unique : count;
                for (uint32_t base = 0; base < n_e; base += CHUNK) {
                    const uint32_t j = base + lane / LPC;
                    const bool active = j < n_e;
                    const uint32_t id = active ? el[j] : 0u;
                    const float dist = dist_any_dim<KIND>(v, id, active, h, yq);
                    if (active && h == 0) sD[j] = dist;
                }
                wave_fence();
                if (winners)
                    for (uint32_t t = lane; t < count; t += 64) d.out_gaps[out0 + t] = sD[t];
            }
        }
    }
    if (status != HNSW_OK) unique = dropped = 0;
    const float worst = linear ? __builtin_inff() : -__builtin_inff();
    for (uint32_t s = count + lane; s < n_out; s += 64) {
        d.out_ids[out0 + s] = HX_EMPTY_SLOT;
        d.out_dists[out0 + s] = worst;
        if (d.out_gaps) d.out_gaps[out0 + s] = __builtin_inff();
    }
    if (lane == 0) {
        st.status = status;
        if (d.out_counts) d.out_counts[q] = count;
        if (d.unique_out) d.unique_out[q] = unique;
        if (d.dropped_out) d.dropped_out[q] = dropped;
        if (d.out_stats) d.out_stats[q] = st;
    }
}
