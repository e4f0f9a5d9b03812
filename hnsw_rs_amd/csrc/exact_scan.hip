// exact_scan.hip -- the exact scans under the index's own metric, gfx950: hx_brute_kernel (the reference's ground truth,
// every query against all points) and hx_distance_kernel (dist2many for one query, a test seam; in its second form the
// MMR selection of diversified search: stored rows against a stored row; in its third the query rows composed out of
// stored rows; in its fourth the fusion of a query's per-vector candidate lists; in its fifth the late interaction that
// scores those candidates as documents; in its sixth the refinement of a candidate list against a table of full rows; in
// its seventh the scoring of named documents over every stored row they have; in its eighth the rank fusion of a query's
// dense list with external ranked lists under the handle's filters; in its ninth the boost of a candidate list by per-id
// attributes out of a row table), with their launchers.
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
// ---------------------------------------------------------------------------------------------
// The kernel's second form (DiverseLists with n_out != 0, device_index.h): query blockIdx.x's
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

// ---------------------------------------------------------------------------------------------
// The kernel's third form (DiverseLists with width != 0, device_index.h): query blockIdx.x's row
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

// ---------------------------------------------------------------------------------------------
// The kernel's fourth form (DiverseLists with n_vecs != 0, device_index.h): query blockIdx.x's
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

// ---------------------------------------------------------------------------------------------
// The kernel's fifth form (DiverseLists with late != 0, device_index.h): query blockIdx.x's
// n_vecs candidate lists of d.pool ids each scored as DOCUMENTS -- the candidates that share a label -- by the sum over
// the query's vectors of the distance to the document's nearest candidate, one wave per query.  Behind the staged vector
// the LDS table holds, with cap = n_vecs * pool rounded up to 64, seven arrays of cap words and one of cap double words:
//   sid    the entries as loaded, absent ones as HX_EMPTY_SLOT; once the ids are compacted, compacted candidate j's label
//   cid    the distinct present ids, compacted            cdoc   candidate j's document, an index into the arrays below
//   dlab   the distinct labels, compacted                 dmin   document g's minimum under the vector in hand, as bits
//   dsum   its running fold                               dsize  its candidates
//   dbest  the smallest (distance bits << 32 | id) any of its candidates had under any vector
// Nothing of it lives in registers: every step is a loop over the table, 64 entries a turn.  Presence, range and the
// incoming statuses are decided (a ballot) before any row is read.  Duplicates go by fuse_lists' all-pairs compare -- four
// words a read, the same address in every lane -- over the entries before an entry's own turn; the labels are numbered
// the same way, the compare keeping the first equal entry's index so that a later candidate finds its document.  Per
// vector: stage_query, then fuse_lists' pass loop (QUANT8 a lane pair per entry and 32 entries a pass, F32 a lane per
// entry and 64; a pass's row reads all in flight together), each distance folded into its document by LDS atomic
// minima on the bits -- distances are >= +0 or NaN and a NaN is skipped, so the bits order as the floats do and the
// result does not depend on the order of arrival -- and after the pass e_t into dsum.  The emission takes n_out times
// the wave's minimum of (orderable score, label); labels are distinct, so one lane owns it.  Plain vector stores.
//
// The kernel's seventh form (DiverseLists with docs != 0) is the same function: query blockIdx.x's
// ONE list of d.pool LABELS scored as documents over EVERY undeleted row they have -- a label's rows are a slice of the
// document index d.doc_keys (label << 32 | id, ascending).  It shares everything from the per-vector pass loop on -- one
// call site of dist_any_dim -- and differs before it.  Its LDS table is HX_DOCS_LDS(n_in, n_vecs):
//   dbest  256 double words   dlab, dstart, dsize, dpre, dsum  256 words each: a document's label, the index of its first
//   key, its FULL size, the scored rows before it (the prefix sums of min(size, rows_cap)), its fold
//   cid, cdoc  HX_DOCS_CHUNK words each: a chunk's row ids and their documents (cid first holds the labels as loaded)
//   dmin   n_in * n_vecs words: the minima of document g under vector t at g * n_vecs + t, kept ACROSS chunks
// The incoming status, presence (a prefix of the list: there is no pad) and the NaN check of all n_vecs vectors are decided
// before any index row is read.  The distinct labels go by the same all-pairs compare; one lane per distinct label runs
// the two binary searches over the keys in HBM; labels without a row drop out in the ballot compaction.  The scored rows
// of all documents, in document order, are walked in chunks of HX_DOCS_CHUNK entries: every lane finds its entry's
// document by a binary search over dpre and reads the id from the key's low word; then, per vector, stage_query and the
// pass loop.  A document may straddle chunks or be larger than one: its minima wait in dmin.  After the last chunk the
// owner lane of a document folds e_t in vector order, and the emission is the fifth form's.
// ---------------------------------------------------------------------------------------------
#define HX_LATE_LDS(cap) ((size_t)(cap) * 36)
#define HX_DOCS_CHUNK 1024
#define HX_DOCS_LDS(n_in, n_vecs) ((size_t)HX_DOCS_MAX_IN * 28 + (size_t)HX_DOCS_CHUNK * 8 + (size_t)(n_in) * (n_vecs) * 4)
template <int KIND>
__device__ __forceinline__ void late_interaction(const DevView &v, const DiverseLists &d, float *yq, unsigned char *tab, int lane) {
    constexpr int LPC = (KIND == HNSW_VEC_QUANT8) ? 2 : 1;
    constexpr int CHUNK = 64 / LPC;
    constexpr uint32_t INF_BITS = 0x7F800000u, NONE = 0xFFFFFFFFu, LATER = 0x80000000u;
    const int h = (LPC == 2) ? (lane & 1) : 0;
    const bool docs = d.docs != 0;  // (a kernel argument: every branch on it is the wave's)
    const uint32_t q = blockIdx.x, T = d.n_vecs, pool = d.pool, n_out = d.n_out;
    if (q >= d.nq || T > HX_LATE_MAX_VECS) return;  // (the launcher's limits, here and below)
    if (docs ? (pool > HX_DOCS_MAX_IN || n_out > pool || d.rows_cap == 0 || d.rows_cap > HX_DOCS_MAX_ROWS)
             : (pool > HX_LATE_MAX_CANDS || T * pool > HX_LATE_MAX_CANDS || n_out > HX_LATE_MAX_DOCS || n_out > T * pool))
        return;
    const uint32_t total = docs ? pool : T * pool, cap = (total + 63u) & ~63u;
    uint32_t *sid, *cid, *cdoc, *dlab, *dmin, *dsize, *dstart, *dpre;
    float *dsum;
    u64 *dbest;
    if (docs) {
        dbest = reinterpret_cast<u64 *>(tab);
        dlab = reinterpret_cast<uint32_t *>(dbest + HX_DOCS_MAX_IN);
        dstart = dlab + HX_DOCS_MAX_IN, dsize = dstart + HX_DOCS_MAX_IN, dpre = dsize + HX_DOCS_MAX_IN;
        dsum = reinterpret_cast<float *>(dpre + HX_DOCS_MAX_IN);
        cid = dpre + 2 * HX_DOCS_MAX_IN, cdoc = cid + HX_DOCS_CHUNK, dmin = cdoc + HX_DOCS_CHUNK;
        sid = cid;  // (the labels as loaded: they have served before the first chunk is laid out)
    } else {
        sid = reinterpret_cast<uint32_t *>(tab);
        cid = sid + cap, cdoc = cid + cap, dlab = cdoc + cap, dmin = dlab + cap;
        dsum = reinterpret_cast<float *>(dmin + cap);
        dsize = dmin + 2 * cap;
        dbest = reinterpret_cast<u64 *>(dsize + cap);  // (28 * cap bytes in: 8-byte aligned)
        dstart = dpre = nullptr;
    }
    const size_t l0 = (size_t)q * T, in0 = (size_t)q * total, out0 = (size_t)q * n_out;
    hnsw_query_stats st;
    st.n_dist = st.n_exp = st.sum_deg = 0;
    st.status = HNSW_OK;
    if (d.stats) {
        if (docs) {
            st = d.stats[q];  // (one record per list)
        } else {
            for (uint32_t t = 0; t < T; t++) {  // (wave-uniform: the wrapping sums, the first status that is not OK)
                const hnsw_query_stats s = d.stats[l0 + t];
                st.n_dist += s.n_dist, st.n_exp += s.n_exp, st.sum_deg += s.sum_deg;
                if (st.status == HNSW_OK) st.status = s.status;
            }
        }
    }
    const bool ok = st.status == HNSW_OK;  // a failed query has no present entry: count 0 and padded rows
    uint32_t count = 0, unique = 0, n_docs = 0, n_rows = 0;  // wave-uniform
    bool walk = false;                                       // the passes run
    if (docs) {
        bool bad = false;  // a NaN in any of the T vectors, before any index row is read
        if (ok) {
            const float *qv = d.queries + l0 * v.dim;
            for (uint32_t e = lane; e < T * v.dim; e += 64) {
                const float x = qv[e];
                bad |= (x != x);
            }
        }
        const bool nan = __ballot(bad) != 0;
        if (nan) st.status = HNSW_ERR_NAN_INPUT;
        const uint32_t cnt = ok && !nan ? (d.counts ? min(d.counts[q], pool) : pool) : 0u;  // the present entries: a prefix
        for (uint32_t j = lane; j < cap; j += 64) sid[j] = j < cnt ? d.ids[in0 + j] : 0u;
        wave_fence();
        const uint64_t *keys = d.doc_keys;
        for (uint32_t base = 0; base < cnt; base += 64) {  // the distinct present labels that have a row, in list order
            const uint32_t j = base + lane, lab = sid[j], end = min(cnt, base + 64);
            bool dup = false;
            for (uint32_t i = 0; i < end; i += 4) {  // (a word at or behind cnt is never before a present j)
                const uint4 w = *reinterpret_cast<const uint4 *>(sid + i);
                dup |= (w.x == lab && i < j) | (w.y == lab && i + 1 < j) | (w.z == lab && i + 2 < j) | (w.w == lab && i + 3 < j);
            }
            const bool live = j < cnt && !dup;
            // the slice of the label's keys: [first key >= label << 32, first key > label << 32 | 0xFFFFFFFF)
            const u64 klo = (u64)lab << 32, khi = klo | 0xFFFFFFFFull;
            u64 a = 0, b = live ? d.n_doc_keys : 0;
            while (a < b) {
                const u64 m = (a + b) >> 1;
                if (keys[m] < klo) a = m + 1; else b = m;
            }
            const u64 first = a;
            b = live ? d.n_doc_keys : first;
            while (a < b) {
                const u64 m = (a + b) >> 1;
                if (keys[m] <= khi) a = m + 1; else b = m;
            }
            const uint32_t size = (uint32_t)(a - first);  // (ids are 32-bit and distinct: below 2^32)
            const bool has = live && size != 0;           // a label without a row is not a document
            const u64 bal = __ballot(has);
            if (has) {
                const uint32_t g = n_docs + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1));
                dlab[g] = lab;
                dstart[g] = (uint32_t)first;
                dsize[g] = size;
                dpre[g] = min(size, d.rows_cap);  // (summed below)
                dbest[g] = KEY_INVALID;
            }
            n_docs += (uint32_t)__builtin_popcountll(bal);
        }
        wave_fence();
        for (uint32_t base = 0; base < n_docs; base += 64) {  // dpre[g] = the scored rows of the documents before g
            const uint32_t g = base + lane, x = g < n_docs ? dpre[g] : 0u;
            uint32_t incl = x;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= o) incl += y;
            }
            if (g < n_docs) dpre[g] = n_rows + incl - x;
            n_rows += (uint32_t)__shfl((int)incl, 63);
        }
        for (uint32_t i = lane; i < n_docs * T; i += 64) dmin[i] = INF_BITS;
        wave_fence();
        walk = n_rows != 0;
    } else {
        bool beyond = false;
        for (uint32_t j = lane; j < cap; j += 64) {
            uint32_t id = HX_EMPTY_SLOT;
            if (j < total) {
                const uint32_t t = j / pool, jj = j - t * pool;
                const uint32_t raw = d.ids[in0 + j];
                const bool present = ok && (d.counts ? jj < min(d.counts[l0 + t], pool) : raw != HX_EMPTY_SLOT);
                beyond |= present && raw >= v.n_points;
                id = present ? raw : HX_EMPTY_SLOT;
            }
            sid[j] = id;
        }
        wave_fence();
        if (__ballot(beyond)) {
            st.status = HNSW_ERR_ARG;  // no row of the index is read for this query
        } else if (ok) {
            walk = true;
            for (uint32_t base = 0; base < total; base += 64) {  // the distinct present ids, in table order, to cid[0 .. unique)
                const uint32_t j = base + lane, id = sid[j], end = min(total, base + 64);
                bool dup = false;
                for (uint32_t i = 0; i < end; i += 4) {  // (the table is EMPTY from `total` to cap)
                    const uint4 w = *reinterpret_cast<const uint4 *>(sid + i);
                    dup |= (w.x == id && i < j) | (w.y == id && i + 1 < j) | (w.z == id && i + 2 < j) | (w.w == id && i + 3 < j);
                }
                const bool live = id != HX_EMPTY_SLOT && !dup;
                const u64 b = __ballot(live);
                if (live) cid[unique + __builtin_popcountll(b & ((1ull << lane) - 1))] = id;
                unique += (uint32_t)__builtin_popcountll(b);
            }
            wave_fence();
            uint32_t *clab = sid;  // (the entries have served)
            const uint64_t label_len = d.labels ? d.label_len : 0;
            for (uint32_t j = lane; j < unique; j += 64) {
                const uint32_t c = cid[j];
                clab[j] = c < label_len ? d.labels[c] : 0u;
            }
            wave_fence();
            for (uint32_t base = 0; base < unique; base += 64) {  // the distinct labels, in candidate order, to dlab[0 .. n_docs)
                const uint32_t j = base + lane, lab = clab[j], end = min(unique, base + 64);
                const bool live = j < unique;
                uint32_t fi = NONE;  // the first candidate before j with j's label
                for (uint32_t i = 0; i < end; i += 4) {  // (a word at or behind `unique` is never before a live j)
                    const uint4 w = *reinterpret_cast<const uint4 *>(clab + i);
                    fi = min(fi, w.x == lab && i < j ? i : NONE);
                    fi = min(fi, w.y == lab && i + 1 < j ? i + 1 : NONE);
                    fi = min(fi, w.z == lab && i + 2 < j ? i + 2 : NONE);
                    fi = min(fi, w.w == lab && i + 3 < j ? i + 3 : NONE);
                }
                const bool first = live && fi == NONE;
                const u64 b = __ballot(first);
                if (first) {
                    const uint32_t g = n_docs + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1));
                    cdoc[j] = g;
                    dlab[g] = lab;
                    dmin[g] = INF_BITS;
                    dsum[g] = 0.0f;
                    dsize[g] = 0u;
                    dbest[g] = KEY_INVALID;
                } else if (live) {
                    cdoc[j] = fi | LATER;  // (resolved below, once the first's document is numbered)
                }
                n_docs += (uint32_t)__builtin_popcountll(b);
            }
            wave_fence();
            for (uint32_t j = lane; j < unique; j += 64) {
                uint32_t g = cdoc[j];
                if (g & LATER) {
                    g = cdoc[g & ~LATER];  // (a first's entry: not rewritten here)
                    cdoc[j] = g;
                }
                atomicAdd(&dsize[g], 1u);
            }
            wave_fence();
        }
    }
    if (walk) {
        bool nan = false;                // wave-uniform
        uint32_t c0 = 0, n_e = unique;  // the entries of cid / cdoc: the candidates, or the chunk in hand
        do {
            if (docs) {  // rows c0 .. c0 + n_e of the documents' scored rows, in document order
                n_e = min((uint32_t)HX_DOCS_CHUNK, n_rows - c0);
                for (uint32_t j = lane; j < n_e; j += 64) {
                    const uint32_t r = c0 + j;
                    uint32_t lo = 0, hi = n_docs;  // the last document with dpre <= r (dpre[0] is 0; no scored size is 0)
                    while (hi - lo > 1) {
                        const uint32_t m = (lo + hi) >> 1;
                        if (dpre[m] <= r) lo = m; else hi = m;
                    }
                    cdoc[j] = lo;
                    // the id is the key's low word (little-endian)
                    cid[j] = reinterpret_cast<const uint32_t *>(d.doc_keys)[2 * ((u64)dstart[lo] + (r - dpre[lo]))];
                }
                wave_fence();
            }
            const uint32_t stride = docs ? T : 1u;
            for (uint32_t t = 0; t < T; t++) {
                if (!stage_query<KIND>(v, d.queries + (l0 + t) * v.dim, yq, lane)) {  // (never in the seventh form)
                    nan = true;
                    break;
                }
                const uint32_t col = docs ? t : 0u;
                for (uint32_t base = 0; base < n_e; base += CHUNK) {
                    const uint32_t j = base + lane / LPC;
                    const uint32_t id = j < n_e ? cid[j] : 0u;
                    // (a key's id is below the index length the keys were made for: the snapshot's)
                    const bool active = j < n_e && id < v.n_points;
                    const float dist = dist_any_dim<KIND>(v, active ? id : 0u, active, h, yq);
                    if (active && h == 0 && dist == dist) {  // (a NaN leaves the minimum and the best row as they are)
                        const uint32_t bits = __builtin_bit_cast(uint32_t, dist), g = cdoc[j];
                        atomicMin(&dmin[g * stride + col], bits);
                        atomicMin(&dbest[g], ((u64)bits << 32) | id);
                    }
                }
                wave_fence();
                if (!docs) {
                    for (uint32_t g = lane; g < n_docs; g += 64) {
                        const float m = __builtin_bit_cast(float, dmin[g]);
                        const float e = d.mode == HNSW_LATE_SUM_SQ ? m * m : m;
                        dsum[g] = t == 0 ? e : dsum[g] + e;
                        dmin[g] = INF_BITS;
                    }
                    wave_fence();
                }
            }
            c0 += HX_DOCS_CHUNK;
        } while (docs && !nan && c0 < n_rows);
        if (nan) {
            st.status = HNSW_ERR_NAN_INPUT;
            n_docs = 0;
        } else {
            if (docs) {  // the owner lane of a document folds its minima in vector order
                for (uint32_t g = lane; g < n_docs; g += 64) {
                    float s = 0.0f;
                    for (uint32_t t = 0; t < T; t++) {
                        const float m = __builtin_bit_cast(float, dmin[g * T + t]);
                        const float e = d.mode == HNSW_LATE_SUM_SQ ? m * m : m;
                        s = t == 0 ? e : s + e;
                    }
                    dsum[g] = s;
                }
                wave_fence();
            }
            for (uint32_t t = 0; t < n_out; t++) {
                u64 mine = KEY_INVALID;
                uint32_t mg = 0;
                for (uint32_t g = lane; g < n_docs; g += 64) {
                    const float score = dsum[g];
                    if (score != score) continue;  // a NaN score is never returned (nor is a document twice: below)
                    const uint32_t u = __builtin_bit_cast(uint32_t, score == 0.0f ? 0.0f : score);  // -0 == +0: one key
                    const u64 key = ((u64)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | dlab[g];
                    if (key < mine) mine = key, mg = g;
                }
                u64 best = mine;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const u64 other = ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o) << 32) |
                                      (uint32_t)__shfl_xor((int)(uint32_t)best, o);
                    best = other < best ? other : best;
                }
                if (best == KEY_INVALID) break;  // nothing left
                if (mine == best) {  // (labels are distinct: one document of one lane)
                    d.out_ids[out0 + t] = (uint32_t)best;
                    d.out_dists[out0 + t] = dsum[mg];
                    if (d.best_out) d.best_out[out0 + t] = (uint32_t)dbest[mg];
                    if (d.sizes_out) d.sizes_out[out0 + t] = dsize[mg];
                    dsum[mg] = __builtin_nanf("");
                }
                wave_fence();
                count = t + 1;
            }
        }
    }
    for (uint32_t s = count + lane; s < n_out; s += 64) {
        d.out_ids[out0 + s] = 0u;
        d.out_dists[out0 + s] = __builtin_inff();
        if (d.best_out) d.best_out[out0 + s] = HX_EMPTY_SLOT;
        if (d.sizes_out) d.sizes_out[out0 + s] = 0u;
    }
    if (lane == 0) {
        if (d.out_counts) d.out_counts[q] = count;
        if (d.n_docs_out) d.n_docs_out[q] = n_docs;
        if (d.out_stats) d.out_stats[q] = st;
    }
}

// ---------------------------------------------------------------------------------------------
// The kernel's sixth form (DiverseLists with table != nullptr, device_index.h): query blockIdx.x's
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
                // (read as a HIP uint4 from the swizzled address: coop_rows.inc)
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
    // (f16 rows take a lane per row at every width: measured faster)
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

// ---------------------------------------------------------------------------------------------
// The kernel's ninth form (DiverseLists with boost != 0, device_index.h): query blockIdx.x's
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

// ---------------------------------------------------------------------------------------------
// The kernel's eighth form (DiverseLists with hybrid != 0, device_index.h): query blockIdx.x's
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

int launch_diversify(const DevView &v, const DiverseLists &d, hipStream_t stream) {
    if (d.nq == 0) return HNSW_OK;
    if (d.n_out == 0 || d.n_out > d.pool || d.pool > HX_DIVERSE_POOL_MAX || !(d.lambda >= 0.0f && d.lambda <= 1.0f) ||
        d.nq > 0x7FFFFFFFu || !d.ids || !d.dists || !d.out_ids || !d.out_dists || (d.stats != nullptr) != (d.out_stats != nullptr)) {
        set_error("diversify: needs 1 <= n_out <= pool <= %d, lambda in [0, 1], at most 2^31 - 1 queries, the lists and the "
                  "outputs", HX_DIVERSE_POOL_MAX);
        return HNSW_ERR_ARG;
    }
    return launch_checked({"diversify kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), query_lds_bytes(v) + HX_DIVERSE_LDS, stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    return launch_checked({"compose rows kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(nq), dim3(64), 0, stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    return launch_checked({"fuse lists kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), query_lds_bytes(v) + HX_DIVERSE_LDS, stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    return launch_checked({"late interaction kernel launch", "late interaction: the staged vector and the table need %zu bytes of LDS"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), query_lds_bytes(v) + HX_LATE_LDS(cap), stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    return launch_checked({"score documents kernel launch", "score documents: the staged vector and the tables need %zu bytes of LDS"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), query_lds_bytes(v) + HX_DOCS_LDS(d.pool, d.n_vecs), stream, v,
                          static_cast<const float *>(nullptr), static_cast<const uint32_t *>(nullptr), (uint64_t)0,
                          static_cast<float *>(nullptr), static_cast<int32_t *>(nullptr), d);
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
    return launch_checked({"fuse ranked kernel launch"},
                          v.kind == HNSW_VEC_QUANT8 ? hx_distance_kernel<HNSW_VEC_QUANT8> : hx_distance_kernel<HNSW_VEC_F32>,
                          dim3(d.nq), dim3(64), query_lds_bytes(v) + HX_HYBRID_LDS, stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    DevView v{};  // (the form reads nothing of it)
    v.kind = HNSW_VEC_F32;
    return launch_checked({"refine kernel launch"}, hx_distance_kernel<HNSW_VEC_F32>, dim3(d.nq), dim3(64),
                          refine_lds_bytes(d.full_dim, d.pool), stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
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
    DevView v{};  // (the form reads nothing of it)
    v.kind = HNSW_VEC_F32;
    return launch_checked({"boost kernel launch"}, hx_distance_kernel<HNSW_VEC_F32>, dim3(d.nq), dim3(64),
                          boost_lds_bytes(d.full_dim, d.pool), stream, v, static_cast<const float *>(nullptr),
                          static_cast<const uint32_t *>(nullptr), (uint64_t)0, static_cast<float *>(nullptr),
                          static_cast<int32_t *>(nullptr), d);
}

}  // namespace hx
