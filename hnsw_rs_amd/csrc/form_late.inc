// form_late.inc -- included inside namespace hx by exact_scan.hip, after search_common.h and launch.h:
// hx_distance_kernel's fifth and seventh forms: late interaction over candidates, and over named documents.
// ---------------------------------------------------------------------------------------------
// The kernel's fifth form (DiverseLists with late != 0, list_forms.h; DESIGN.md section 29): query blockIdx.x's
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
// The kernel's seventh form (DiverseLists with docs != 0; DESIGN.md section 32) is the same function: query blockIdx.x's
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
