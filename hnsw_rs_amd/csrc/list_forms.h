// list_forms.h -- the list forms of hx_distance_kernel (exact_scan.hip): the post-process stages that work on candidate
// lists in HBM, one wave per query.  DiverseLists is the one record all of them are launched under (a kernel argument,
// passed by value: its layout is the kernel's), a form is selected by one field of it, and every form's paragraph below
// says which fields it reads.  Then the forms' limits and their launchers.  A form's body and LDS layout: form_*.inc.
#pragma once

#include "device_index.h"

namespace hx {

// The second source form of hx_distance_kernel (hnsw_diversify_device), selected by n_out != 0
// (zero in launch_distance_batch's launches, which read nothing of this record): ONE candidate list per query,
// ids[q][j] / dists[q][j], j < pool, counts[q] (nullptr: an entry is present iff its id is not the pad) and stats[q]
// (nullptr: none are read or written), re-ranked by maximal marginal relevance -- THE SELECTION of
// include/hnsw_mi355x.h -- into out_ids / out_dists / out_gaps [q][n_out] (out_gaps may be nullptr), the number selected
// into out_counts[q] (may be nullptr), the stats record into out_stats[q] (with stats), its status HNSW_ERR_ARG when a
// present id is at or beyond the index length.  The kernel's q, ids, k, out and status_out are not read.
#define HX_DIVERSE_POOL_MAX 256  // candidates per query: ids, distance bits and running minima in 3 KiB of LDS
struct DiverseLists {
    const uint32_t *ids;
    const float *dists;
    const uint32_t *counts;
    const hnsw_query_stats *stats;
    uint32_t pool, n_out;
    float lambda;
    uint32_t nq;
    uint32_t *out_ids;
    float *out_dists, *out_gaps;
    uint32_t *out_counts;
    hnsw_query_stats *out_stats;
    // The third source form (hnsw_compose_rows_device), selected by width != 0 (zero in every
    // other launch, whose kernels read nothing below): query q's row rows_out[q][dim] is THE COMPOSED QUERY of
    // include/hnsw_mi355x.h over the stored rows ids[q][s], s < width (pad HX_EMPTY_SLOT), with weights[q][s] (nullptr:
    // every weight 1.0f); row_status[q] (may be nullptr) is HNSW_OK, or HNSW_ERR_ARG for a query without a present slot
    // or with a present id at or beyond the index length, whose row is all zeros.  Of the fields above the form reads
    // ids and nq alone.
    uint32_t width;
    // The fourth source form (hnsw_fuse_lists_device), selected by n_vecs != 0 (zero in every other
    // launch) and looked at before n_out: query q has n_vecs vectors queries[q][t][dim] with weights[q][t] (nullptr: no
    // multiply) and n_vecs candidate lists ids[q][t][j], j < pool, counts[q][t] and stats[q][t] (either may be nullptr),
    // n_vecs * pool <= HX_DIVERSE_POOL_MAX.  THE FUSION of include/hnsw_mi355x.h under `mode` goes to out_ids / out_dists
    // (the scores) [q][n_out], out_counts[q], unique_out[q] (either may be nullptr) and out_stats[q] (with stats).  dists,
    // lambda, out_gaps and the third form's outputs are not read.
    uint32_t n_vecs;
    const float *weights;
    float *rows_out;
    int32_t *row_status;
    uint32_t mode;
    // The fifth source form (hnsw_late_interaction_device), selected by late != 0 (zero in every
    // other launch) and looked at FIRST: query q has n_vecs vectors queries[q][t][dim] and n_vecs candidate lists
    // ids[q][t][j], j < pool, counts[q][t] and stats[q][t] (either may be nullptr), n_vecs * pool <= HX_LATE_MAX_CANDS;
    // labels[id], id < label_len, is the label column (nullptr: every label 0).  THE LATE INTERACTION of
    // include/hnsw_mi355x.h under `mode` goes to out_ids (the documents' labels) / out_dists (their scores) [q][n_out],
    // best_out / sizes_out [q][n_out], out_counts[q], n_docs_out[q] (all four may be nullptr) and out_stats[q] (with
    // stats).  dists, lambda, weights, out_gaps, unique_out and the third form's outputs are not read.
    uint32_t late;
    const float *queries;
    uint32_t *unique_out;
    const uint32_t *labels;
    uint64_t label_len;
    uint32_t *best_out, *sizes_out, *n_docs_out;
    // The sixth source form (hnsw_refine_device), selected by table != nullptr (null in every other
    // launch) and looked at FIRST; it reads nothing of the DevView.  Query q has ONE candidate list ids[q][j], j < pool,
    // counts[q] and stats[q] (either may be nullptr) and a full row queries[q][full_dim]; table is table_rows rows of
    // full_dim elements of table_dtype (HX_ROWS_F32: f32, HX_ROWS_F16: IEEE binary16, widened exactly).  THE REFINEMENT of
    // include/hnsw_mi355x.h goes to out_ids / out_dists [q][n_out], out_counts[q] (may be nullptr) and out_stats[q] (with
    // stats).  lane_rows != 0: a lane per row whatever the width (the switch HNSW_MI355X_REFINE_LANE_ROWS, A/B runs).
    // Nothing else above is read.
    const void *table;
    uint64_t table_rows;
    uint32_t full_dim, table_dtype, lane_rows;
    // The seventh source form (hnsw_score_documents_device), selected by docs != 0 (zero in every
    // other launch) and looked at FIRST of all: query q has n_vecs vectors queries[q][t][dim] and ONE list of labels
    // ids[q][j], j < pool (the list's length n_in), counts[q] (nullptr: every entry is present -- every uint32 is a label)
    // and stats[q] (may be nullptr); doc_keys[i], i < n_doc_keys, is the document index: the keys label << 32 | id of the
    // undeleted ids, ascending, so that a label's rows are a slice of it.  THE DOCUMENT SCORING of include/hnsw_mi355x.h
    // under `mode`, every document over its min(size, rows_cap) lowest ids, goes to the fifth form's outputs.  labels,
    // label_len and everything the fifth form does not read are not read.
    uint32_t docs, rows_cap;
    const uint64_t *doc_keys;
    uint64_t n_doc_keys;
    // The eighth source form (hnsw_fuse_ranked_device), selected by hybrid != 0 (zero in every other
    // launch; 1 + the mode) and looked at before ALL others: query q has up to 1 + HX_HYBRID_MAX_EXT ranked lists -- the
    // optional dense one ids[q][j], j < pool, counts[q] and stats[q] (ids nullptr: none; either of the others may be
    // nullptr), then n_ext external ones ext_ids / ext_scores [q][e][j], j < ext_width, ext_counts[q][e] (scores and counts
    // may be nullptr) -- weights[q][1 + n_ext] (nullptr: none), absent[e] by value, rank_constant, and optionally its row
    // queries[q][dim].  The filter: deny / deny_bits (the deleted ids' mask, nullptr: nothing deleted), rowed != 0: the
    // rows `allow` of mask_words words each, n_masks of them, allow_bits ids each, query q under row mask_of[q] (nullptr:
    // row 0) or HNSW_MASK_NONE; range_lo / range_hi [q] (nullptr: no range) over labels / label_len.  THE RANK FUSION of
    // include/hnsw_mi355x.h goes to out_ids / out_dists (the scores) / out_gaps (D of every hit; may be nullptr)
    // [q][n_out], out_counts[q], unique_out[q], dropped_out[q] (all three may be nullptr) and out_stats[q] (with stats).
    uint32_t hybrid, n_ext, ext_width, rank_constant;
    const uint32_t *ext_ids;
    const float *ext_scores;
    const uint32_t *ext_counts;
    float absent[7];  // (HX_HYBRID_MAX_EXT)
    uint32_t rowed;
    const uint64_t *deny, *allow;
    uint64_t deny_bits, allow_bits, mask_words;
    const uint32_t *mask_of, *range_lo, *range_hi;
    uint32_t n_masks;
    uint32_t *dropped_out;
    // The ninth source form (hnsw_boost_device), selected by boost != 0 (zero in every other launch:
    // no other launcher sets it, and every record starts zeroed; 1: one weight row for all queries, 2: a row per query)
    // and looked at before ALL others; it reads nothing of the DevView.  Query q has ONE candidate list ids[q][j] /
    // dists[q][j], j < pool, counts[q] and stats[q] (either may be nullptr) and a weight row weights[1 + full_dim]; table
    // is table_rows rows of full_dim attributes of table_dtype, as in the sixth form.  THE BOOST of
    // include/hnsw_mi355x.h goes to out_ids / out_dists (the scores) / out_gaps (the incoming distance of every hit; may
    // be nullptr) [q][n_out], out_counts[q] (may be nullptr) and out_stats[q] (with stats).  Nothing else above is read.
    uint32_t boost;
};
#define HX_HYBRID_MAX_EXT 7  // external lists per query of the rank fusion
#define HX_BOOST_POOL_MAX 1024  // candidates per boosted query: a key of 8 bytes each in LDS
#define HX_BOOST_MAX_ATTRS 32   // attributes per id: an f32 row is at most one 128-byte line
#define HX_ROWS_F32 0
#define HX_ROWS_F16 1
#define HX_REFINE_POOL_MAX 1024  // candidates per refined query: a key of 8 bytes each in LDS
#define HX_REFINE_MAX_DIM 4096   // elements of a full row: the staged query is at most 16 KiB of LDS
#define HX_FROM_ROWS_MAX_TERMS 64  // slots per composed query: one lane each
#define HX_MULTI_MAX_VECS 16       // vectors per fused query
#define HX_LATE_MAX_VECS 32        // vectors per late-interaction query
#define HX_LATE_MAX_CANDS 1024     // its candidates, n_vecs * pool: 36 bytes of LDS each
#define HX_LATE_MAX_DOCS 256       // the documents it returns
#define HX_DOCS_MAX_IN 256         // labels per list of the document scoring: 28 bytes of LDS each, and n_vecs minima
// rows scored per document: the prefix sums of the scored sizes are 32-bit words in LDS, and HX_DOCS_MAX_IN documents of
// this many rows total 2^28
#define HX_DOCS_MAX_ROWS (1u << 20)
// the selection of d.nq candidate lists (1 <= n_out <= pool <= HX_DIVERSE_POOL_MAX, lambda in [0, 1]): ONE launch of
// hx_distance_kernel in its second form, one wave per query
int launch_diversify(const DevView &v, const DiverseLists &d, hipStream_t stream);
// nq composed queries of `width` slots each (1 <= width <= HX_FROM_ROWS_MAX_TERMS) into d_rows [nq][v.dim]: ONE launch of
// hx_distance_kernel in its third form, one wave per query.  d_weights and d_status may be nullptr.
int launch_compose_rows(const DevView &v, uint32_t nq, uint32_t width, const uint32_t *d_src_ids, const float *d_weights,
                        float *d_rows, int32_t *d_status, hipStream_t stream);
// the fusion of d.nq queries of d.n_vecs lists each (1 <= n_vecs <= HX_MULTI_MAX_VECS, 1 <= n_out <= pool, n_vecs * pool <=
// HX_DIVERSE_POOL_MAX, mode 0 or 1): ONE launch of hx_distance_kernel in its fourth form, one wave per query
int launch_fuse_lists(const DevView &v, const DiverseLists &d, hipStream_t stream);
// the late interaction of d.nq queries of d.n_vecs lists each (1 <= n_vecs <= HX_LATE_MAX_VECS, n_vecs * pool <=
// HX_LATE_MAX_CANDS, 1 <= n_out <= min(n_vecs * pool, HX_LATE_MAX_DOCS), mode 0 or 1): ONE launch of hx_distance_kernel in
// its fifth form, one wave per query; sets d.late itself
int launch_late_interaction(const DevView &v, DiverseLists d, hipStream_t stream);
// the document scoring of d.nq lists of d.pool labels each (1 <= n_vecs <= HX_LATE_MAX_VECS, 1 <= n_out <= pool <=
// HX_DOCS_MAX_IN, 1 <= rows_cap <= HX_DOCS_MAX_ROWS, mode 0 or 1) over d.doc_keys: ONE launch of hx_distance_kernel in its
// seventh form, one wave per query; sets d.docs itself
int launch_score_documents(const DevView &v, DiverseLists d, hipStream_t stream);
// the rank fusion of d.nq queries (d.mode 0: reciprocal rank fusion, 1: linear; total = (d.ids ? pool : 0) + n_ext *
// ext_width <= HX_DIVERSE_POOL_MAX, n_ext <= HX_HYBRID_MAX_EXT, 1 <= n_out <= total): ONE launch of hx_distance_kernel in
// its eighth form, one wave per query; sets d.hybrid from d.mode itself
int launch_fuse_ranked(const DevView &v, DiverseLists d, hipStream_t stream);
// the refinement of d.nq candidate lists against d.table (1 <= n_out <= pool <= HX_REFINE_POOL_MAX, 1 <= full_dim <=
// HX_REFINE_MAX_DIM, a dtype of the two): ONE launch of hx_distance_kernel<HNSW_VEC_F32> in its sixth form under a zeroed
// view, one wave per query; takes no handle and sets d.lane_rows from the switch itself
int launch_refine(DiverseLists d, hipStream_t stream);
// the boost of d.nq candidate lists by the attributes of d.table (1 <= n_out <= pool <= HX_BOOST_POOL_MAX, 1 <= full_dim <=
// HX_BOOST_MAX_ATTRS, a dtype of the two; d.mode 0: d.weights is one row of 1 + full_dim for every query, 1: a row per
// query): ONE launch of hx_distance_kernel<HNSW_VEC_F32> in its ninth form under a zeroed view, one wave per query; takes
// no handle and sets d.boost from d.mode itself
int launch_boost(DiverseLists d, hipStream_t stream);

}  // namespace hx
